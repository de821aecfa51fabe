// msm_buckets.cuh -- the parts of a Pippenger multi-scalar multiplication that do not depend on the curve: the signed window
// recoding of a scalar, the bucket pass of one workgroup, and the carve of the workspace regions that pass works on.
// Included by the twisted-Edwards unit (msm.cuh, once per base field), the secp256r1 unit (k_p256_msm.hip) and the BLS12-381 G1
// unit (g1_digits.cuh); it knows no field and no group law.  A unit hands msm_bucket_pass a policy struct G:
//   types      Acc (bucket accumulator), Aff (affine input point)
//   constants  BLOCK (lanes per workgroup), BPL (buckets per lane, 1 or 2: BLOCK * BPL buckets per window), PT_WORDS (words of a
//              stored Acc), AFF_STRIDE (words between the affine slots), IDX_BITS (bits of a point index inside its group),
//              HIST_LOADS / SCATTER_LOADS (independent digit loads per trip of the histogram / of the scatter)
//   functions  identity(), load(src), store(dst, acc), aff_load(src), aff_identity(), madd(acc, aff, neg), add(a, b), and for
//              BPL == 2 dbl(a)
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#ifndef VRF_HD
#define VRF_HD __host__ __device__ __forceinline__
#endif

namespace vrf {

// ------------------------------------------------------------------------------- digits
// signed radix-2^C digits of the little-endian integer k < 2^(C W - 1), digit w of point i at digits[w * n + i]: each in
// [-2^(C-1) + 1, 2^(C-1)].  `negate` flips every digit (callers that subtract the term); `zero` writes zeros: the point
// takes no part.
template <int C>
VRF_HD void msm_recode_windows(int16_t* digits, size_t n, size_t i, int W, const uint32_t k[8], bool negate, bool zero) {
  uint32_t carry = 0;
#pragma unroll 1
  for (int w = 0; w < W; ++w) {
    const int bit = w * C, wi = bit >> 5, sh = bit & 31;
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (j == wi) lo = k[j];
      if (j == wi + 1) hi = k[j];
    }
    uint32_t v = (sh ? ((lo >> sh) | (hi << (32 - sh))) : lo) & ((1u << C) - 1);
    v += carry;
    int d = (int)v;
    carry = 0;
    if (v > (1u << (C - 1))) { d = (int)v - (1 << C); carry = 1; }
    digits[(size_t)w * n + i] = (int16_t)(zero ? 0 : negate ? -d : d);
  }
}

// canonical scalar k (< r, R::r32(j) = word j of r) -> W folded digits: k > r - k is replaced by r - k with the sign of the
// term flipped, so the recoded integer is below 2^(C W - 1) and the top window never carries out
template <int C, int W, class R>
VRF_HD void msm_write_folded_digits(int16_t* digits, size_t n, size_t i, const uint32_t k_in[8], bool negate, bool zero) {
  uint32_t k[8], nk[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) k[j] = zero ? 0u : k_in[j];
  {
    uint32_t borrow = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint64_t d = (uint64_t)R::r32(j) - k[j] - borrow;
      nk[j] = (uint32_t)d;
      borrow = (uint32_t)(d >> 63);
    }
  }
  bool flip = false, decided = false;
#pragma unroll
  for (int j = 7; j >= 0; --j)
    if (!decided && nk[j] != k[j]) { flip = nk[j] < k[j]; decided = true; }
  flip = flip && !zero;
#pragma unroll
  for (int j = 0; j < 8; ++j) k[j] = flip ? nk[j] : k[j];
  msm_recode_windows<C>(digits, n, i, W, k, flip != negate, false);      // zero: k is 0 already
}

// ------------------------------------------------------------------------------- bucket pass
// What one workgroup works on: one window of one point group.
struct MsmBucketJob {
  const int16_t* digits;   // the window's digits of the group's points
  const uint32_t* pts;     // the group's affine slots
  uint32_t count;          // points in the group (< 2^IDX_BITS)
  uint32_t* list;          // [count rounded up to BLOCK] bucket-sorted entries, lane-transposed
  uint32_t* heads;         // [BLOCK][PT_WORDS] first-run partial sums
  uint32_t* out;           // [PT_WORDS] receives the window sum  sum_j j B_j
};

template <class G>
constexpr size_t msm_bucket_lds_bytes() {      // buckets | counts | cursors | per-wave totals
  return ((size_t)G::BLOCK * G::BPL * G::PT_WORDS + 2 * (size_t)G::BLOCK * G::BPL + 16) * 4;
}
constexpr int msm_log2(int x) { return x <= 1 ? 0 : 1 + msm_log2(x >> 1); }

// The BLOCK * BPL buckets of the window live in LDS (`lds`: msm_bucket_lds_bytes<G>() bytes).  The workgroup counting-sorts
// its points by bucket, then the sorted list is cut into BLOCK EQUAL chunks, one per lane: every lane performs the same number
// of mixed additions whatever the digit distribution.  A lane keeps the running sum of the current bucket in registers and
// flushes it when the bucket changes: runs that start inside the chunk go straight to their LDS bucket (exactly one lane owns
// the start of a bucket), the first run of a chunk -- possibly the continuation of the previous lane's bucket -- is parked as
// a "head" and merged afterwards by the first lane of each chain.  Then the buckets are reduced to sum_j j B_j inside the
// workgroup.  Every lane of the workgroup must call it (barriers).
template <class G>
__device__ __forceinline__ void msm_bucket_pass(const MsmBucketJob& job, uint32_t* lds) {
  using Acc = typename G::Acc;
  using Aff = typename G::Aff;
  constexpr int BLOCK = G::BLOCK, BPL = G::BPL, BUCKETS = BLOCK * BPL, PT = G::PT_WORDS, LOG2_BLOCK = msm_log2(BLOCK);
  constexpr uint32_t IDX_MASK = (1u << G::IDX_BITS) - 1, NONE = 0xffffffffu;
  static_assert((1 << LOG2_BLOCK) == BLOCK && BLOCK % 64 == 0 && BLOCK / 64 <= 16 && (BPL == 1 || BPL == 2), "workgroup shape");
  static_assert(G::IDX_BITS + msm_log2(BUCKETS) <= 31, "list entry: index | bucket | sign");
  uint32_t* bucket = lds;                                   // [BUCKETS][PT] bucket accumulators
  uint32_t* counts = lds + BUCKETS * PT;                    // [BUCKETS] bucket sizes
  uint32_t* cursor = counts + BUCKETS;                      // [BUCKETS] scatter cursors, later head bucket ids
  uint32_t* wsum = cursor + BUCKETS;                        // [BLOCK / 64] per-wave totals for the block scan
  const int t = threadIdx.x;
  const uint32_t cnt_all = job.count;
  const int16_t* dig = job.digits;
  const uint32_t* P = job.pts;
  uint32_t* list = job.list;
  uint32_t* heads = job.heads;
  {
    const Acc id = G::identity();
#pragma unroll
    for (int u = 0; u < BPL; ++u) G::store(bucket + (BPL * t + u) * PT, id);
  }
  // 1. histogram of the group's digits.  HIST_LOADS independent digit loads per trip keep the memory pipe busy (a lane's
  // trip is latency-bound)
#pragma unroll
  for (int u = 0; u < BPL; ++u) counts[t + u * BLOCK] = 0;
  __syncthreads();
  for (uint32_t j0 = t; j0 < cnt_all; j0 += G::HIST_LOADS * BLOCK) {
    int d[G::HIST_LOADS];
#pragma unroll
    for (int u = 0; u < G::HIST_LOADS; ++u) {
      const uint32_t j = j0 + u * BLOCK;
      d[u] = j < cnt_all ? dig[j] : 0;
    }
#pragma unroll
    for (int u = 0; u < G::HIST_LOADS; ++u)
      if (d[u] != 0) atomicAdd(&counts[(d[u] < 0 ? -d[u] : d[u]) - 1], 1u);
  }
  __syncthreads();
  // 2. exclusive scan of the counts: lane t scans its BPL buckets, waves scan by shuffles, wave totals through LDS
  uint32_t m;
  {
    const uint32_t c0 = counts[BPL * t], c1 = BPL == 2 ? counts[BPL * t + BPL - 1] : 0u;
    const uint32_t v = c0 + c1;
    uint32_t incl = v;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
      const uint32_t u = __shfl_up(incl, s, 64);
      if ((t & 63) >= s) incl += u;
    }
    if ((t & 63) == 63) wsum[t >> 6] = incl;
    __syncthreads();
    uint32_t wbase = 0, total = 0;
    for (int k = 0; k < BLOCK / 64; ++k) {
      const uint32_t x = wsum[k];
      if (k < (t >> 6)) wbase += x;
      total += x;
    }
    m = total;
    const uint32_t excl = wbase + incl - v;
    cursor[BPL * t] = excl;
    if (BPL == 2) cursor[BPL * t + BPL - 1] = excl + c0;
  }
  __syncthreads();
  // 3. scatter into bucket order, transposed so that entry i of lane l sits at list[i * BLOCK + l]
  const uint32_t chunk = (m + BLOCK - 1) / BLOCK;
  for (uint32_t j0 = t; j0 < cnt_all; j0 += G::SCATTER_LOADS * BLOCK) {
    int dd[G::SCATTER_LOADS];
#pragma unroll
    for (int u = 0; u < G::SCATTER_LOADS; ++u) {
      const uint32_t j = j0 + u * BLOCK;
      dd[u] = j < cnt_all ? dig[j] : 0;
    }
#pragma unroll
    for (int u = 0; u < G::SCATTER_LOADS; ++u) {
      const int d = dd[u];
      const uint32_t j = j0 + u * BLOCK;
      if (d != 0) {
        const uint32_t b = (uint32_t)(d < 0 ? -d : d) - 1;
        const uint32_t pos = atomicAdd(&cursor[b], 1u);
        const uint32_t lane = pos / chunk, i = pos - lane * chunk;
        list[(size_t)i * BLOCK + lane] = j | (b << G::IDX_BITS) | (d < 0 ? 0x80000000u : 0u);
      }
    }
  }
  __threadfence_block();
  __syncthreads();
  // 4. every lane folds its chunk; same trip count for all lanes
  uint32_t head_b = NONE;
  {
    const uint32_t my0 = (uint32_t)t * chunk;
    const uint32_t cnt = my0 >= m ? 0u : (m - my0 < chunk ? m - my0 : chunk);
    Acc acc = G::identity();
    uint32_t cur = NONE;
    bool first_run = true;
    uint32_t* myhead = heads + (size_t)t * PT;
    // Two loads feed an addition -- the list entry, then the point it names -- and the second address depends on the first:
    // entries are fetched TWO trips ahead and points one trip ahead, so that neither latency is exposed (with both one
    // trip ahead the gather waited for its own index: 0.70 of the issue slots).
    uint32_t ent_n = 0, ent_nn = 0;
    Aff pa_n = G::aff_identity();
    if (cnt > 0) ent_n = list[t];
    if (cnt > 1) ent_nn = list[(size_t)BLOCK + t];
    if (cnt > 0) pa_n = G::aff_load(P + (size_t)(ent_n & IDX_MASK) * G::AFF_STRIDE);
#pragma unroll 1
    for (uint32_t i = 0; i < chunk; ++i) {
      if (i < cnt) {
        const uint32_t ent = ent_n;
        const Aff pa = pa_n;
        ent_n = ent_nn;
        if (i + 2 < cnt) ent_nn = list[(size_t)(i + 2) * BLOCK + t];
        if (i + 1 < cnt) pa_n = G::aff_load(P + (size_t)(ent_n & IDX_MASK) * G::AFF_STRIDE);
        const uint32_t b = (ent >> G::IDX_BITS) & (BUCKETS - 1);
        if (b != cur) {
          if (cur != NONE) {
            if (first_run) { G::store(myhead, acc); head_b = cur; first_run = false; }
            else G::store(bucket + cur * PT, acc);
          }
          cur = b;
          acc = G::identity();
        }
        acc = G::madd(acc, pa, (ent >> 31) != 0);
      }
    }
    if (cnt > 0) {
      if (first_run) { G::store(myhead, acc); head_b = cur; }
      else G::store(bucket + cur * PT, acc);
    }
  }
  cursor[t] = head_b;
  __threadfence_block();
  __syncthreads();
  // 5. merge the heads: the first lane of each chain of equal head buckets adds the chain to the bucket
  if (head_b != NONE && (t == 0 || cursor[t - 1] != head_b)) {
    Acc h = G::load(heads + (size_t)t * PT);
    for (int k = t + 1; k < BLOCK && cursor[k] == head_b; ++k) h = G::add(h, G::load(heads + (size_t)k * PT));
    uint32_t* slot = bucket + head_b * PT;
    G::store(slot, G::add(G::load(slot), h));
  }
  __syncthreads();
  // 6. R = sum_j j B_j.  One bucket per lane: lane t holds B_{t+1}; a suffix scan gives S_t = sum_{u >= t} B_{u+1} and
  // R = sum_t S_t.  Two per lane: S_t = B_{2t+1} + B_{2t+2}, L_t = S_t + B_{2t+2}, R = sum_t L_t + 2 sum_{t >= 1} Suf_t with Suf
  // the suffix sums of S.  The staging area re-uses the bucket storage.  The two shapes share the loop but keep their own data
  // flow (one bucket per lane: one live point; two: S, V and the running value): written as one flow, either shape's kernel
  // took about 20 registers more.
  Acc cur;
  [[maybe_unused]] Acc Ssum, V;
  if constexpr (BPL == 2) {
    const Acc b1 = G::load(bucket + (2 * t + 1) * PT);
    Ssum = G::add(G::load(bucket + (2 * t) * PT), b1);
    V = G::add(Ssum, b1);                                   // L_t
  } else {
    cur = G::load(bucket + t * PT);
  }
  uint32_t* stage = lds;                                    // [BLOCK][PT]
  // pass 0: suffix scan of S (Hillis-Steele);  pass 1: tree reduction.  With one bucket per lane the scan's S_t are what the
  // tree sums; with two, the tree sums V_t = L_t + 2 Suf_t.
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
    if constexpr (BPL == 2) cur = pass == 0 ? Ssum : V;
#pragma unroll 1
    for (int k = 0; k < LOG2_BLOCK; ++k) {
      const int s = pass == 0 ? (1 << k) : (BLOCK >> (k + 1));
      __syncthreads();
      G::store(stage + t * PT, cur);
      __syncthreads();
      const bool active = pass == 0 ? (t + s < BLOCK) : (t < s);
      if (active) cur = G::add(cur, G::load(stage + (t + s) * PT));
    }
    if constexpr (BPL == 2) {
      if (pass == 0) {
        if (t >= 1) V = G::add(V, G::dbl(cur));
      } else {
        V = cur;
      }
    }
  }
  if constexpr (BPL == 2) cur = V;
  if (t == 0) G::store(job.out, cur);
}

// ------------------------------------------------------------------------------- workspace
// Bump allocator over a workspace in 256-byte steps; with a null base it only measures (off = the bytes a layout needs).
// A layout is written once as a carve over it: run on a measuring MsmCarve it gives the size the workspace must have, run on
// the workspace it hands out the regions -- the two cannot disagree.
struct MsmCarve {
  uint8_t* base;
  size_t off = 0;
  explicit MsmCarve(void* b) : base(static_cast<uint8_t*>(b)) {}
  template <class T>
  T* take(size_t bytes) {
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += (bytes + 255) & ~size_t(255);
    return p;
  }
};
// the five regions every layout starts with, over `wgs` workgroups whose lists hold list_cap entries each
struct MsmRegions {
  uint32_t* pts;      // [aff_slots][AFF_STRIDE]
  int16_t* digits;    // [digit_rows][n]
  uint32_t* lists;    // [wgs][list_cap]
  uint32_t* heads;    // [wgs][BLOCK][PT_WORDS]
  uint32_t* part;     // [wgs][PT_WORDS]
};
template <class G>
inline MsmRegions msm_carve_regions(MsmCarve& c, size_t aff_slots, size_t digit_rows, size_t n, size_t wgs, size_t list_cap) {
  MsmRegions r;
  r.pts = c.take<uint32_t>(aff_slots * G::AFF_STRIDE * 4);
  r.digits = c.take<int16_t>(digit_rows * n * 2);
  r.lists = c.take<uint32_t>(wgs * list_cap * 4);
  r.heads = c.take<uint32_t>(wgs * G::BLOCK * G::PT_WORDS * 4);
  r.part = c.take<uint32_t>(wgs * G::PT_WORDS * 4);
  return r;
}

}  // namespace vrf
