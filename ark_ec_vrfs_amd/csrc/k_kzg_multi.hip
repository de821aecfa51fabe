// k_kzg_multi.hip -- multi-commitment, multi-point KZG opening checks from wire bytes (kzg_multi.cuh):
// e(A_i, h) e(B_i, beta_h) = 1 with A_i = sum s_ij C_ij + sum t_ij S_j + sum (u_ij z_ij) pi_ij, B_i = -sum u_ij pi_ij.
//   k_kzgm_item_rows  : per-item form.  One lane per item writes the rows of the two k_g1_lincomb launches (A_i: k + p own
//                       and m + 1 shared terms; B_i: p own terms under r - u_ij); the linear combinations and the pairings are
//                       the existing launches (api.hip chains them).  The rows are a copy with one Fr product per proof, next
//                       to 255-step ladders per term behind it.
//   k_kzgm_prep_items : batched form, one lane per item, 128 per block: validity, the weight (parked for the next kernel,
//                       with the status), the m + 1 products r_i t_ij.  Column by column the products of a block are summed
//                       by wave shuffles; the waves' sums meet in LDS, and after ONE barrier lane j adds up column j and
//                       writes the block's partial: partials[j][block].
//   k_kzgm_prep_terms : one lane per own term (item, j): the point, one or three Fr products, the digit rows of layout A and,
//                       for a proof, of layout B.  One lane per item would hold up to 15 point loads and digit rows in a
//                       loop; per term the kernel has the shape and the occupancy of k_kzg_prep_rlc.
//   k_kzgm_fold       : one workgroup per column sums the column's partials as k_kzg_fold does and writes shared base j (g
//                       for j = 0) as one of the last m + 1 points of layout A.
//   k_kzgm_combine    : one lane: S_A || S_B = A.sums[0] || -B.sums[0] -> the one pairing item.
// k_g1_buckets / k_g1_final (k_msm_g1.hip) run unchanged on both layouts in between.
#include "msm_g1.h"

#include "kzg_multi.cuh"

namespace vrf {

struct KzgmIn {                                  // the arrays of a call, as the header orders them
  const uint8_t *g1c, *s, *t, *g1p, *z, *u;      // g1c, g1p: the decoded points, n k and n p x 96 B
  const uint8_t *dec_c, *dec_p;                  // their decode statuses
};

__global__ void __launch_bounds__(KZG_BLOCK) k_kzgm_item_rows(size_t n, KzgmShape sh, KzgmIn in, uint8_t* bases_a,
                                                              uint8_t* scalars_a, uint8_t* shared_a, uint8_t* bases_b,
                                                              uint8_t* scalars_b) {
  const size_t i = (size_t)blockIdx.x * KZG_BLOCK + threadIdx.x;
  if (i >= n) return;
  const bool ok = kzgm_item_valid(sh, i, in.dec_c, in.dec_p, in.s, in.t, in.z, in.u);
  kzgm_item_rows(sh, i, ok, in.g1c, in.g1p, in.s, in.t, in.z, in.u, bases_a, scalars_a, shared_a, bases_b, scalars_b);
}

struct KzgmSeed { uint8_t b[32]; };
constexpr int KZGM_WAVES = KZG_BLOCK / 64;

__global__ void __launch_bounds__(KZG_BLOCK) k_kzgm_prep_items(size_t n, KzgmShape sh, KzgmIn in, KzgmSeed seed,
                                                               const uint8_t* root, uint32_t* weights, uint32_t* partials,
                                                               size_t n_part, uint8_t* status) {
  __shared__ uint32_t stage[KZGM_MAX_TERMS * KZGM_WAVES * NL];
  const int t = threadIdx.x;
  const size_t i = (size_t)blockIdx.x * KZG_BLOCK + t;
  const bool live = i < n;                      // a lane past the last item adds nothing; no lane leaves before the shuffles
  bool ok = false;
  uint32_t r[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (live) {
    ok = kzgm_item_valid(sh, i, in.dec_c, in.dec_p, in.s, in.t, in.z, in.u);
    kzgm_weight(r, sh, seed.b, root, (uint64_t)i);
#pragma unroll
    for (int j = 0; j < KZGM_WEIGHT_WORDS; ++j) weights[i * KZGM_WEIGHT_WORDS + j] = r[j];
    status[i] = ok ? 0 : 2;
  }
#pragma unroll 1
  for (uint32_t c = 0; c <= sh.m; ++c) {
    uint32_t tw[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (live) kzgm_load_words(tw, in.t + (i * (sh.m + 1) + c) * 32);
    FeN acc = kzgm_col_term(r, tw, ok);
#pragma unroll 1
    for (int off = 1; off < 64; off <<= 1) {
      FeN o;
#pragma unroll
      for (int j = 0; j < NL; ++j) o.v[j] = (uint32_t)__shfl_xor((int)acc.v[j], off);
      acc = kzg_acc(acc, o);
    }
    if ((t & 63) == 0) fe_store(stage + (c * KZGM_WAVES + (t >> 6)) * NL, acc);
  }
  __syncthreads();
  if ((uint32_t)t <= sh.m) {
    FeN acc = fe_load<1, 2>(stage + (size_t)t * KZGM_WAVES * NL);
#pragma unroll 1
    for (int w = 1; w < KZGM_WAVES; ++w) acc = kzg_acc(acc, fe_load<1, 2>(stage + ((size_t)t * KZGM_WAVES + w) * NL));
    fe_store(partials + ((size_t)t * n_part + blockIdx.x) * NL, acc);
  }
}

__global__ void __launch_bounds__(KZG_BLOCK) k_kzgm_prep_terms(G1MsmLayout A, G1MsmLayout B, size_t n, KzgmShape sh, KzgmIn in,
                                                               const uint32_t* weights, const uint8_t* status) {
  const size_t lane = (size_t)blockIdx.x * KZG_BLOCK + threadIdx.x;
  const uint32_t T = sh.k + sh.p;
  if (lane >= n * T) return;
  const size_t i = lane / T;
  const uint32_t j = (uint32_t)(lane - i * T);
  uint32_t pw[24], a[8], z[8] = {0, 0, 0, 0, 0, 0, 0, 0}, r4[KZGM_WEIGHT_WORDS];
  if (j < sh.k) {
    kzgm_load_words(pw, in.g1c + (i * sh.k + j) * 96);
    kzgm_load_words(a, in.s + (i * sh.k + j) * 32);
  } else {
    const size_t q = i * sh.p + (j - sh.k);
    kzgm_load_words(pw, in.g1p + q * 96);
    kzgm_load_words(a, in.u + q * 32);
    kzgm_load_words(z, in.z + q * 32);
  }
#pragma unroll
  for (int w = 0; w < KZGM_WEIGHT_WORDS; ++w) r4[w] = weights[i * KZGM_WEIGHT_WORDS + w];
  kzgm_prep_term(A, B, sh, i, j, pw, a, z, r4, status[i] == 0);
}

constexpr int KZGM_FOLD_BLOCK = 256;
// bases: g (96 B) followed by S_1 .. S_m
__global__ void __launch_bounds__(KZGM_FOLD_BLOCK) k_kzgm_fold(G1MsmLayout A, KzgmShape sh, const uint32_t* partials,
                                                               size_t n_part, const uint8_t* g, const uint8_t* shared_bases) {
  __shared__ uint32_t stage[KZGM_FOLD_BLOCK * NL];
  const int t = threadIdx.x;
  const uint32_t c = blockIdx.x;
  const uint32_t* col = partials + (size_t)c * n_part * NL;
  FeN acc = fe_zero();
#pragma unroll 1
  for (size_t j = t; j < n_part; j += KZGM_FOLD_BLOCK) acc = kzg_acc(acc, fe_load<1, 2>(col + j * NL));
#pragma unroll 1
  for (int s = KZGM_FOLD_BLOCK / 2; s >= 1; s >>= 1) {
    __syncthreads();
    fe_store(stage + t * NL, acc);
    __syncthreads();
    if (t < s) acc = kzg_acc(acc, fe_load<1, 2>(stage + (t + s) * NL));
  }
  if (t == 0) {
    uint32_t bw[24];
    kzgm_load_words(bw, c == 0 ? g : shared_bases + (size_t)(c - 1) * 96);
    kzgm_fold_finish(A, sh, c, acc, bw, A.flags);
  }
}

__global__ void __launch_bounds__(64) k_kzgm_combine(G1MsmLayout A, G1MsmLayout B, uint8_t* item192) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  uint32_t a[24], b[24], out[48];
  kzgm_load_words(a, A.sums);
  kzgm_load_words(b, B.sums);
  kzgm_combine(out, a, b, A.flags[0] == 0);
  kzgm_store_words(item192, out, true);
}

// ------------------------------------------------------------------------------- host
static KzgmIn kzgm_in(const KzgMultiArrays& a) {
  KzgmIn in;
  in.g1c = a.g1c; in.s = a.scalars; in.t = a.shared_scalars; in.g1p = a.g1p; in.z = a.points; in.u = a.coefs;
  in.dec_c = a.dec_c; in.dec_p = a.dec_p;
  return in;
}

void launch_kzg_multi_item_rows(size_t n, uint32_t k, uint32_t m, uint32_t p, const KzgMultiArrays& a, uint8_t* bases_a,
                                uint8_t* scalars_a, uint8_t* shared_a, uint8_t* bases_b, uint8_t* scalars_b, hipStream_t st) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_kzgm_item_rows, dim3((unsigned)((n + KZG_BLOCK - 1) / KZG_BLOCK)), dim3(KZG_BLOCK), 0, st, n,
                     KzgmShape{k, m, p}, kzgm_in(a), bases_a, scalars_a, shared_a, bases_b, scalars_b);
}

void launch_kzg_multi_rlc(const G1MsmLayout& A, const G1MsmLayout& B, size_t n, uint32_t k, uint32_t m, uint32_t p,
                          const KzgMultiArrays& a, const uint8_t* g, const uint8_t* shared_bases, const uint8_t seed[32],
                          const uint8_t* d_root, uint32_t* weights, uint32_t* partials, uint8_t* status, uint8_t* item192,
                          hipStream_t st, hipEvent_t* ev) {
  if (n == 0) return;
  (void)hipMemsetAsync(A.flags, 0, 256, st);
  KzgmSeed sd;
  for (int i = 0; i < 32; ++i) sd.b[i] = seed[i];
  const KzgmShape sh{k, m, p};
  const KzgmIn in = kzgm_in(a);
  const size_t n_part = kzg_partials(n), terms = n * (k + p);
  hipLaunchKernelGGL(k_kzgm_prep_items, dim3((unsigned)n_part), dim3(KZG_BLOCK), 0, st, n, sh, in, sd, d_root, weights, partials,
                     n_part, status);
  hipLaunchKernelGGL(k_kzgm_prep_terms, dim3((unsigned)((terms + KZG_BLOCK - 1) / KZG_BLOCK)), dim3(KZG_BLOCK), 0, st, A, B, n,
                     sh, in, weights, status);
  hipLaunchKernelGGL(k_kzgm_fold, dim3(m + 1), dim3(KZGM_FOLD_BLOCK), 0, st, A, sh, partials, n_part, g, shared_bases);
  if (ev) (void)hipEventRecord(ev[0], st);
  launch_g1_buckets(A, st);
  launch_g1_buckets(B, st);
  if (ev) (void)hipEventRecord(ev[1], st);
  launch_g1_final(A, st);
  launch_g1_final(B, st);
  hipLaunchKernelGGL(k_kzgm_combine, dim3(1), dim3(64), 0, st, A, B, item192);
  if (ev) (void)hipEventRecord(ev[2], st);
}

}  // namespace vrf
