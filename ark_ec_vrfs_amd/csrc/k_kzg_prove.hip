// k_kzg_prove.hip -- KZG commitments and non-hiding openings over a resident base set (kzg_prove.cuh).
//   k_g1_srs_fill        : one lane per base: a decoded point -> its Montgomery affine slot (the form k_g1_buckets gathers).
//   k_kzg_commit_prep    : one lane per (column, index): range test, digits into set `column` of the layout.
//   k_kzg_quotient<FINAL>: one workgroup of KZGQ_BLOCK lanes per (polynomial, slice of KZGQ_BLOCK * chunk coefficients).  Every
//                          lane runs Horner over its chunk, the lanes' maps are suffix-scanned through LDS.  A polynomial of
//                          more than one workgroup runs the kernel twice: FINAL = false leaves each workgroup's H in
//                          wg_sums; FINAL = true repeats the scan, lane 0 chains the later workgroups' H into the carry of
//                          its own, and the second pass writes v and the digits of the quotient.
//   k_kzg_points_finish  : one lane per column: the sum -> 48-byte compressed (+ the 96-byte form), or zeros under status 2.
// k_g1_buckets<true> / k_g1_final (k_msm_g1.hip) run in between with column = set.
#include "msm_g1.h"

#include "kzg_prove.cuh"
#include "g1_codec.cuh"

namespace vrf {

__global__ void __launch_bounds__(128) k_g1_srs_fill(size_t n, const uint8_t* g1_xy, const uint8_t* status, uint32_t* slots) {
  const size_t i = (size_t)blockIdx.x * 128 + threadIdx.x;
  if (i >= n) return;
  uint32_t w[24];
  const uint32_t* src = reinterpret_cast<const uint32_t*>(g1_xy + i * 96);
  const bool valid = status[i] == 0;
#pragma unroll
  for (int j = 0; j < 24; ++j) w[j] = valid ? src[j] : 0u;
  bls::G1Aff P;
  bool inf;
  (void)bls::g1_load(P, inf, w);
  uint32_t* dst = slots + i * G1_AFF_STRIDE;
  g1_store_affine(dst, P);
#pragma unroll
  for (int j = G1_AFF_WORDS; j < G1_AFF_STRIDE; ++j) dst[j] = 0;
  dst[G1_SRS_INF_WORD] = inf ? 1u : 0u;
}

__global__ void __launch_bounds__(128) k_kzg_commit_prep(G1MsmLayout L, const uint8_t* coeffs) {
  const size_t i = (size_t)blockIdx.x * 128 + threadIdx.x;
  if (i >= (size_t)L.sets * L.n) return;
  const size_t c = i / L.n, j = i - c * L.n;
  uint32_t k[8];
  kzg_load8(k, reinterpret_cast<const uint32_t*>(coeffs + i * 32));
  const bool inf = L.pts[j * G1_AFF_STRIDE + G1_SRS_INF_WORD] != 0;
  if (!kzg_commit_item(L, c, j, k, inf)) L.flags[c] = 2;
}

template <bool FINAL>
__global__ void __launch_bounds__(KZGQ_BLOCK) k_kzg_quotient(G1MsmLayout L, uint32_t chunk, const uint8_t* coeffs,
                                                             const uint8_t* z, uint32_t* wg_sums, uint8_t* value) {
  __shared__ uint32_t sa[KZGQ_BLOCK * NL], sh[KZGQ_BLOCK * NL], sc[NL];
  const int t = threadIdx.x;
  const size_t g = blockIdx.x, G = gridDim.x, c = blockIdx.y, len = L.n + 1;
  uint32_t zw[8];
  kzg_load8(zw, reinterpret_cast<const uint32_t*>(z + c * 32));
  FeN zm;
  bool ok = kzg_point(zm, zw);
  const uint32_t* poly = reinterpret_cast<const uint32_t*>(coeffs + c * len * 32);
  const size_t j0 = (g * KZGQ_BLOCK + t) * chunk;
  KzgMap f;
  f.h = kzg_q_lane_sum(ok, poly, len, j0, chunk, zm);
  f.a = kzg_pow(zm, chunk);
  if (!ok) L.flags[c] = 2;
  // inclusive suffix scan: S_t = f_t o f_{t+1} o ... o f_{B-1}
#pragma unroll 1
  for (int s = 1; s < KZGQ_BLOCK; s <<= 1) {
    __syncthreads();
    fe_store(sa + t * NL, f.a);
    fe_store(sh + t * NL, f.h);
    __syncthreads();
    if (t + s < KZGQ_BLOCK) {
      KzgMap o;
      o.a = fe_load<1, 2>(sa + (t + s) * NL);
      o.h = fe_load<1, 2>(sh + (t + s) * NL);
      f = kzg_compose(f, o);
    }
  }
  if constexpr (!FINAL) {
    if (t == 0) fe_store(wg_sums + (c * G + g) * NL, f.h);
  } else {
    __syncthreads();
    fe_store(sa + t * NL, f.a);
    fe_store(sh + t * NL, f.h);
    if (t == 0) {
      // carry of this workgroup: C_g = H_{g+1} + Z C_{g+1}, Z = z^(B chunk) = the a of every workgroup's map; C_{G-1} = 0
      FeN cw = fe_zero();
#pragma unroll 1
      for (size_t gg = G - 1; gg > g; --gg) {
        KzgMap o;
        o.a = f.a;
        o.h = fe_load<1, 2>(wg_sums + (c * G + gg) * NL);
        cw = kzg_apply(o, cw);
      }
      fe_store(sc, cw);
    }
    __syncthreads();
    FeN carry = fe_load<1, 2>(sc);
    if (t + 1 < KZGQ_BLOCK) {
      KzgMap o;
      o.a = fe_load<1, 2>(sa + (t + 1) * NL);
      o.h = fe_load<1, 2>(sh + (t + 1) * NL);
      carry = kzg_apply(o, carry);
    }
    kzg_q_lane_emit(L, c, L.pts, poly, len, j0, chunk, zm, carry, reinterpret_cast<uint32_t*>(value + c * 32));
  }
}

// sums: nullable = every sum is the point at infinity (no points took part); value: nullable
__global__ void __launch_bounds__(64) k_kzg_points_finish(size_t k, const uint8_t* sums, const uint8_t* flags, uint8_t* out48,
                                                          uint8_t* out_xy, uint8_t* value, uint8_t* status) {
  const size_t c = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (c >= k) return;
  const bool ok = flags[c] == 0;
  uint32_t in[24], enc[12];
#pragma unroll
  for (int j = 0; j < 24; ++j) in[j] = sums ? reinterpret_cast<const uint32_t*>(sums + c * 96)[j] : 0u;
  (void)bls::g1_encode_item(enc, in);              // a sum of the final kernel is on the curve by construction
  uint32_t* o48 = reinterpret_cast<uint32_t*>(out48 + c * 48);
#pragma unroll
  for (int j = 0; j < 12; ++j) o48[j] = ok ? enc[j] : 0u;
  if (out_xy) {
    uint32_t* oxy = reinterpret_cast<uint32_t*>(out_xy + c * 96);
#pragma unroll
    for (int j = 0; j < 24; ++j) oxy[j] = ok ? in[j] : 0u;
  }
  if (value && !ok) {
    uint32_t* ov = reinterpret_cast<uint32_t*>(value + c * 32);
#pragma unroll
    for (int j = 0; j < 8; ++j) ov[j] = 0;
  }
  status[c] = ok ? 0 : 2;
}

// ------------------------------------------------------------------------------- host
void launch_g1_srs_fill(size_t n, const uint8_t* g1_xy, const uint8_t* status, uint32_t* slots, hipStream_t st) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_g1_srs_fill, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, st, n, g1_xy, status, slots);
}

static void launch_tail(const G1MsmLayout& L, uint8_t* out48, uint8_t* out_xy, uint8_t* value, uint8_t* status, hipStream_t st,
                        hipEvent_t* ev) {
  if (ev) (void)hipEventRecord(ev[1], st);
  if (L.n) launch_g1_buckets(L, st, true);
  if (ev) (void)hipEventRecord(ev[2], st);
  if (L.n) launch_g1_final(L, st);
  if (ev) (void)hipEventRecord(ev[3], st);
  hipLaunchKernelGGL(k_kzg_points_finish, dim3((unsigned)((L.sets + 63) / 64)), dim3(64), 0, st, (size_t)L.sets,
                     L.n ? L.sums : nullptr, L.flags, out48, out_xy, value, status);
  if (ev) (void)hipEventRecord(ev[4], st);
}

void launch_kzg_commit(const G1MsmLayout& L, const uint8_t* coeffs, uint8_t* out48, uint8_t* out_xy, uint8_t* status,
                       hipStream_t st, hipEvent_t* ev) {
  if (ev) (void)hipEventRecord(ev[0], st);
  (void)hipMemsetAsync(L.flags, 0, (size_t)L.sets, st);
  const size_t lanes = (size_t)L.sets * L.n;
  if (lanes) hipLaunchKernelGGL(k_kzg_commit_prep, dim3((unsigned)((lanes + 127) / 128)), dim3(128), 0, st, L, coeffs);
  launch_tail(L, out48, out_xy, nullptr, status, st, ev);
}

void launch_kzg_open(const G1MsmLayout& L, uint32_t* wg_sums, const uint8_t* coeffs, const uint8_t* z, uint8_t* value,
                     uint8_t* proof48, uint8_t* proof_xy, uint8_t* status, hipStream_t st, hipEvent_t* ev) {
  if (ev) (void)hipEventRecord(ev[0], st);
  (void)hipMemsetAsync(L.flags, 0, (size_t)L.sets, st);
  const KzgCut cut = kzg_cut(L.n + 1);
  const dim3 grid(cut.wgs, (unsigned)L.sets);
  if (cut.wgs > 1)
    hipLaunchKernelGGL(k_kzg_quotient<false>, grid, dim3(KZGQ_BLOCK), 0, st, L, cut.chunk, coeffs, z, wg_sums, value);
  hipLaunchKernelGGL(k_kzg_quotient<true>, grid, dim3(KZGQ_BLOCK), 0, st, L, cut.chunk, coeffs, z, wg_sums, value);
  launch_tail(L, proof48, proof_xy, value, status, st, ev);
}

}  // namespace vrf
