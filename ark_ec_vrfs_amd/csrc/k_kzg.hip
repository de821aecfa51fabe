// k_kzg.hip -- KZG opening checks from wire bytes (kzg.cuh): e(C - v g + z pi, h) e(-pi, beta_h) = 1.
//   k_kzg_item_rows : per-item form.  One lane per item writes the rows of k_g1_lincomb (k = 2, m = 1) and B_i = -pi_i; the
//                     linear combinations and the pairings are the existing launches (api.hip chains them).
//   k_kzg_prep_rlc  : batched form.  One lane per item, 128 per block: both points, the range checks, the weight, the two
//                     products r_i z_i and r_i v_i, the points and digits of the short and the full layout; the r_i v_i of a
//                     block are summed (wave shuffles, then the two waves through LDS) into one partial per block.
//   k_kzg_fold      : ONE workgroup sums the partials (a strided pass per lane, then a tree through LDS), negates and writes
//                     g as point n of the full layout.  At the limit of 2^28 items that is 2^21 partials, 8192 per lane of a
//                     sum-and-product-by-R each: milliseconds next to a multi-scalar multiplication of 2^28 points, so there
//                     is no second level.
//   k_kzg_combine   : one lane: S_A = short.sums[0] + full.sums[0], S_B = -short.sums[1] -> the one pairing item.
// k_g1_buckets / k_g1_final (k_msm_g1.hip) run unchanged on both layouts in between.
#include "msm_g1.h"

#include "kzg.cuh"

namespace vrf {

__global__ void __launch_bounds__(KZG_BLOCK) k_kzg_item_rows(size_t n, const uint8_t* g1c, const uint8_t* g1p,
                                                             const uint8_t* dec_status, const uint8_t* z, const uint8_t* v,
                                                             uint8_t* bases, uint8_t* scalars, uint8_t* shared_scalars,
                                                             uint8_t* items) {
  const size_t i = (size_t)blockIdx.x * KZG_BLOCK + threadIdx.x;
  if (i >= n) return;
  uint32_t cw[24], pw[24], zw[8], vw[8];
  const uint32_t* pc = reinterpret_cast<const uint32_t*>(g1c + i * 96);
  const uint32_t* pp = reinterpret_cast<const uint32_t*>(g1p + i * 96);
  const uint32_t* pz = reinterpret_cast<const uint32_t*>(z + i * 32);
  const uint32_t* pv = reinterpret_cast<const uint32_t*>(v + i * 32);
#pragma unroll
  for (int j = 0; j < 24; ++j) { cw[j] = pc[j]; pw[j] = pp[j]; }
#pragma unroll
  for (int j = 0; j < 8; ++j) { zw[j] = pz[j]; vw[j] = pv[j]; }
  uint32_t b[48], s[16], sh[8], np[24];
  kzg_item_rows(b, s, sh, np, cw, pw, dec_status[i] == 0 && dec_status[n + i] == 0, zw, vw);
  uint32_t* ob = reinterpret_cast<uint32_t*>(bases + i * 192);
  uint32_t* os = reinterpret_cast<uint32_t*>(scalars + i * 64);
  uint32_t* osh = reinterpret_cast<uint32_t*>(shared_scalars + i * 32);
  uint32_t* on = reinterpret_cast<uint32_t*>(items + i * 192 + 96);
#pragma unroll
  for (int j = 0; j < 48; ++j) ob[j] = b[j];
#pragma unroll
  for (int j = 0; j < 16; ++j) os[j] = s[j];
#pragma unroll
  for (int j = 0; j < 8; ++j) osh[j] = sh[j];
#pragma unroll
  for (int j = 0; j < 24; ++j) on[j] = np[j];
}

struct KzgSeed { uint8_t b[32]; };

__global__ void __launch_bounds__(KZG_BLOCK) k_kzg_prep_rlc(G1MsmLayout S, G1MsmLayout F, const uint8_t* g1c, const uint8_t* g1p,
                                                            const uint8_t* z, const uint8_t* v, KzgSeed seed, const uint8_t* root,
                                                            uint32_t* partials, uint8_t* status) {
  __shared__ uint32_t stage[(KZG_BLOCK / 64) * NL];
  const size_t i = (size_t)blockIdx.x * KZG_BLOCK + threadIdx.x;
  FeN acc = fe_zero();                          // a lane past the last item adds nothing; no lane leaves before the shuffles
  if (i < S.n) {
    uint32_t cw[24], pw[24], zw[8], vw[8];
    const uint32_t* pc = reinterpret_cast<const uint32_t*>(g1c + i * 96);
    const uint32_t* pp = reinterpret_cast<const uint32_t*>(g1p + i * 96);
    const uint32_t* pz = reinterpret_cast<const uint32_t*>(z + i * 32);
    const uint32_t* pv = reinterpret_cast<const uint32_t*>(v + i * 32);
#pragma unroll
    for (int j = 0; j < 24; ++j) { cw[j] = pc[j]; pw[j] = pp[j]; }
#pragma unroll
    for (int j = 0; j < 8; ++j) { zw[j] = pz[j]; vw[j] = pv[j]; }
    acc = kzg_prep_item(S, F, i, cw, pw, zw, vw, seed.b, root, status);
  }
#pragma unroll 1
  for (int off = 1; off < 64; off <<= 1) {
    FeN o;
#pragma unroll
    for (int j = 0; j < NL; ++j) o.v[j] = (uint32_t)__shfl_xor((int)acc.v[j], off);
    acc = kzg_acc(acc, o);
  }
  const int t = threadIdx.x;
  if ((t & 63) == 0) fe_store(stage + (t >> 6) * NL, acc);
  __syncthreads();
  if (t == 0) {
#pragma unroll 1
    for (int w = 1; w < KZG_BLOCK / 64; ++w) acc = kzg_acc(acc, fe_load<1, 2>(stage + w * NL));
    fe_store(partials + (size_t)blockIdx.x * NL, acc);
  }
}

constexpr int KZG_FOLD_BLOCK = 256;
__global__ void __launch_bounds__(KZG_FOLD_BLOCK) k_kzg_fold(G1MsmLayout F, const uint32_t* partials, size_t n_part,
                                                             const uint8_t* vk) {
  __shared__ uint32_t stage[KZG_FOLD_BLOCK * NL];
  const int t = threadIdx.x;
  FeN acc = fe_zero();
#pragma unroll 1
  for (size_t j = t; j < n_part; j += KZG_FOLD_BLOCK) acc = kzg_acc(acc, fe_load<1, 2>(partials + j * NL));
#pragma unroll 1
  for (int s = KZG_FOLD_BLOCK / 2; s >= 1; s >>= 1) {
    __syncthreads();
    fe_store(stage + t * NL, acc);
    __syncthreads();
    if (t < s) acc = kzg_acc(acc, fe_load<1, 2>(stage + (t + s) * NL));
  }
  if (t == 0) {
    uint32_t gw[24];
    const uint32_t* pg = reinterpret_cast<const uint32_t*>(vk);
#pragma unroll
    for (int j = 0; j < 24; ++j) gw[j] = pg[j];
    kzg_fold_finish(F, acc, gw, F.flags);
  }
}

__global__ void __launch_bounds__(64) k_kzg_combine(G1MsmLayout S, G1MsmLayout F, uint8_t* item192) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  uint32_t a[24], f[24], b[24], out[48];
  const uint32_t* ps = reinterpret_cast<const uint32_t*>(S.sums);
  const uint32_t* pf = reinterpret_cast<const uint32_t*>(F.sums);
#pragma unroll
  for (int j = 0; j < 24; ++j) { a[j] = ps[j]; b[j] = ps[24 + j]; f[j] = pf[j]; }
  kzg_combine(out, a, f, b, F.flags[0] == 0);
  uint32_t* o = reinterpret_cast<uint32_t*>(item192);
#pragma unroll
  for (int j = 0; j < 48; ++j) o[j] = out[j];
}

// ------------------------------------------------------------------------------- host
void launch_kzg_item_rows(size_t n, const uint8_t* g1c, const uint8_t* g1p, const uint8_t* dec_status, const uint8_t* z,
                          const uint8_t* v, uint8_t* bases, uint8_t* scalars, uint8_t* shared_scalars, uint8_t* items,
                          hipStream_t st) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_kzg_item_rows, dim3((unsigned)((n + KZG_BLOCK - 1) / KZG_BLOCK)), dim3(KZG_BLOCK), 0, st, n, g1c, g1p,
                     dec_status, z, v, bases, scalars, shared_scalars, items);
}

void launch_kzg_rlc(const G1MsmLayout& S, const G1MsmLayout& F, const uint8_t* g1c, const uint8_t* g1p, const uint8_t* z,
                    const uint8_t* v, const uint8_t* vk, const uint8_t seed[32], const uint8_t* d_root, uint32_t* partials,
                    uint8_t* status, uint8_t* item192, hipStream_t st, hipEvent_t* ev) {
  if (S.n == 0) return;
  (void)hipMemsetAsync(F.flags, 0, 256, st);
  KzgSeed sd;
  for (int i = 0; i < 32; ++i) sd.b[i] = seed[i];
  const size_t n_part = kzg_partials(S.n);
  hipLaunchKernelGGL(k_kzg_prep_rlc, dim3((unsigned)n_part), dim3(KZG_BLOCK), 0, st, S, F, g1c, g1p, z, v, sd, d_root, partials,
                     status);
  hipLaunchKernelGGL(k_kzg_fold, dim3(1), dim3(KZG_FOLD_BLOCK), 0, st, F, partials, n_part, vk);
  if (ev) (void)hipEventRecord(ev[0], st);
  launch_g1_buckets(S, st);
  launch_g1_buckets(F, st);
  if (ev) (void)hipEventRecord(ev[1], st);
  launch_g1_final(S, st);
  launch_g1_final(F, st);
  hipLaunchKernelGGL(k_kzg_combine, dim3(1), dim3(64), 0, st, S, F, item192);
  if (ev) (void)hipEventRecord(ev[2], st);
}

}  // namespace vrf
