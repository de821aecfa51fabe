// k_g1_lincomb.hip -- per-item linear combinations of BLS12-381 G1 points (g1_lincomb.cuh):
//   out[i] = sum_{j<k} scalars[i][j] bases[i][j] + sum_{j<m} shared_scalars[i][j] shared_bases[j].
// One lane per term: item i owns K = next_pow2(k + m) adjacent lanes (K divides 64: an item never straddles a wave), lane t
// of the group multiplies term t (t < k: the item's own base, t < k + m: a shared base, else nothing), log2 K rounds of
// g1_add over cross-lane reads sum the group, and its lane 0 converts to affine and stores.  No LDS and no workspace: the
// kernel reads its inputs and writes its output, so it chains on a stream like the codec kernels.
//
// No lane leaves before the cross-lane reads: the lanes past the last item of the last block are clamped to that item and
// carry the identity like any padding lane; only the stores are guarded.
#include "msm_g1.h"

#include "g1_lincomb.cuh"

namespace vrf {
using namespace bls;

struct LcArgs {
  size_t n;
  uint32_t k, m, log2K;
  const uint8_t *bases, *scalars, *shared_bases, *shared_scalars;
  uint8_t* out;
  size_t out_stride;
  uint8_t* status;
};

__global__ void __launch_bounds__(G1_LINCOMB_BLOCK) k_g1_lincomb(LcArgs a) {
  const size_t lane = (size_t)blockIdx.x * G1_LINCOMB_BLOCK + threadIdx.x;
  const uint32_t K = 1u << a.log2K;
  const size_t item = lane >> a.log2K;
  const uint32_t t = (uint32_t)lane & (K - 1);
  const bool live = item < a.n && t < a.k + a.m;
  const size_t i = item < a.n ? item : a.n - 1;                // every address below is one of the arrays' own
  const uint32_t tt = t < a.k + a.m ? t : a.k + a.m - 1;
  const uint8_t *pb, *ps;
  if (tt < a.k) {
    pb = a.bases + (i * a.k + tt) * 96;
    ps = a.scalars + (i * a.k + tt) * 32;
  } else {
    pb = a.shared_bases + (size_t)(tt - a.k) * 96;
    ps = a.shared_scalars + (i * a.m + (tt - a.k)) * 32;
  }
  uint32_t words[24], sc[8];
  const uint32_t* w = reinterpret_cast<const uint32_t*>(pb);
#pragma unroll
  for (int j = 0; j < 24; ++j) words[j] = w[j];
  const uint32_t* kw = reinterpret_cast<const uint32_t*>(ps);
#pragma unroll
  for (int j = 0; j < 8; ++j) sc[j] = kw[j];
  G1P acc;
  int bad = lc_term(acc, words, sc, live) ? 0 : 1;
  // butterfly over the K lanes of the item: after round r every lane holds the sum of its 2^(r+1)-lane block
  uint32_t buf[G1P_WORDS];
#pragma unroll 1
  for (uint32_t off = 1; off < K; off <<= 1) {
    g1p_store(buf, acc);
#pragma unroll
    for (int j = 0; j < G1P_WORDS; ++j) buf[j] = (uint32_t)__shfl_xor((int)buf[j], (int)off);
    bad |= __shfl_xor(bad, (int)off);
    acc = g1_add(acc, g1p_load(buf));
  }
  if (t == 0 && item < a.n) {
    uint32_t o[24];
    const uint32_t st = lc_finish(o, acc, bad == 0);
    uint32_t* dst = reinterpret_cast<uint32_t*>(a.out + item * a.out_stride);
#pragma unroll
    for (int j = 0; j < 24; ++j) dst[j] = o[j];
    a.status[item] = (uint8_t)st;
  }
}

// ------------------------------------------------------------------------------- host
void launch_g1_lincomb(size_t n, uint32_t k, const uint8_t* bases, const uint8_t* scalars, uint32_t m,
                       const uint8_t* shared_bases, const uint8_t* shared_scalars, uint8_t* out, size_t out_stride,
                       uint8_t* status, hipStream_t st) {
  if (n == 0) return;
  LcArgs a;
  a.n = n; a.k = k; a.m = m;
  a.log2K = 0;
  while ((1u << a.log2K) < k + m) ++a.log2K;
  a.bases = bases; a.scalars = scalars; a.shared_bases = shared_bases; a.shared_scalars = shared_scalars;
  a.out = out; a.out_stride = out_stride; a.status = status;
  const size_t lanes = n << a.log2K;
  hipLaunchKernelGGL(k_g1_lincomb, dim3((unsigned)((lanes + G1_LINCOMB_BLOCK - 1) / G1_LINCOMB_BLOCK)), dim3(G1_LINCOMB_BLOCK),
                     0, st, a);
}

}  // namespace vrf
