// k_fr_ntt.hip -- radix-2 transforms over Fr of BLS12-381 on a resident domain (fr_ntt.cuh).
//   k_fr_domain_consts : one lane: n^-1, the offset and its inverse as Montgomery images.
//   k_fr_domain_fill   : one lane per index: w^i, and for a coset offset^i and n^-1 offset^-i.
//   k_fr_ntt_pass      : one workgroup of NTT_BLOCK lanes per (column, tile) of one pass of the plan: load the tile into LDS
//                        (range test and coset scaling in the first pass), b stages of butterflies with a barrier each, store
//                        (inter-pass twiddles; in the last pass the transposed, scaled, canonical result).  A column of up to
//                        2^NTT_T scalars is one launch; 2^20 is three.
//   k_fr_ntt_merge     : one lane per column after a commitment / opening from evaluations (ntt_merge_status).
#include "msm_g1.h"

#include "fr_ntt.cuh"

namespace vrf {

__global__ void k_fr_domain_consts(uint32_t* consts, uint32_t log_n, const uint8_t* offset32) {
  if (threadIdx.x == 0 && blockIdx.x == 0)
    (void)ntt_domain_consts(consts, log_n, reinterpret_cast<const uint32_t*>(offset32));
}

__global__ void __launch_bounds__(128) k_fr_domain_fill(uint32_t* w, uint32_t* off, uint32_t* offi, const uint32_t* consts,
                                                        uint32_t log_n) {
  const size_t i = (size_t)blockIdx.x * 128 + threadIdx.x;
  if (i >= ((size_t)1 << log_n)) return;
  ntt_domain_entry(w, off, offi, consts, log_n, (uint32_t)i);
}

__global__ void __launch_bounds__(NTT_BLOCK) k_fr_ntt_pass(NttDomain D, NttPass P, uint32_t tiles, const uint8_t* src,
                                                           uint8_t* dst, uint8_t* status) {
  extern __shared__ uint32_t tile[];               // NTT_TILE_WORDS, then the flag
  uint32_t* bad = tile + NTT_TILE_WORDS;
  const uint32_t tid = threadIdx.x, c = blockIdx.x / tiles, tix = blockIdx.x - c * tiles;
  const size_t col = ((size_t)c << P.log_n) * 8;
  const uint32_t* s = reinterpret_cast<const uint32_t*>(src) + col;
  uint32_t* d = reinterpret_cast<uint32_t*>(dst) + col;
  const uint32_t elems = ntt_tile_elems(P);
  if (tid == 0) bad[0] = 0;
  __syncthreads();
  bool ok = true;
  for (uint32_t t = tid; t < elems; t += NTT_BLOCK) ok = ntt_load_lane(tile, D, P, tix, t, s) && ok;
  if (!ok) bad[0] = 1;
  __syncthreads();
  const bool refused = P.first ? bad[0] != 0 : status[c] != 0;
  if (P.first && refused && tid == 0) status[c] = 2;
#pragma unroll 1
  for (uint32_t st = 0; st < P.b; ++st) {
    for (uint32_t t = tid; t < elems / 2; t += NTT_BLOCK) ntt_bfly_lane(tile, D, P, st, t);
    __syncthreads();
  }
  for (uint32_t t = tid; t < elems; t += NTT_BLOCK) ntt_store_lane(tile, D, P, tix, t, d, P.last && refused);
}

__global__ void __launch_bounds__(64) k_fr_ntt_merge(size_t k, const uint8_t* ntt_status, uint8_t* out48, uint8_t* out_xy,
                                                     uint8_t* value, uint8_t* status) {
  const size_t c = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (c < k) ntt_merge_status(c, ntt_status, out48, out_xy, value, status);
}

// ------------------------------------------------------------------------------- host
int fr_ntt_passes(uint32_t log_n) { return ntt_plan((int)log_n).passes; }
int fr_ntt_max_log() { return NTT_MAX_LOG; }
size_t fr_ntt_table_words(uint32_t log_n) { return ((size_t)NL) << log_n; }
size_t fr_ntt_const_words() { return 3 * NL; }

void launch_fr_domain_fill(const FrNttTables& T, const uint8_t* d_offset32, hipStream_t st) {
  hipLaunchKernelGGL(k_fr_domain_consts, dim3(1), dim3(64), 0, st, T.consts, T.log_n, d_offset32);
  const size_t n = (size_t)1 << T.log_n;
  hipLaunchKernelGGL(k_fr_domain_fill, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, st, T.w, T.off, T.offi, T.consts,
                     T.log_n);
}

void launch_fr_ntt(const FrNttTables& T, size_t k, bool inverse, const uint8_t* in, uint8_t* out, uint8_t* scratch,
                   uint8_t* status, hipStream_t st) {
  constexpr size_t lds = (NTT_TILE_WORDS + 1) * sizeof(uint32_t);
  static const bool once = [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_fr_ntt_pass), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds);
    return true;
  }();
  (void)once;
  NttDomain D{};
  D.log_n = T.log_n; D.w = T.w; D.off = T.off; D.offi = T.offi; D.ninv = T.consts;
  const NttPlan pl = ntt_plan((int)T.log_n);
  (void)hipMemsetAsync(status, 0, k, st);
  for (int p = 0; p < pl.passes; ++p) {
    const NttPass P = ntt_pass(pl, p, inverse);
    const uint32_t tiles = ntt_tiles(P);
    hipLaunchKernelGGL(k_fr_ntt_pass, dim3((unsigned)(k * tiles)), dim3(NTT_BLOCK), lds, st, D, P, tiles,
                       P.first ? in : scratch, P.last ? out : scratch, status);
  }
}

void launch_fr_ntt_merge(size_t k, const uint8_t* ntt_status, uint8_t* out48, uint8_t* out_xy, uint8_t* value, uint8_t* status,
                         hipStream_t st) {
  hipLaunchKernelGGL(k_fr_ntt_merge, dim3((unsigned)((k + 63) / 64)), dim3(64), 0, st, k, ntt_status, out48, out_xy, value,
                     status);
}

}  // namespace vrf
