// k_g1_codec.hip -- batch kernels of the BLS12-381 G1 codec (g1_codec.cuh): compressed wire points -> validated affine
// points, validation of affine points, affine -> compressed.  One lane per point, no workspace: every kernel reads its
// input array and writes its output array, so the result can feed vrfhip_pairing_check_batch* / vrfhip_g1_msm on the
// same stream.
#include "msm_g1.h"

#include "g1_codec.cuh"

namespace vrf {
using namespace bls;

template <bool SUBGROUP>
__global__ void __launch_bounds__(128) k_g1_decode(size_t n, const uint8_t* points48, uint8_t* g1_xy, uint8_t* status) {
  const size_t i = (size_t)blockIdx.x * 128 + threadIdx.x;
  if (i >= n) return;
  const uint32_t* src = reinterpret_cast<const uint32_t*>(points48 + i * 48);
  uint32_t in[12], out[24];
#pragma unroll
  for (int j = 0; j < 12; ++j) in[j] = src[j];
  const uint32_t st = g1_decode_item<SUBGROUP>(out, in);
  uint32_t* dst = reinterpret_cast<uint32_t*>(g1_xy + i * 96);
#pragma unroll
  for (int j = 0; j < 24; ++j) dst[j] = out[j];
  status[i] = (uint8_t)st;
}

__global__ void __launch_bounds__(128) k_g1_validate(size_t n, const uint8_t* g1_xy, uint8_t* status) {
  const size_t i = (size_t)blockIdx.x * 128 + threadIdx.x;
  if (i >= n) return;
  const uint32_t* src = reinterpret_cast<const uint32_t*>(g1_xy + i * 96);
  uint32_t in[24];
#pragma unroll
  for (int j = 0; j < 24; ++j) in[j] = src[j];
  status[i] = (uint8_t)g1_validate_item(in);
}

__global__ void __launch_bounds__(128) k_g1_encode(size_t n, const uint8_t* g1_xy, uint8_t* points48, uint8_t* status) {
  const size_t i = (size_t)blockIdx.x * 128 + threadIdx.x;
  if (i >= n) return;
  const uint32_t* src = reinterpret_cast<const uint32_t*>(g1_xy + i * 96);
  uint32_t in[24], out[12];
#pragma unroll
  for (int j = 0; j < 24; ++j) in[j] = src[j];
  const uint32_t st = g1_encode_item(out, in);
  uint32_t* dst = reinterpret_cast<uint32_t*>(points48 + i * 48);
#pragma unroll
  for (int j = 0; j < 12; ++j) dst[j] = out[j];
  status[i] = (uint8_t)st;
}

// ------------------------------------------------------------------------------- host
static dim3 grid128(size_t n) { return dim3((unsigned)((n + 127) / 128)); }

void launch_g1_decode(size_t n, const uint8_t* points48, bool check_subgroup, uint8_t* g1_xy, uint8_t* status, hipStream_t st) {
  if (n == 0) return;
  if (check_subgroup) hipLaunchKernelGGL(k_g1_decode<true>, grid128(n), dim3(128), 0, st, n, points48, g1_xy, status);
  else hipLaunchKernelGGL(k_g1_decode<false>, grid128(n), dim3(128), 0, st, n, points48, g1_xy, status);
}
void launch_g1_validate(size_t n, const uint8_t* g1_xy, uint8_t* status, hipStream_t st) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_g1_validate, grid128(n), dim3(128), 0, st, n, g1_xy, status);
}
void launch_g1_encode(size_t n, const uint8_t* g1_xy, uint8_t* points48, uint8_t* status, hipStream_t st) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_g1_encode, grid128(n), dim3(128), 0, st, n, g1_xy, points48, status);
}

}  // namespace vrf
