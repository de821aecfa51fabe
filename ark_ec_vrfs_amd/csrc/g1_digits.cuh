// g1_digits.cuh -- what a prep kernel of the BLS12-381 G1 multi-scalar multiplication writes into a G1MsmLayout: the signed
// window digits of a scalar and the Montgomery affine coordinates of a point (k_msm_g1.hip, k_kzg.hip).
#pragma once
#include "msm_g1.h"

#include "g1.cuh"
#include "msm_buckets.cuh"

namespace vrf {

// signed radix-2^10 digits of a little-endian integer k < 2^(10 W - 1); zero = every digit 0
VRF_HD void g1_write_digits(int16_t* digits, size_t n, size_t i, int W, const uint32_t k[8], bool zero) {
  msm_recode_windows<G1_C>(digits, n, i, W, k, false, zero);
}

VRF_HD void g1_store_affine(uint32_t* dst, const bls::G1Aff& P) {
#pragma unroll
  for (int j = 0; j < bls::NLB; ++j) { dst[j] = (uint32_t)P.x.v[j]; dst[bls::NLB + j] = (uint32_t)P.y.v[j]; }
}

}  // namespace vrf
