// g1_digits.cuh -- what a prep kernel of the BLS12-381 G1 multi-scalar multiplication writes into a G1MsmLayout: the signed
// window digits of a scalar and the Montgomery affine coordinates of a point (k_msm_g1.hip, k_kzg.hip).
#pragma once
#include "msm_g1.h"

#include "g1.cuh"

namespace vrf {

// signed radix-2^10 digits of a little-endian integer k < 2^(10 W - 1); zero = every digit 0
VRF_HD void g1_write_digits(int16_t* digits, size_t n, size_t i, int W, const uint32_t k[8], bool zero) {
  uint32_t carry = 0;
#pragma unroll 1
  for (int w = 0; w < W; ++w) {
    const int bit = w * G1_C, wi = bit >> 5, sh = bit & 31;
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (j == wi) lo = k[j];
      if (j == wi + 1) hi = k[j];
    }
    uint32_t v = (sh ? ((lo >> sh) | (hi << (32 - sh))) : lo) & ((1u << G1_C) - 1);
    v += carry;
    int d = (int)v;
    carry = 0;
    if (v > (uint32_t)G1_BUCKETS) { d = (int)v - (1 << G1_C); carry = 1; }
    digits[(size_t)w * n + i] = (int16_t)(zero ? 0 : d);
  }
}

VRF_HD void g1_store_affine(uint32_t* dst, const bls::G1Aff& P) {
#pragma unroll
  for (int j = 0; j < bls::NLB; ++j) { dst[j] = (uint32_t)P.x.v[j]; dst[bls::NLB + j] = (uint32_t)P.y.v[j]; }
}

}  // namespace vrf
