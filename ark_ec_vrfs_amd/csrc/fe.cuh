// fe.cuh -- Fq arithmetic for gfx950: 9 limbs x 29 bits, Montgomery radix R = 2^261.
//
// Replaces ark_ff::Fp<MontBackend, 4> (the type behind `BaseField`, /root/reference
// src/lib.rs:15) on the VRF hot path.  Design notes:
//
//  * gfx950 has a full-rate 32x32+64 multiply-add (v_mad_u64_u32, measured at the same issue
//    rate as v_add: profiles/r01_instr_rate_microbench.jsonl) but that instruction has no
//    carry-IN.  A saturated 2^32 radix therefore pays an add-with-carry per product.  With
//    29-bit limbs nine products plus nine reduction products fit a 64-bit accumulator with
//    no carry handling at all: a field multiplication is 81 + 72 v_mad_u64_u32 plus one
//    shift/mask per column.
//  * Limbs are *lazy*: additions and subtractions are nine independent 32-bit adds with no
//    carry propagation and no modular reduction.  Every value carries two compile-time
//    bounds: L (each limb < L * (2^29 + 2^13)) and V (value < V * q).  fe_mul static_asserts
//    that its 64-bit column accumulators cannot overflow (L1 * L2 <= 6) and derives the
//    output bound, so an overflow is a compile error, not a wrong proof.
//  * q = 1 (mod 2^32) => -q^-1 = -1 (mod 2^29) and q's low limb is 1: the Montgomery
//    quotient digit is (-acc) & mask, no multiply.
//
// Everything is __host__ __device__ so the same source can be unit-tested on the CPU by
// tests/hostsim (test tooling only; never linked into libvrfhip.so).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "field.h"
#include "vrf_types.h"

VRF_NS_BEGIN

using vrfk::LMASK;
constexpr int NL = 9;
constexpr int LW = 29;

// out value bound of a Montgomery product: (a*b + m*q)/R < q * (1 + Va*Vb*q/R), q/R = MULV_NUM / 1e5 (0.014152 for
// BLS12-381 Fr); the pseudo-Mersenne product of 2^255 - 19 always comes out below 2^255 + 2^30 < 2q
constexpr int mul_v(int v1, int v2) {
  return vrfk::FIELD_KIND == 2 ? 2 : 1 + (v1 * v2 * vrfk::MULV_NUM + 99999) / 100000;
}

template <int L, int V>
struct Fe {
  static_assert(L >= 1 && L <= 7, "limb bound out of range");
  static_assert(V >= 1 && V <= vrfk::VMAX, "value bound out of range (top limb must stay < 2^29)");
  uint32_t v[NL];
  Fe() = default;
  template <int L2, int V2>
  VRF_HD Fe(const Fe<L2, V2>& o) {
    static_assert(L2 <= L && V2 <= V, "narrowing Fe conversion");
#pragma unroll
    for (int i = 0; i < NL; ++i) v[i] = o.v[i];
  }
};

using FeN = Fe<1, 2>;   // storage type: a Montgomery product (limbs < 2^29, value < 2q)
using FeP = Fe<1, 5>;   // point-coordinate type (closure bound of the TE formulas, te.cuh)

template <int L, int V>
VRF_HD Fe<L, V> fe_load(const uint32_t* p) {
  Fe<L, V> r;
#pragma unroll
  for (int i = 0; i < NL; ++i) r.v[i] = p[i];
  return r;
}
VRF_HD FeN fe_const(const uint32_t (&c)[NL]) {
  FeN r;
#pragma unroll
  for (int i = 0; i < NL; ++i) r.v[i] = c[i];
  return r;
}
template <int L, int V>
VRF_HD void fe_store(uint32_t* p, const Fe<L, V>& a) {
#pragma unroll
  for (int i = 0; i < NL; ++i) p[i] = a.v[i];
}

VRF_HD FeN fe_zero() {
  FeN r;
#pragma unroll
  for (int i = 0; i < NL; ++i) r.v[i] = 0;
  return r;
}
VRF_HD FeN fe_one() { return fe_const(vrfk::ONE_M); }

// ------------------------------------------------------------------ lazy add / sub
template <int L1, int V1, int L2, int V2>
VRF_HD Fe<L1 + L2, V1 + V2> fe_add(const Fe<L1, V1>& a, const Fe<L2, V2>& b) {
  Fe<L1 + L2, V1 + V2> r;
#pragma unroll
  for (int i = 0; i < NL; ++i) r.v[i] = a.v[i] + b.v[i];
  return r;
}

template <int K, int LB>
struct Bias;
#define VRF_BIAS(K_, LB_)                                            \
  template <>                                                        \
  struct Bias<K_, LB_> {                                             \
    static VRF_HD uint32_t at(int i) { return vrfk::BIAS_L##LB_##_K##K_[i]; } \
  };
VRF_BIAS(4, 1) VRF_BIAS(8, 1) VRF_BIAS(16, 1) VRF_BIAS(32, 1) VRF_BIAS(64, 1)
VRF_BIAS(4, 2) VRF_BIAS(8, 2) VRF_BIAS(16, 2) VRF_BIAS(32, 2) VRF_BIAS(64, 2)
#undef VRF_BIAS

constexpr int bias_k(int v) { return v < 4 ? 4 : v < 8 ? 8 : v < 16 ? 16 : v < 32 ? 32 : 64; }

// a - b (mod q) computed as a + K*q - b limb-wise.  The bias word has limbs >= LB*(2^29+2^13)
// and a top limb >= V2*q / 2^232, so no limb ever borrows.
template <int L1, int V1, int L2, int V2>
VRF_HD Fe<L1 + L2 + 1, V1 + bias_k(V2)> fe_sub(const Fe<L1, V1>& a, const Fe<L2, V2>& b) {
  static_assert(L2 <= 2, "subtrahend must have L <= 2 (normalise first)");
  constexpr int K = bias_k(V2);   // K >= V2 + 1
  Fe<L1 + L2 + 1, V1 + K> r;
#pragma unroll
  for (int i = 0; i < NL; ++i) r.v[i] = a.v[i] + (Bias<K, L2>::at(i) - b.v[i]);
  return r;
}

template <int L, int V>
VRF_HD Fe<L + 1, bias_k(V)> fe_neg(const Fe<L, V>& b) {
  static_assert(L <= 2, "fe_neg operand must have L <= 2");
  constexpr int K = bias_k(V);
  Fe<L + 1, K> r;
#pragma unroll
  for (int i = 0; i < NL; ++i) r.v[i] = Bias<K, L>::at(i) - b.v[i];
  return r;
}

// small multiples (shift-adds, one v_lshl_add_u32 per limb)
template <int L, int V>
VRF_HD Fe<2 * L, 2 * V> fe_dbl(const Fe<L, V>& a) {
  Fe<2 * L, 2 * V> r;
#pragma unroll
  for (int i = 0; i < NL; ++i) r.v[i] = a.v[i] << 1;
  return r;
}
template <int L, int V>
VRF_HD Fe<5 * L, 5 * V> fe_mul5(const Fe<L, V>& a) {
  Fe<5 * L, 5 * V> r;
#pragma unroll
  for (int i = 0; i < NL; ++i) r.v[i] = (a.v[i] << 2) + a.v[i];
  return r;
}

// weak normalisation: one parallel carry pass; limbs < 2^29 + 8 afterwards (L = 1).
template <int L, int V>
VRF_HD Fe<1, V> fe_norm(const Fe<L, V>& a) {
  Fe<1, V> r;
  r.v[0] = a.v[0] & LMASK;
#pragma unroll
  for (int i = 1; i < NL - 1; ++i) r.v[i] = (a.v[i] & LMASK) + (a.v[i - 1] >> LW);
  r.v[NL - 1] = a.v[NL - 1] + (a.v[NL - 2] >> LW);
  return r;
}

#if VRF_FIELD == 3
// Weak reduction for P-256, where a 256-bit modulus leaves the lazy sums only V <= 32 of headroom (2^261 / 2^256):
// any value < 32 q comes back below 2^256 + 2^229 < 2 q with exact limbs.  k = floor(v / 2^256) <= 31 and
// v - k q = (v mod 2^256) + k (2^224 - 2^192 - 2^96 + 1): one exact carry pass to read k, one signed pass to add the
// four terms.  ~60 32-bit instructions, a third of a product by one (the only reduction the other fields need).
template <int L, int V>
VRF_HD Fe<1, 2> fe_wred(const Fe<L, V>& a) {
  uint32_t x[NL];
  uint32_t c = 0;
#pragma unroll
  for (int i = 0; i < NL - 1; ++i) {
    const uint32_t t = a.v[i] + c;
    x[i] = t & LMASK;
    c = t >> LW;
  }
  x[NL - 1] = a.v[NL - 1] + c;
  const int32_t k = (int32_t)(x[NL - 1] >> 24);          // bit 256 is bit 24 of limb 8
  x[NL - 1] &= 0x00ffffffu;
  Fe<1, 2> r;
  int32_t cc = k;                                        // + k at bit 0
#pragma unroll
  for (int i = 0; i < NL; ++i) {
    int32_t t = (int32_t)x[i] + cc;
    if (i == 3) t -= k << 9;                             // - k 2^96  (96 = 3 * 29 + 9)
    if (i == 6) t -= k << 18;                            // - k 2^192 (192 = 6 * 29 + 18)
    if (i == 7) t += k << 21;                            // + k 2^224 (224 = 7 * 29 + 21)
    r.v[i] = (i < NL - 1) ? ((uint32_t)t & LMASK) : (uint32_t)t;
    cc = t >> LW;
  }
  return r;
}
#endif

template <int L, int V>
VRF_HD Fe<L, V> fe_select(bool c, const Fe<L, V>& a, const Fe<L, V>& b) {   // c ? a : b
  Fe<L, V> r;
#pragma unroll
  for (int i = 0; i < NL; ++i) r.v[i] = c ? a.v[i] : b.v[i];
  return r;
}

// ------------------------------------------------------------------ multiply
VRF_HD uint64_t mad(uint32_t a, uint32_t b, uint64_t c) { return (uint64_t)a * b + c; }
// The multiply-add of the product columns.  Left alone, LLVM reassociates a column of fe_mul: it sums the a*b terms apart
// from the carried accumulator, so that they need not wait for the Montgomery digits, and pays a 64-bit addition per column
// to join the two (24 v_lshl_add_u64 per product where 9 are the bias).  CHAIN = true passes the result through an empty
// asm on the device, which keeps every column the single multiply-add chain it is written as: 214 -> 198 VALU instructions
// per product, 184 -> 169 per square, and a third fewer live registers -- but one dependent chain of 153 multiply-adds.
// That pays in the verification ladders (straus2 / straus4 / win_mul, vrf_core.cuh), which it takes from three to four
// waves per SIMD; it costs time in the kernels that sit at two waves with scratch whatever the product does (checked
// decode: +2 %, measured), so CHAIN is an argument that only those ladders set.  The host build has
// no such instruction to protect.
template <bool CHAIN>
VRF_HD uint64_t mac(uint32_t a, uint32_t b, uint64_t c) {
  uint64_t r = (uint64_t)a * b + c;
#if defined(__HIP_DEVICE_COMPILE__)
  if constexpr (CHAIN) asm("" : "+v"(r));
#endif
  return r;
}
// Three digit rules, chosen at compile time by the field (field.h, vrfk::FIELD_KIND):
//
//  kind 0 (BLS12-381 Fr, q = 1 mod 2^29): the Montgomery digit of a column t is m = -t mod 2^29 and the column leaves the
//  carry (t + m) >> 29 = (t >> 29) + (t mod 2^29 != 0) = (t + 2^29 - 1) >> 29.  Carrying the bias 2^29 - 1 in the
//  accumulator turns "negate, mask, add m back (64-bit)" into one v_bitop3 (~t & mask) and no addition:
//  17 fewer instructions per product (measured on gfx950: 1.64e11 -> 1.75e11 products/s).  The bias is far
//  below the headroom the L1 * L2 <= 6 assertion leaves (about 2^59).
//
//  kind 1 (BN254 Fr, general q): m = t * (-q^-1) mod 2^29 -- NINV29 = 2^28 - 1 there, a shift and a subtraction -- and
//  the column takes m * q[0] like every other limb of q: 9 more multiply-adds per product than kind 0.
//
//  kind 2 (2^255 - 19): no Montgomery form at all (R = 1).  The 17 columns of the plain product are carried into 29-bit
//  digits, then 2^261 = 1216 (mod q) folds digit k + 9 onto digit k in a second carry pass, and what is left above bit
//  255 comes back as 19 * carry into limb 0: 81 + 9 multiply-adds instead of 153.  Output < 2^255 + 2^30.
VRF_HD constexpr uint64_t mont_bias() { return vrfk::FIELD_KIND == 0 ? (uint64_t)LMASK : 0; }
VRF_HD uint32_t mont_digit(uint32_t col) {
  if constexpr (vrfk::FIELD_KIND == 0) return ~col & LMASK;          // the accumulator carries the bias LMASK
  else return (col * vrfk::NINV29) & LMASK;
}
constexpr uint32_t PM_FOLD = 1216;      // 2^261 mod (2^255 - 19)
constexpr int PM_TOPBITS = 23;          // bit 255 is bit 23 of limb 8

// second pass of the pseudo-Mersenne product: d = the plain product, or sum of two products, in 18 digits (d[17] < 2^29
// because the sum is < 2^522: operands < 64 q in fe_mul, V1 V2 + V3 V4 <= 4096 asserted in fe_mul2); digit k + 9 folds
// onto digit k with the factor 2^261 = 1216, and what then lies above bit 255 (bit 23 of limb 8) comes back as 19 * carry
// into limb 0.  Out: limbs < 2^29 + 2, value < 2^255 + 2^30 < 2q.
template <int V>
VRF_HD void pm_fold(Fe<1, V>& r, const uint32_t (&d)[2 * NL]) {
  uint64_t acc = 0;
#pragma unroll
  for (int k = 0; k < NL - 1; ++k) {
    acc = mad(d[k + NL], PM_FOLD, acc + d[k]);            // < 2^41
    r.v[k] = (uint32_t)acc & LMASK;
    acc >>= LW;
  }
  acc = mad(d[2 * NL - 1], PM_FOLD, acc + d[NL - 1]);
  r.v[NL - 1] = (uint32_t)acc & ((1u << PM_TOPBITS) - 1);
  const uint32_t c = (uint32_t)(acc >> PM_TOPBITS);       // < 2^18
  const uint32_t r0 = r.v[0] + 19u * c;                   // < 2^30
  r.v[0] = r0 & LMASK;
  r.v[1] += r0 >> LW;
}

// The columns of a*b (TWO = false) or of a*b + c*d (TWO = true: both products go into the same columns and the sum is
// reduced ONCE), on raw limbs; V is the caller's value bound of the result.
template <bool CHAIN, bool TWO, int V>
VRF_HD Fe<1, V> fe_mul_cols(const uint32_t (&a)[NL], const uint32_t (&b)[NL], const uint32_t (&c)[NL], const uint32_t (&d)[NL]) {
  Fe<1, V> r;
  if constexpr (vrfk::FIELD_KIND == 2) {
    uint32_t dg[2 * NL];                                  // the plain product in 29-bit digits: < 2^522
    uint64_t acc = 0;
#pragma unroll
    for (int k = 0; k < 2 * NL - 1; ++k) {
#pragma unroll
      for (int i = (k < NL ? 0 : k - NL + 1); i <= (k < NL ? k : NL - 1); ++i) {
        acc = mac<CHAIN>(a[i], b[k - i], acc);
        if constexpr (TWO) acc = mac<CHAIN>(c[i], d[k - i], acc);
      }
      dg[k] = (uint32_t)acc & LMASK;
      acc >>= LW;
    }
    dg[2 * NL - 1] = (uint32_t)acc;
    pm_fold(r, dg);
  } else {
    uint32_t m[NL];
    uint64_t acc = 0;
#pragma unroll
    for (int k = 0; k < NL; ++k) {
      acc += mont_bias();
#pragma unroll
      for (int i = 0; i <= k; ++i) {
        acc = mac<CHAIN>(a[i], b[k - i], acc);
        if constexpr (TWO) acc = mac<CHAIN>(c[i], d[k - i], acc);
      }
#pragma unroll
      for (int i = 0; i < k; ++i) acc = mac<CHAIN>(m[i], vrfk::Q29[k - i], acc);
      m[k] = mont_digit((uint32_t)acc);
      if constexpr (vrfk::FIELD_KIND != 0) acc = mac<CHAIN>(m[k], vrfk::Q29[0], acc);
      acc >>= LW;                        // kind 0: == (column + m[k] * Q29[0]) >> LW, Q29[0] == 1 (see mont_bias)
    }
#pragma unroll
    for (int k = NL; k < 2 * NL - 1; ++k) {
#pragma unroll
      for (int i = k - NL + 1; i < NL; ++i) {
        acc = mac<CHAIN>(a[i], b[k - i], acc);
        if constexpr (TWO) acc = mac<CHAIN>(c[i], d[k - i], acc);
      }
#pragma unroll
      for (int i = k - NL + 1; i < NL; ++i) acc = mac<CHAIN>(m[i], vrfk::Q29[k - i], acc);
      r.v[k - NL] = (uint32_t)acc & LMASK;
      acc >>= LW;
    }
    r.v[NL - 1] = (uint32_t)acc;
  }
  return r;
}

template <bool CHAIN = false, int L1, int V1, int L2, int V2>
VRF_HD Fe<1, mul_v(V1, V2)> fe_mul(const Fe<L1, V1>& a, const Fe<L2, V2>& b) {
  static_assert(L1 * L2 <= 6, "fe_mul: 64-bit column accumulator could overflow");
  return fe_mul_cols<CHAIN, false, mul_v(V1, V2)>(a.v, b.v, a.v, b.v);
}

// a*b + c*d with ONE reduction: 2 * 81 + 72 multiply-adds against two full products (2 * 153) plus a lazy addition.
// The column bound is the one of fe_mul with L1 L2 + L3 L4 in the place of L1 L2: 9 (L1 L2 + L3 L4) 2^58 (1 + 2^-15)
// + 9 * 2^58 + carry < 2^64 for a sum <= 6.  Value: (a b + c d + m q) / R < q (1 + (V1 V2 + V3 V4) q / R).
// 2^255 - 19: the plain sum of the two products must stay below 2^522 for pm_fold's top digit d[17] < 2^29:
// (V1 V2 + V3 V4) q^2 < 2^12 * 2^510; its result is < 2q whatever came in.
constexpr int mul2_v(int v1, int v2, int v3, int v4) {
  return vrfk::FIELD_KIND == 2 ? 2 : 1 + ((v1 * v2 + v3 * v4) * vrfk::MULV_NUM + 99999) / 100000;
}
template <bool CHAIN = false, int L1, int V1, int L2, int V2, int L3, int V3, int L4, int V4>
VRF_HD Fe<1, mul2_v(V1, V2, V3, V4)> fe_mul2(const Fe<L1, V1>& a, const Fe<L2, V2>& b, const Fe<L3, V3>& c, const Fe<L4, V4>& d) {
  static_assert(L1 * L2 + L3 * L4 <= 6, "fe_mul2: 64-bit column accumulator could overflow");
  static_assert(vrfk::FIELD_KIND != 2 || V1 * V2 + V3 * V4 <= 4096, "fe_mul2: the plain sum of products must stay below 2^522");
  return fe_mul_cols<CHAIN, true, mul2_v(V1, V2, V3, V4)>(a.v, b.v, c.v, d.v);
}

template <bool CHAIN = false, int L, int V>
VRF_HD Fe<1, mul_v(V, V)> fe_sqr(const Fe<L, V>& a) {
  static_assert(L * L <= 6, "fe_sqr: 64-bit column accumulator could overflow");
  Fe<1, mul_v(V, V)> r;
  uint32_t a2[NL];
#pragma unroll
  for (int i = 0; i < NL; ++i) a2[i] = a.v[i] << 1;
  if constexpr (vrfk::FIELD_KIND == 2) {
    uint32_t d[2 * NL];
    uint64_t acc = 0;
#pragma unroll
    for (int k = 0; k < 2 * NL - 1; ++k) {
#pragma unroll
      for (int i = (k < NL ? 0 : k - NL + 1); 2 * i < k; ++i) acc = mac<CHAIN>(a2[i], a.v[k - i], acc);
      if ((k & 1) == 0) acc = mac<CHAIN>(a.v[k / 2], a.v[k / 2], acc);
      d[k] = (uint32_t)acc & LMASK;
      acc >>= LW;
    }
    d[2 * NL - 1] = (uint32_t)acc;
    pm_fold(r, d);
    return r;
  } else {
  uint32_t m[NL];
  uint64_t acc = 0;
#pragma unroll
  for (int k = 0; k < NL; ++k) {
    acc += mont_bias();
#pragma unroll
    for (int i = 0; 2 * i < k; ++i) acc = mac<CHAIN>(a2[i], a.v[k - i], acc);
    if ((k & 1) == 0) acc = mac<CHAIN>(a.v[k / 2], a.v[k / 2], acc);
#pragma unroll
    for (int i = 0; i < k; ++i) acc = mac<CHAIN>(m[i], vrfk::Q29[k - i], acc);
    m[k] = mont_digit((uint32_t)acc);
    if constexpr (vrfk::FIELD_KIND != 0) acc = mac<CHAIN>(m[k], vrfk::Q29[0], acc);
    acc >>= LW;
  }
#pragma unroll
  for (int k = NL; k < 2 * NL - 1; ++k) {
#pragma unroll
    for (int i = k - NL + 1; 2 * i < k; ++i) acc = mac<CHAIN>(a2[i], a.v[k - i], acc);
    if ((k & 1) == 0) acc = mac<CHAIN>(a.v[k / 2], a.v[k / 2], acc);
#pragma unroll
    for (int i = k - NL + 1; i < NL; ++i) acc = mac<CHAIN>(m[i], vrfk::Q29[k - i], acc);
    r.v[k - NL] = (uint32_t)acc & LMASK;
    acc >>= LW;
  }
  r.v[NL - 1] = (uint32_t)acc;
  return r;
  }
}

// ------------------------------------------------------------------ canonical forms
// Exact carry propagation + one conditional subtraction of q.  Input value must be < 2q.
template <int L>
VRF_HD void fe_reduce_once(uint32_t out[NL], const Fe<L, 2>& a) {
  uint32_t x[NL], d[NL];
  uint32_t c = 0;
#pragma unroll
  for (int i = 0; i < NL - 1; ++i) {
    uint32_t t = a.v[i] + c;
    x[i] = t & LMASK;
    c = t >> LW;
  }
  x[NL - 1] = a.v[NL - 1] + c;
  uint32_t borrow = 0;
#pragma unroll
  for (int i = 0; i < NL; ++i) {
    uint32_t t = x[i] - vrfk::Q29[i] - borrow;
    borrow = t >> 31;
    d[i] = (i < NL - 1) ? (t & LMASK) : t;
  }
#pragma unroll
  for (int i = 0; i < NL; ++i) out[i] = borrow ? x[i] : d[i];
}

// canonical Montgomery image: the unique representative in [0, q) of the same residue.
template <int L, int V>
VRF_HD FeN fe_canon(const Fe<L, V>& a) {
  static_assert(L <= 6, "");
  FeN t = fe_mul(a, fe_one());     // a * R / R = a, value < q(1 + V*0.0142) < 2q
  FeN r;
  fe_reduce_once(r.v, t);
  return r;
}

template <int L, int V>
VRF_HD bool fe_is_zero(const Fe<L, V>& a) {
  FeN c = fe_canon(a);
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < NL; ++i) o |= c.v[i];
  return o == 0;
}

template <int L1, int V1, int L2, int V2>
VRF_HD bool fe_eq(const Fe<L1, V1>& a, const Fe<L2, V2>& b) {
  FeN x = fe_canon(a), y = fe_canon(b);
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < NL; ++i) o |= x.v[i] ^ y.v[i];
  return o == 0;
}

// 8 x u32 little-endian integer (< 2^256) -> 9 x 29 plain limbs
VRF_HD void u256_to_limbs(uint32_t out[NL], const uint32_t w[8]) {
#pragma unroll
  for (int i = 0; i < NL; ++i) {
    const int bit = i * LW, j = bit >> 5, s = bit & 31;
    uint32_t lo = w[j] >> s;
    if (s > 3 && j + 1 < 8) lo |= w[j + 1] << (32 - s);
    out[i] = (i < NL - 1) ? (lo & LMASK) : lo;
  }
}
// 9 x 29 exact limbs (value < 2^256) -> 8 x u32
VRF_HD void limbs_to_u256(uint32_t w[8], const uint32_t x[NL]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int bit = j * 32, i = bit / LW, s = bit % LW;
    uint32_t v = x[i] >> s;
    if (i + 1 < NL) v |= x[i + 1] << (LW - s);
    if (LW - s + LW < 32 && i + 2 < NL) v |= x[i + 2] << (2 * LW - s);
    w[j] = v;
  }
}

// integer < 2^256 (need not be < q) -> Montgomery
VRF_HD FeN fe_from_u256(const uint32_t w[8]) {
  Fe<1, vrfk::V256> t;                // 2^256 < 2.21 q (BLS12-381 Fr), 5.3 q (BN254 Fr)
  u256_to_limbs(t.v, w);
  return fe_mul(t, fe_const(vrfk::R2_29));
}
// Montgomery -> canonical integer in [0, q) as 8 x u32
template <int L, int V>
VRF_HD void fe_to_u256(uint32_t w[8], const Fe<L, V>& a) {
  static_assert(L <= 6, "");
  FeN one;
#pragma unroll
  for (int i = 0; i < NL; ++i) one.v[i] = (i == 0);
  FeN t = fe_mul(a, one);             // a / R, value < q + tiny
  uint32_t c[NL];
  fe_reduce_once(c, t);
  limbs_to_u256(w, c);
}

// Coordinates at the ABI come as canonical integers or -- VRFHIP_FLAG_COORDS_MONT256 -- as arkworks' in-memory field
// elements: the Montgomery image x 2^256 mod q, four little-endian u64.  Both are integers < q on the wire.
//   in : words -> Fe (x 2^261) and the canonical words of x (the sign of x, the encoding of y need them)
//   out: Fe -> words
VRF_HD FeN fe_from_abi(uint32_t canon[8], const uint32_t w[8], bool mont256) {
  Fe<1, vrfk::V256> t;
  u256_to_limbs(t.v, w);
  FeN k;
#pragma unroll
  for (int i = 0; i < NL; ++i) k.v[i] = mont256 ? vrfk::TWO266_29[i] : vrfk::R2_29[i];
  const FeN r = fe_mul(t, k);          // canonical: x R^2 / R; Montgomery-256: (x 2^256) 2^266 / 2^261
  if (mont256) {
    fe_to_u256(canon, r);
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) canon[i] = w[i];
  }
  return r;
}
template <int L, int V>
VRF_HD void fe_to_mont256(uint32_t w[8], const Fe<L, V>& a) {
  static_assert(L <= 6, "");
  FeN t = fe_mul(a, fe_const(vrfk::TWO256_29));      // (x 2^261) 2^256 / 2^261 = x 2^256, value < q + tiny
  uint32_t c[NL];
  fe_reduce_once(c, t);
  limbs_to_u256(w, c);
}
// canonical words of x -> the words of its Montgomery-256 image (outputs that were produced canonically)
VRF_HD void u256_canon_to_mont256(uint32_t w[8]) {
  Fe<1, vrfk::V256> t;
  u256_to_limbs(t.v, w);
  FeN k;
#pragma unroll
  for (int i = 0; i < NL; ++i) k.v[i] = vrfk::R2_29[i];
  fe_to_mont256(w, fe_mul(t, k));
}

// 512-bit integer (16 x u32 LE) mod q -> Montgomery (hash_to_field, 48-byte inputs fit)
VRF_HD Fe<1, 4> fe_from_u512(const uint32_t w[16]) {
  Fe<1, vrfk::V256> lo, hi;
  u256_to_limbs(lo.v, w);
  u256_to_limbs(hi.v, w + 8);
  FeN a = fe_mul(lo, fe_const(vrfk::R2_29));
  FeN b = fe_mul(hi, fe_const(vrfk::TWO256_R2));
  return fe_norm(fe_add(a, b));
}

// ------------------------------------------------------------------ fixed exponentiation
// x^e by a generated sliding-window program (constants.gen.h POW_*_PROG, tools/gen_constants.py): word 0
// selects the start value among the odd powers x^1..x^15, every later word is (squarings << 4) | index of
// the odd power to multiply by (15 = none).  The program is the same for every lane: scalar control flow.
// x^(q-2): 253 squarings + 60 multiplications; x^((t-1)/2): 220 + 52 (fixed 3-bit windows took 85 / 80).
template <int LEN>
VRF_HD FeN fe_pow_prog(const FeN& x, const uint16_t (&prog)[LEN]) {
  FeN t[8];
  t[0] = x;
  const FeN x2 = fe_sqr(x);
#pragma unroll
  for (int i = 1; i < 8; ++i) t[i] = fe_mul(t[i - 1], x2);
  auto pick = [&](uint32_t idx) {
    FeN s = t[0];
#pragma unroll
    for (int j = 1; j < 8; ++j)
      if (idx == (uint32_t)j) s = t[j];
    return s;
  };
  FeN acc = pick(prog[0] & 15u);
#pragma unroll 1
  for (int i = 1; i < LEN; ++i) {
    const uint32_t op = prog[i], nsq = op >> 4, idx = op & 15u;
#pragma unroll 1
    for (uint32_t k = 0; k < nsq; ++k) acc = fe_sqr(acc);
    if (idx != 15u) acc = fe_mul(acc, pick(idx));
  }
  return acc;
}

template <int L, int V>
VRF_HD FeN fe_inv_pow(const Fe<L, V>& a) {   // a^(q-2); 0 -> 0
  FeN x = fe_mul(a, fe_one());
  return fe_pow_prog(x, vrfk::POW_INV_PROG);
}

// ------------------------------------------------------------------ square root
// Table-driven Tonelli-Shanks.  q - 1 = 2^S t, g = Z^t generates the 2^S-torsion (Z the field's non-residue: 5, 2, 5),
// h = 1/g.  w^t = g^e; the discrete logarithm e is read off digit by digit: a power of w^t that depends on the digits
// found so far and the next one only, corrected by table entries h^(j 2^level), lands in the 2^8-torsion, where a
// perfect hash of the canonical low limb (lut = SQRT_LUT) gives the digit.  Then sqrt(w) = w^((t+1)/2) h^(e/2).
//   S = 32 (BLS12-381 Fr): byte digits; tables k = 0..3 at levels 0, 8, 16, 24.  220 + 24 squarings.
//   S = 28 (BN254 Fr): digits 8 | 8 | 8 | 4; the same four tables plus levels 4 and 12 (k = 4, 5).
//   S = 2 (2^255 - 19): the 4-torsion is four constants, no table.
//   S = 1 (P-256): the exponentiation is the root.
// Returns is_square(w) and sets `root` to sqrt(w) if w is a square, else to sqrt(Z*w) (Z doubles as the Elligator
// non-residue of the Bandersnatch suite).  Constant shape.
VRF_HD uint32_t sqrt_lut_index(const SqrtTables& T, const FeN& y) {
  FeN c = fe_canon(y);
  uint32_t h = (c.v[0] * vrfk::SQRT_LUT_MULT) >> (32 - vrfk::SQRT_LUT_BITS);
  return T.lut[h];
}
VRF_HD FeN sqrt_tbl(const SqrtTables& T, int k, uint32_t j) {
  return fe_load<1, 2>(T.P + ((size_t)k * 256 + j) * NL);
}
VRF_HD bool limbs_eq(const FeN& a, const uint32_t (&c)[NL]) {
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < NL; ++i) o |= a.v[i] ^ c[i];
  return o == 0;
}

// root = w^((t+1)/2) h^(e/2) (e even) or sqrt(Z w) = Z^((t+1)/2) w^((t+1)/2) h^((e+1)/2) (e odd); returns e even.
// INV: x0 is w^((t-1)/2) instead, and root = w^((t-1)/2) h^(e/2) = 1 / sqrt(w) for e even (the product with the line
// above is w^t h^e = 1); for e odd it is left as that product stands, which no caller reads.
template <bool INV>
VRF_HD bool sqrt_finish(FeN& root, const FeN& x0, uint32_t e, const SqrtTables& T) {
  bool odd = e & 1;
  uint32_t half = (e >> 1) + (e & 1);               // in [0, 2^31]
  FeN r = fe_mul(x0, sqrt_tbl(T, 0, half & 255));
  r = fe_mul(r, sqrt_tbl(T, 1, (half >> 8) & 255));
  r = fe_mul(r, sqrt_tbl(T, 2, (half >> 16) & 255));
  r = fe_mul(r, sqrt_tbl(T, 3, half >> 24));
  if constexpr (INV) {
    root = r;
  } else {
    FeN rz = fe_mul(r, fe_const(vrfk::SQRT_CZ_M));
    root = fe_select(odd, rz, r);
  }
  return !odd;    // w == 0: b = 0, lut garbage, but x0 = 0 => root = 0; caller treats 0 as square
}

// The walk behind fe_sqrt_or_zsqrt and fe_inv_sqrt (INV) below, on a normalised w.
template <bool INV>
VRF_HD bool fe_sqrt_walk(FeN& root, const FeN& w, const SqrtTables& T) {
  FeN v = fe_pow_prog(w, vrfk::POW_SQRT_PROG);        // w^((t-1)/2)
  FeN x0 = fe_mul(w, v);                            // w^((t+1)/2)
  FeN b = fe_mul(x0, v);                            // w^t, in the 2^S-torsion
  const FeN base = INV ? v : x0;
  if constexpr (vrfk::SQRT_S == 1) {
    static_assert(!INV, "no inverse root where the exponentiation is the root");
    // q = 3 (mod 4), Z = -1: x0 = w^((q+1)/4) squares to w chi(w), i.e. it is sqrt(w) or sqrt(Z w) as it stands
    root = x0;
    const FeN bc = fe_canon(b);                       // chi(w): 1, -1 or 0
    uint32_t nz = 0;
#pragma unroll
    for (int i = 0; i < NL; ++i) nz |= bc.v[i];
    return limbs_eq(bc, vrfk::ONE_M) || nz == 0;
  } else if constexpr (vrfk::SQRT_S == 2) {
#if VRF_FIELD == 1
    uint32_t e;
    // x0 = w^((q+3)/8); b = x0^2 / w is 1, -1 (root x0 / sqrt(-1)) or a primitive 4th root of unity (w a non-residue)
    const FeN bc = fe_canon(b);
    e = limbs_eq(bc, vrfk::SQRT_G1_M) ? 1u : limbs_eq(bc, vrfk::SQRT_G2_M) ? 2u : limbs_eq(bc, vrfk::SQRT_G3_M) ? 3u : 0u;
    const bool odd = e & 1;
    const uint32_t half = (e >> 1) + (e & 1);       // 0, 1, 1, 2
    const FeN hm = fe_select(half == 0, fe_one(), fe_select(half == 1, fe_const(vrfk::SQRT_H1_M), fe_const(vrfk::SQRT_H2_M)));
    FeN r = fe_mul(base, hm);
    if constexpr (INV) {
      root = r;
    } else {
      FeN rz = fe_mul(r, fe_const(vrfk::SQRT_CZ_M));
      root = fe_select(odd, rz, r);
    }
    return !odd;
#endif
  } else if constexpr (vrfk::SQRT_S == 28) {
    FeN b4 = b;
    for (int i = 0; i < 4; ++i) b4 = fe_sqr(b4);
    FeN b12 = b4;
    for (int i = 0; i < 8; ++i) b12 = fe_sqr(b12);
    FeN b20 = b12;
    for (int i = 0; i < 8; ++i) b20 = fe_sqr(b20);
    // b = g^e, e = e0 + e1 2^8 + e2 2^16 + e3 2^24, e3 < 16; the 2^8-torsion is generated by g^(2^20)
    uint32_t e0 = sqrt_lut_index(T, b20);
    uint32_t e1 = sqrt_lut_index(T, fe_mul(b12, sqrt_tbl(T, 5, e0)));
    uint32_t e2 = sqrt_lut_index(T, fe_mul(fe_mul(b4, sqrt_tbl(T, 4, e0)), sqrt_tbl(T, 5, e1)));
    uint32_t e3 = sqrt_lut_index(
        T, fe_mul(fe_mul(fe_mul(b, sqrt_tbl(T, 0, e0)), sqrt_tbl(T, 1, e1)), sqrt_tbl(T, 2, e2))) >> 4;
    return sqrt_finish<INV>(root, base, e0 | (e1 << 8) | (e2 << 16) | (e3 << 24), T);
  } else {
    static_assert(vrfk::SQRT_S <= 2 || vrfk::SQRT_S == 28 || vrfk::SQRT_S == 32, "no square-root plan for this 2-adicity");
    FeN b8 = b;
    for (int i = 0; i < 8; ++i) b8 = fe_sqr(b8);
    FeN b16 = b8;
    for (int i = 0; i < 8; ++i) b16 = fe_sqr(b16);
    FeN b24 = b16;
    for (int i = 0; i < 8; ++i) b24 = fe_sqr(b24);
    // b = g^e, e = e0 + e1 2^8 + e2 2^16 + e3 2^24
    uint32_t e0 = sqrt_lut_index(T, b24);
    uint32_t e1 = sqrt_lut_index(T, fe_mul(b16, sqrt_tbl(T, 2, e0)));
    uint32_t e2 = sqrt_lut_index(T, fe_mul(fe_mul(b8, sqrt_tbl(T, 1, e0)), sqrt_tbl(T, 2, e1)));
    uint32_t e3 = sqrt_lut_index(
        T, fe_mul(fe_mul(fe_mul(b, sqrt_tbl(T, 0, e0)), sqrt_tbl(T, 1, e1)), sqrt_tbl(T, 2, e2)));
    return sqrt_finish<INV>(root, base, e0 | (e1 << 8) | (e2 << 16) | (e3 << 24), T);
  }
}

template <int L, int V>
VRF_HD bool fe_sqrt_or_zsqrt(FeN& root, const Fe<L, V>& w_in, const SqrtTables& T) {
  return fe_sqrt_walk<false>(root, fe_mul(w_in, fe_one()), T);
}

// 1 / sqrt(w) from the same exponentiation, the same discrete-logarithm walk and the same four table products: with
// v = w^((t-1)/2), x0 = w v and x0 v = w^t = g^e, sqrt(w) = x0 h^(e/2) and 1 / sqrt(w) = v h^(e/2).  Returns
// is_square(w) and sets `root` to the inverse root if w is a non-zero square and to 0 if w = 0 (v = 0; the caller treats
// 0 as a square, as with fe_sqrt_or_zsqrt); for a non-square w `root` is not a root of anything.  For the fields whose
// 2-adicity has a table plan or the four constants (S = 32, 28, 2).  Constant shape.
#if VRF_FIELD != 3
VRF_HD bool fe_inv_sqrt(FeN& root, const FeN& w, const SqrtTables& T) { return fe_sqrt_walk<true>(root, w, T); }
#endif


// Low byte of the 2-adic discrete logarithm: w = (odd-order part) * g^e with g the generator of the
// 2^S-torsion behind the square-root tables; returns e mod 256.  w (non-zero) is a 2^k-th power, k <= 8, iff
// 2^k divides the result.  One fixed exponentiation (220 + 24 squarings for S = 32), constant shape.
template <int L, int V>
VRF_HD uint32_t fe_dlog2_low8(const Fe<L, V>& w_in, const SqrtTables& T) {
  static_assert(L > 0 && vrfk::SQRT_S >= 8, "the field has no 2^8-torsion");
  FeN w = fe_mul(w_in, fe_one());
  FeN v = fe_pow_prog(w, vrfk::POW_SQRT_PROG);        // w^((t-1)/2)
  FeN b = fe_mul(fe_mul(w, v), v);                  // w^t, in the 2^S-torsion
  for (int i = 0; i < vrfk::SQRT_S - 8; ++i) b = fe_sqr(b);       // g^(e 2^(S-8)): depends on e mod 2^8 only
  return sqrt_lut_index(T, b);
}

// ------------------------------------------------------------------ quadratic character (Jacobi symbol)
// Is w a non-zero square?  The Euler criterion costs an exponentiation (~255 squarings, ~58 k instruction
// slots).  Here: the Jacobi symbol (g / q) by "positive divsteps" (Bernstein-Yang safegcd with the sum in
// place of the difference, so f and g stay non-negative and quadratic reciprocity applies as is):
//     g odd and eta < 0 : swap (f, g), eta = -eta       sign flips iff f = g = 3 (mod 4)
//     g odd             : g += f                        (g / f) depends on g mod f only
//     then              : g /= 2, eta -= 1              sign flips iff f = 3, 5 (mod 8)
// The pair converges to f = g = gcd; the symbol is known once f = 1.  Every decision reads the low bits of f
// and g and the counter eta only, so a round of JAC_K = 29 steps runs on the low 32-bit words (one VGPR each) and
// yields a 2x2 matrix of non-negative entries, each row summing to at most 2^29 (every step doubles the f row and
// adds it to the g row at most once); applying it to the 9-limb numbers divides by 2^29 exactly, i.e. drops one
// 29-bit limb, and the 64-bit column sums stay below 2 * 2^29 * 2^29 + carry < 2^60.
// The steps run several at a time (libsecp256k1's variable-time "posdivsteps"): all trailing zeros of g in one shift,
// then, with g odd and eta >= 0 after the swap, up to min(eta + 1, steps left, 4) low bits of g cleared at once by
// g += f w, w = -g / f (mod 2^k).  eta + 1 bounds k because no swap can come before eta turns negative, so the batch is
// the single steps' own sequence and the matrix, the sign and eta come out identical.
// Rounds are paced evenly (jac_steps_paced): a round is JAC_NITER such trips, the same for every lane, and takes the
// s <= 29 steps those trips give the lane; its matrix is scaled by 2^(29 - s), so the column code still drops one limb
// exactly and the lane has divided by 2^s.  The divsteps sequence, the sign and eta are the single steps' own, cut at
// other places.  Running exactly 29 steps per round instead cost a wave the trips of its slowest lane in every round
// (~13 against ~9 for a lane, a third of the loop under a partly empty mask); a lane's total trips average out over
// its ~30 rounds, so the wave's maximum of whole rounds is 12 % above the lane's mean where the maximum of trips was 44 %.
// JAC_NITER = 8, from the compiled loop on gfx950 (36 VALU per unrolled trip, ~160 per round for the matrix product,
// the final shift and the bookkeeping; the parent's divergent trip ~45 slots with its mask handling) and the rounds a
// wave of 64 random inputs below q needs (300 waves; lane mean / wave maximum):
//     NITER   rounds         slots per symbol and wave
//     7       30.6 / 34.9    14.4 k
//     8       28.2 / 31.6    14.2 k        (29 steps, wave-maximum trips: 28.2 / 29, 21 k)
//     9       27.0 / 29.7    14.4 k
//     10      26.5 / 28.8    15.0 k
// JAC_VAR_ROUNDS: every trip of a running lane takes at least one step, and a single step (eta = 0, k = 1) leaves
// eta = -1, so the next trip swaps and takes at least two: a round is worth >= 12 steps however the input was chosen, and
// inputs that keep eta small ride the cycle of two steps per trip.  Random inputs need <= 36 rounds (1.2e5 samples per
// field, the tail falls ~5x per round); 2^k, q - 2^k, values with long runs of low zeros and the Montgomery images of
// 1, 2, q - 1 need up to 48.  The cap is 62, as far as fe_inv's value bound lets it go; a lane beyond it takes the
// exponentiation, as before.  The symbol also keeps the step budget of 40 rounds of 29 (JAC_STEP_BUDGET), so that it gives
// up exactly where it did (tests/test_divsteps.py pins that set): q - 2, q - 2^21 of 2^255 - 19 are such inputs.
// chi(R) = chi(2)^261 = 1 because q = 1 (mod 8) for both Montgomery fields (and R = 1 for 2^255 - 19): the symbol of
// the stored image is the symbol of the value.
static_assert(vrfk::CHI_R == 1, "jacobi_limbs callers assume chi(R) = 1");
constexpr int JAC_K = 29;
constexpr int JAC_MAX_ROUNDS = 40;      // the prover's fixed count of full 29-step rounds (jac_steps_ct): <= 30 needed in 3e4 samples
#ifndef VRF_JAC_NITER
#define VRF_JAC_NITER 8
#endif
constexpr int JAC_NITER = VRF_JAC_NITER;   // trips of an evenly paced round (the table above; -DVRF_JAC_NITER=7, 9 built the kernels timed beside it: DESIGN.md section 4)
constexpr int JAC_VAR_ROUNDS = 62;      // cap of the evenly paced rounds (above)
// A compatibility constraint, not a need of the algorithm: the symbol gives up on the inputs it gave up on with rounds of
// 29 steps, i.e. once the 40 * 29 steps of those are spent, because tests/test_divsteps.py pins that set with its model of
// single steps.  Without it the cap of 62 rounds would answer some of them (q - 2^21 of 2^255 - 19 in 58 rounds).
constexpr int JAC_STEP_BUDGET = JAC_K * JAC_MAX_ROUNDS;
static_assert(JAC_VAR_ROUNDS + 1 < 64, "fe_inv: d < (rounds + 1) q must stay inside the value bound of its result");
static_assert(JAC_K + 3 <= 32, "after JAC_K steps the low words must still hold the bits 1 and 2 that the sign reads");

// wave-level "any lane" on the device, identity on the host build
VRF_HD bool vrf_any(bool x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __any((int)x) != 0;
#else
  return x;
#endif
}

// The matrix of one round: 2^JAC_K (f', g') = (u f + v g, q f + r g).
struct JacTrans { uint32_t u, v, q, r; };

// JAC_K steps one at a time, branch-free and of fixed shape (the prover's constant-time inversion).
VRF_HD int32_t jac_steps_ct(int32_t eta, uint32_t f, uint32_t g, JacTrans& t) {
  uint32_t u = 1, v = 0, q = 0, r = 1;
#pragma unroll
  for (int i = 0; i < JAC_K; ++i) {
    const uint32_t m = 0u - (g & 1u);                        // g odd
    const uint32_t sw = m & (uint32_t)(eta >> 31);           // ... and eta < 0: swap
    uint32_t x = (f ^ g) & sw; f ^= x; g ^= x;
    x = (u ^ q) & sw; u ^= x; q ^= x;
    x = (v ^ r) & sw; v ^= x; r ^= x;
    eta = (eta ^ (int32_t)sw) - (int32_t)sw;
    g += f & m; q += u & m; r += v & m;
    g >>= 1; u <<= 1; v <<= 1; eta -= 1;
  }
  t = JacTrans{u, v, q, r};
  return eta;
}

// One evenly paced round: JAC_NITER trips of the variable-time batch above, or fewer once `left` steps (JAC_K, or 0 for a
// lane that idles) are used up, then the trailing zeros of g that the steps left still cover.  Returns the steps taken,
// s <= left; eta is updated in place.  SIGN: bit 1 of `jac` follows the sign of the symbol.  The trip count is the same
// for every lane, so the loop unrolls and no lane waits under the mask for the slowest of its wave; a lane out of steps
// (i = 0) is inert in a trip: the sentinel makes z = 0, it does not swap, and k = 0 makes w = 0.
// Every partial matrix is the single steps' matrix at some step, so no entry exceeds 2^s: u w and v w are the f row after
// k more doublings and fit 32 bits like the rest.
template <bool SIGN>
VRF_HD int jac_steps_paced(int32_t& eta_io, uint32_t f, uint32_t g, int left, JacTrans& t, uint32_t& jac) {
  uint32_t u = 1, v = 0, q = 0, r = 1;
  int32_t eta = eta_io;
  int i = left;
#pragma unroll
  for (int trip = 0; trip <= JAC_NITER; ++trip) {
    const int z = __builtin_ctz(g | (~0u << i));             // steps with g even, at most the i left (sentinel bit)
    g >>= z; u <<= z; v <<= z; eta -= z; i -= z;
    if (SIGN) jac ^= (f ^ (f >> 1)) & ((uint32_t)z << 1);  // (2 / f)^z: -1 iff f = 3, 5 (mod 8) and z odd
    if (trip == JAC_NITER) break;                            // the last pass only takes the zeros the last trip made
    const bool sw = i != 0 && eta < 0;                       // g odd: swap if eta < 0
    if (SIGN) jac ^= sw ? f & g : 0u;
    const uint32_t nf = sw ? g : f, ng = sw ? f : g, nu = sw ? q : u, nq = sw ? u : q, nv = sw ? r : v, nr = sw ? v : r;
    f = nf; g = ng; u = nu; q = nq; v = nv; r = nr;
    eta = sw ? -eta : eta;
    // k = min(eta + 1, i, 4); a lane with i = 0 may hold eta < -1, which the unsigned minimum turns into k = 0 as well
    uint32_t k = (uint32_t)(eta + 1) < (uint32_t)i ? (uint32_t)(eta + 1) : (uint32_t)i;
    k = k < 4u ? k : 4u;
    // w = -g / f (mod 2^k): f (f^2 - 2) = -1 / f (mod 16); the operands are cut to 4 bits so the products are 24-bit ones
    const uint32_t f4 = f & 15u, g4 = g & 15u;
    const uint32_t w = (g4 * f4 * ((f4 * f4 + 14u) & 15u)) & ((1u << k) - 1u);
    g += f * w; q += u * w; r += v * w;                      // clears the k low bits of g; the next shift takes them
  }
  // s = left - i steps were taken: scale by 2^(JAC_K - s) so that the callers' exact division by 2^JAC_K divides by 2^s,
  // (2^(K-s) u f + 2^(K-s) v g) / 2^K = (u f + v g) / 2^s.  Entries and row sums stay <= 2^JAC_K.
  const int pad = JAC_K - (left - i);
  t = JacTrans{u << pad, v << pad, q << pad, r << pad};
  eta_io = eta;
  return left - i;
}

// x: exact 29-bit limbs of an integer in [0, 2q), below 2^256.  Returns +1 / -1, 0 if x = 0 (mod q), 2 if the lane gave up:
// f = 1 not seen at the end of a round within JAC_STEP_BUDGET steps or JAC_VAR_ROUNDS rounds.
VRF_HD int jacobi_limbs(const uint32_t x[NL], int* rounds_out = nullptr) {
  uint32_t f[NL], g[NL], d[NL];
  // inputs are < 2q; one in [q, 2q) goes in as x - q (this replaces the test x == q: callers pass fe_canon's [0, q)): the rounds pace themselves on values below f (q + 1 as it stands
  // would ride the slow cycle for 83 rounds where q = 2^255 - 19)
  uint32_t borrow = 0;
#pragma unroll
  for (int i = 0; i < NL; ++i) {
    const uint32_t t = x[i] - vrfk::Q29[i] - borrow;
    borrow = t >> 31;
    d[i] = (i < NL - 1) ? (t & LMASK) : t;
  }
  uint32_t nz = 0;
#pragma unroll
  for (int i = 0; i < NL; ++i) { f[i] = vrfk::Q29[i]; g[i] = borrow ? x[i] : d[i]; nz |= g[i]; }
  const bool zero = nz == 0;
  int32_t eta = -1;
  uint32_t jac = 0;                               // bit 1 carries the sign
  bool done = zero;
  int rounds = 0, steps = 0;
#pragma unroll 1
  for (int round = 0; round < JAC_VAR_ROUNDS; ++round) {
    const bool idle = done || steps >= JAC_STEP_BUDGET;       // finished, or given up
    if (!vrf_any(!idle)) break;
    rounds += idle ? 0 : 1;
    const uint32_t f0 = f[0] | (f[1] << LW), g0 = g[0] | (g[1] << LW);
    uint32_t jl = jac;
    JacTrans t;
    int32_t e = eta;
    // the last round stops at the budget, where the rounds of 29 steps looked at f for the last time
    const int room = JAC_STEP_BUDGET - steps;
    steps += jac_steps_paced<true>(e, f0, g0, idle ? 0 : (room < JAC_K ? room : JAC_K), t, jl);
    const uint32_t u = t.u, v = t.v, q = t.q, r = t.r;
    // (f, g) <- (u f + v g, q f + r g) / 2^29, the matrix scaled so that this is the round's 2^s: the low limb of both
    // sums is zero by construction
    uint32_t nf[NL], ng[NL];
    uint64_t af = mad(u, f[0], (uint64_t)v * g[0]) >> LW, ag = mad(q, f[0], (uint64_t)r * g[0]) >> LW;
#pragma unroll
    for (int i = 1; i < NL; ++i) {
      af = mad(u, f[i], mad(v, g[i], af));
      ag = mad(q, f[i], mad(r, g[i], ag));
      nf[i - 1] = (uint32_t)af & LMASK; af >>= LW;
      ng[i - 1] = (uint32_t)ag & LMASK; ag >>= LW;
    }
    nf[NL - 1] = (uint32_t)af; ng[NL - 1] = (uint32_t)ag;
    uint32_t rest = 0;
#pragma unroll
    for (int i = 1; i < NL; ++i) rest |= nf[i];
    const bool now_one = nf[0] == 1u && rest == 0;
    // lanes that had finished keep their state (f = 1 is not absorbing under further steps)
#pragma unroll
    for (int i = 0; i < NL; ++i) { f[i] = idle ? f[i] : nf[i]; g[i] = idle ? g[i] : ng[i]; }
    eta = idle ? eta : e;
    jac = idle ? jac : jl;
    done = done || (!idle && now_one);
  }
  if (rounds_out) *rounds_out = rounds;
  if (zero) return 0;
  if (!done) return 2;
  return (jac & 2u) ? -1 : 1;
}

// w is a non-zero square.  The fall-back (rounds exhausted; not observed) is the exponentiation.
template <int L, int V>
VRF_HD bool fe_is_nonzero_square(const Fe<L, V>& w, const SqrtTables& T) {
  const FeN c = fe_canon(w);
  const int j = jacobi_limbs(c.v);
  if (j == 2) {
    FeN root;
    return fe_sqrt_or_zsqrt(root, c, T) && !fe_is_zero(c);
  }
  return j == 1;
}

// w is a square (zero included)
template <int L, int V>
VRF_HD bool fe_is_square_or_zero(const Fe<L, V>& w, const SqrtTables& T) {
  const FeN c = fe_canon(w);
  const int j = jacobi_limbs(c.v);
  if (j == 2) {
    FeN root;
    return fe_sqrt_or_zsqrt(root, c, T) || fe_is_zero(c);
  }
  return j >= 0;
}

// ------------------------------------------------------------------ inversion
// 1 / a by the positive divsteps of the Jacobi symbol above with the cofactors kept: f = q, g = the canonical Montgomery
// image a~, and f = d a~, g = e a~ (mod q) throughout.  The round's 2x2 matrix (entries <= 2^29, rows summing to at most
// 2^29) is applied to (f, g) -- an exact division by 2^29 -- and to (d, e), where the multiple of q that makes the division
// exact is (low limb) * (-q^-1 mod 2^29): -(low limb) when q = 1 (mod 2^29).  f = 1 ends a lane with d = a~^-1 < (rounds + 1) q:
// each round maps d, e < k q to u d + v e + md q < (2^29 k + 2^29) q / 2^29 = (k + 1) q.  The rounds are the evenly
// paced ones of the symbol (jac_steps_paced: eight trips, s <= 29 steps, the matrix scaled by 2^(29 - s), so that (d, e)
// are divided by 2^s like (f, g)): ~28 for a lane, ~32 for a wave; row sums stay <= 2^29, so the bound on d holds with the
// rounds counted as they are now.  Against 255 squarings + 30 products (~60 k) for a^(q-2).  0 -> 0, as the power gives.
// CT = true (the prover's inversions: the Z coordinates of sk*H, k*H, k*G depend on secrets): every lane runs all
// JAC_MAX_ROUNDS rounds of 29 single steps (jac_steps_ct), so the time no longer follows the operand.
// Verification and decoding invert public data and keep the early exit and the variable steps.
template <bool CT = false, int L, int V>
VRF_HD FeN fe_inv(const Fe<L, V>& a, int* rounds_out = nullptr) {
  const FeN c = fe_canon(a);
  uint32_t f[NL], g[NL], d[NL], e[NL];
  uint32_t nz = 0;
#pragma unroll
  for (int i = 0; i < NL; ++i) { f[i] = vrfk::Q29[i]; g[i] = c.v[i]; d[i] = 0; e[i] = (i == 0); nz |= c.v[i]; }
  int32_t eta = -1;
  bool done = nz == 0;
  int rounds = 0;
#pragma unroll 1
  for (int round = 0; round < (CT ? JAC_MAX_ROUNDS : JAC_VAR_ROUNDS); ++round) {
    if (!CT && !vrf_any(!done)) break;
    rounds += done ? 0 : 1;
    const uint32_t f0 = f[0] | (f[1] << LW), g0 = g[0] | (g[1] << LW);
    JacTrans t;
    int32_t et = eta;
    if constexpr (CT) {
      et = jac_steps_ct(eta, f0, g0, t);
    } else {
      uint32_t no_sign = 0;
      jac_steps_paced<false>(et, f0, g0, done ? 0 : JAC_K, t, no_sign);
    }
    const uint32_t u = t.u, v = t.v, q = t.q, r = t.r;
    uint32_t nf[NL], ng[NL], nd[NL], ne[NL];
    uint64_t af = mad(u, f[0], (uint64_t)v * g[0]) >> LW, ag = mad(q, f[0], (uint64_t)r * g[0]) >> LW;
    const uint64_t td = mad(u, d[0], (uint64_t)v * e[0]), te = mad(q, d[0], (uint64_t)r * e[0]);
    // the multiple of q that clears the low limb: -(low limb) when q = 1 (mod 2^29), (low limb) * (-q^-1) in general
    const uint32_t md = ((uint32_t)td * vrfk::NINV29) & LMASK, me = ((uint32_t)te * vrfk::NINV29) & LMASK;
    uint64_t ad = mad(md, vrfk::Q29[0], td) >> LW, ae = mad(me, vrfk::Q29[0], te) >> LW;
#pragma unroll
    for (int i = 1; i < NL; ++i) {
      af = mad(u, f[i], mad(v, g[i], af));
      ag = mad(q, f[i], mad(r, g[i], ag));
      ad = mad(u, d[i], mad(v, e[i], mad(md, vrfk::Q29[i], ad)));
      ae = mad(q, d[i], mad(r, e[i], mad(me, vrfk::Q29[i], ae)));
      nf[i - 1] = (uint32_t)af & LMASK; af >>= LW;
      ng[i - 1] = (uint32_t)ag & LMASK; ag >>= LW;
      nd[i - 1] = (uint32_t)ad & LMASK; ad >>= LW;
      ne[i - 1] = (uint32_t)ae & LMASK; ae >>= LW;
    }
    nf[NL - 1] = (uint32_t)af; ng[NL - 1] = (uint32_t)ag; nd[NL - 1] = (uint32_t)ad; ne[NL - 1] = (uint32_t)ae;
    uint32_t rest = 0;
#pragma unroll
    for (int i = 1; i < NL; ++i) rest |= nf[i];
    const bool now_one = nf[0] == 1u && rest == 0;
#pragma unroll
    for (int i = 0; i < NL; ++i) {           // a finished lane keeps its state
      f[i] = done ? f[i] : nf[i]; g[i] = done ? g[i] : ng[i];
      d[i] = done ? d[i] : nd[i]; e[i] = done ? e[i] : ne[i];
    }
    eta = done ? eta : et;
    done = done || now_one;
  }
  if (rounds_out) *rounds_out = done ? rounds : -1;
  if (vrf_any(!done)) {                       // rounds exhausted (not observed): the power, for the whole wave
    const FeN slow = fe_inv_pow(a);
    if (!done) return slow;
  }
  // d < (JAC_VAR_ROUNDS + 1) q = 63 q.  A 256-bit q (P-256, VMAX = 32) puts that above the typed range: there the top
  // limb is < 2^30 (declared as L = 2) and the first product below is by the constant R^2 mod q < q, so its value is
  // < q (1 + 63 q / R) < 2.97 q, inside what mul_v(32, 2) = 3 claims for it.
  Fe<(vrfk::VMAX < 64 ? 2 : 1), (vrfk::VMAX < 64 ? vrfk::VMAX : 64)> dd;
#pragma unroll
  for (int i = 0; i < NL; ++i) dd.v[i] = nz == 0 ? 0u : d[i];
  // d = a^-1 / R as an integer: two Montgomery products by R^2 give a^-1 R
  return fe_mul(fe_mul(dd, fe_const(vrfk::R2_29)), fe_const(vrfk::R2_29));
}

VRF_NS_END
