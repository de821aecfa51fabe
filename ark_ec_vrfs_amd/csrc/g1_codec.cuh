// g1_codec.cuh -- checked decoding, validation and encoding of BLS12-381 G1 points (the front
// of the batched pairing check).  Replaces `G1Affine::deserialize_compressed` / `::check` / `serialize_compressed` of
// ark-bls12-381 (`CanonicalDeserialize` with `Validate::Yes`: on the curve AND in the prime-order subgroup) for the 48-byte
// G1 elements of a ring proof and of a verifier key, so that vrfhip_pairing_check_batch* and vrfhip_g1_msm -- which take
// 96-byte affine points and leave subgroup membership to the caller -- can be fed from wire data on the same stream.
//
// Wire format (zcash / ark-bls12-381): x as a 48-byte BIG-endian integer; bit 7 of byte 0 = "compressed", bit 6 =
// "infinity", bit 5 = "y is the lexicographically larger root" (y > p - y).  The 96-byte form is the one the other BLS
// entry points read: x || y as 48-byte LITTLE-endian canonical integers, all-zero = infinity.
//
// One lane handles one point; every function compiles for the host too (the CPU test tier runs these very item functions).
//   fp_sqrt         p = 3 (mod 4): a^((p+1)/4) with a 3-bit fixed window (uniform exponent, scalar loop), accepted only if
//                   its square is a.
//   g1_in_subgroup  the endomorphism test arkworks uses for this curve (Scott, "A note on group membership tests for G1,
//                   G2 and GT on BLS pairing-friendly curves", 2021): phi(P) = -[x^2] P with phi(x, y) = (beta x, y) and
//                   x = -0xD201000000010000 the curve parameter; [x^2] P as two multiplications by |x| (63 doublings + 5
//                   additions each, the complete law of g1.cuh), compared projectively.  beta is generated and checked
//                   against the generator by tools/gen_constants.py (the other cube root of unity fails there).
//
// DEVIATION from ark-bls12-381 0.4, deliberate: an encoding with the infinity flag is accepted
// only in its canonical form 0xC0 00...00 -- the strict zcash rule.  arkworks, as far as is recalled here, returns infinity
// as soon as the flag is set without looking at the remaining bytes; no source at hand settles it.
#pragma once
#include "g1.cuh"

namespace bls {

// a^((p+1)/4); true (and *out a root) iff a is a square.  0 -> 0.
VRF_HD_NOINLINE bool fp_sqrt(FpS* out, const FpS* a) {
  FpN t[8];
  t[1] = fp_mul(*a, fp_one());
  t[2] = fp_sqr(t[1]);
  for (int i = 3; i < 8; ++i) t[i] = fp_mul(t[i - 1], t[1]);
  FpN acc = fp_one();
  bool started = false;
  for (int w = 126; w >= 0; --w) {                 // (p + 1) / 4 has 379 bits: 127 windows of 3
    const int bit = 3 * w;
    uint32_t d = vrfk::BLS_EXP_SQRT[bit >> 5] >> (bit & 31);
    if ((bit & 31) > 29 && (bit >> 5) + 1 < 12) d |= vrfk::BLS_EXP_SQRT[(bit >> 5) + 1] << (32 - (bit & 31));
    d &= 7;
    if (started) { acc = fp_sqr(acc); acc = fp_sqr(acc); acc = fp_sqr(acc); }
    if (d != 0) {
      FpN s = t[1];
      for (int j = 2; j < 8; ++j) if (d == (uint32_t)j) s = t[j];
      acc = started ? fp_mul(acc, s) : s;
      started = true;
    }
  }
  *out = acc;
  return fp_eq(fp_sqr(acc), *a);
}

// |x| = 0xD201000000010000 = 2^63 + 2^62 + 2^60 + 2^57 + 2^48 + 2^16: after the leading bit, runs of doublings each
// closed by one addition of the base (the last run by none).  The shape is fixed at compile time: no lane decides anything.
constexpr int XABS_RUNS = 6;
constexpr int XABS_RUN[XABS_RUNS] = {1, 2, 3, 9, 32, 16};
constexpr uint64_t xabs_from_runs() {
  uint64_t v = 1;
  for (int i = 0; i < XABS_RUNS; ++i) v = (v << XABS_RUN[i]) | (i + 1 < XABS_RUNS ? 1u : 0u);
  return v;
}
static_assert(xabs_from_runs() == X_ABS, "runs of |x|");

// [|x|] (x, y) for an affine base that is not the point at infinity
VRF_HD_NOINLINE void g1_mul_xabs_affine(G1P* out, const FpS* x, const FpS* y) {
  G1P acc;
  acc.X = *x; acc.Y = *y; acc.Z = fp_one();
#pragma unroll 1
  for (int i = 0; i < XABS_RUNS; ++i) {
    const int n = XABS_RUN[i];
#pragma unroll 1
    for (int j = 0; j < n; ++j) acc = g1_dbl(acc);
    if (i + 1 < XABS_RUNS) acc = g1_madd(acc, *x, *y, false);
  }
  *out = acc;
}
// [|x|] Q for a projective base
VRF_HD_NOINLINE void g1_mul_xabs_proj(G1P* out, const G1P* q) {
  G1P acc = *q;
#pragma unroll 1
  for (int i = 0; i < XABS_RUNS; ++i) {
    const int n = XABS_RUN[i];
#pragma unroll 1
    for (int j = 0; j < n; ++j) acc = g1_dbl(acc);
    if (i + 1 < XABS_RUNS) acc = g1_add(acc, *q);
  }
  *out = acc;
}

// (x, y): a finite point ON the curve.  True iff it lies in the subgroup of order r: phi(P) = -[x^2] P and [x] P != P.
// The second condition is arkworks' guard; it is stated there on [|x|] P, here both signs are refused ([|x|] P = +/- P
// holds for no point of order r, and costs two products).
VRF_HD bool g1_in_subgroup(const FpS& x, const FpS& y) {
  G1P q1, q2;
  g1_mul_xabs_affine(&q1, &x, &y);
  g1_mul_xabs_proj(&q2, &q1);
  const bool fixed = fp_eq(fp_mul(x, q1.Z), q1.X) &&
                     (fp_eq(fp_mul(y, q1.Z), q1.Y) || fp_eq(fp_mul(y, q1.Z), fp_neg(q1.Y))) && !fp_is_zero(q1.Z);
  const auto bx = fp_mul(x, fp_const(vrfk::BLS_BETA_M));
  const bool endo = fp_eq(fp_mul(bx, q2.Z), q2.X) && fp_eq(fp_mul(y, q2.Z), fp_neg(q2.Y)) && !fp_is_zero(q2.Z);
  return endo && !fixed;
}

// a > b as 384-bit little-endian integers
VRF_HD bool words12_gt(const uint32_t a[12], const uint32_t b[12]) {
  bool gt = false, decided = false;
#pragma unroll
  for (int i = 11; i >= 0; --i)
    if (!decided && a[i] != b[i]) { gt = a[i] > b[i]; decided = true; }
  return gt;
}

// in: the 48 wire bytes as 12 little-endian words (word k = bytes 4k .. 4k+3).  out: 24 words x || y.  Status 0 / 2.
// An invalid item's output is all 0xFF (a coordinate >= p: InvalidData to every BLS entry point), never the all-zero
// encoding of infinity, so a chained call that ignores the status cannot drop the term silently.
template <bool SUBGROUP>
VRF_HD uint32_t g1_decode_item(uint32_t out[24], const uint32_t in[12]) {
  const uint32_t top = __builtin_bswap32(in[0]);
  const bool compressed = (top >> 31) & 1, infinity = (top >> 30) & 1, sort = (top >> 29) & 1;
  uint32_t w[12];
#pragma unroll
  for (int j = 0; j < 11; ++j) w[j] = __builtin_bswap32(in[11 - j]);
  w[11] = top & 0x1fffffffu;
  uint32_t xnz = 0;
#pragma unroll
  for (int j = 0; j < 12; ++j) xnz |= w[j];
  FpS x, y;
  const bool lt = fp_from_words(x, w);
  const FpS rhs = fp_fit(fp_add(fp_mul(fp_sqr(x), x), fp_dbl(fp_dbl(fp_one()))));    // x^3 + 4
  const bool square = fp_sqrt(&y, &rhs);
  uint32_t yw[12], nyw[12];
  fp_to_words(yw, y);
  fp_to_words(nyw, fp_neg(y));
  const bool flip = words12_gt(yw, nyw) != sort;
  bool ok = compressed && lt && square;
  if constexpr (SUBGROUP) ok = g1_in_subgroup(x, y) && ok;
  if (infinity) ok = compressed && !sort && xnz == 0;
#pragma unroll
  for (int j = 0; j < 12; ++j) {
    out[j] = !ok ? 0xffffffffu : (infinity ? 0u : w[j]);
    out[12 + j] = !ok ? 0xffffffffu : (infinity ? 0u : (flip ? nyw[j] : yw[j]));
  }
  return ok ? PST_OK : PST_INVALID;
}

// the 96-byte affine form: coordinates < p, on the curve (g1_load), in the subgroup.  All-zero = infinity: valid.
VRF_HD uint32_t g1_validate_item(const uint32_t in[24]) {
  G1Aff P;
  bool inf;
  const bool ok = g1_load(P, inf, in);
  const bool sub = g1_in_subgroup(P.x, P.y);
  return (ok && (inf || sub)) ? PST_OK : PST_INVALID;
}

// the 96-byte affine form -> 48 wire bytes (12 little-endian words); infinity = 0xC0 00...; no subgroup test.
// Status 2 and an all-0xFF output when a coordinate is >= p or the point is off the curve.
VRF_HD uint32_t g1_encode_item(uint32_t out[12], const uint32_t in[24]) {
  G1Aff P;
  bool inf;
  const bool ok = g1_load(P, inf, in);
  uint32_t nyw[12];
  fp_to_words(nyw, fp_neg(P.y));
  const bool larger = words12_gt(in + 12, nyw);
#pragma unroll
  for (int k = 0; k < 12; ++k) out[k] = !ok ? 0xffffffffu : (inf ? 0u : __builtin_bswap32(in[11 - k]));
  if (ok) out[0] |= inf ? 0xc0u : (0x80u | (larger ? 0x20u : 0u));
  return ok ? PST_OK : PST_INVALID;
}

}  // namespace bls
