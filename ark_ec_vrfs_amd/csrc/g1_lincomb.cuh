// g1_lincomb.cuh -- per-item linear combinations of BLS12-381 G1 points (the middle of the
// batched pairing check).  A KZG / ring-proof verifier computes, per proof, A_i = sum s_ij C_ij + sum t_ij S_j and
// B_i = sum u_ij pi_ij from about a dozen points with full-size Fr scalars -- in arkworks a `VariableBaseMSM::msm` of that
// size per proof, far below what the Pippenger schedule of k_msm_g1.hip is built for.  Here one lane multiplies one term
// and the lanes of an item add their partial sums (k_g1_lincomb.hip); these are the per-lane functions, compiled for the
// host too (the CPU test tier runs them, with the lane reduction replaced by a sequential g1_add).
//
//   lc_recode     s -> s + C with C = sum_w 4 * 8^w, w = 0 .. 85: window w of the sum, minus 4, is a signed digit d_w in
//                 [-4, 3] with sum d_w 8^w = s.  One 9-word addition replaces the carry chain of the usual signed recoding
//                 and any window can be read on its own, so the ladder walks down from the top without storing digits.
//                 s < 2^255 = 8^85 and C < 0.58 * 8^86 keep the sum below 8^86: the top window, 85, is 4 or 5 (d = 0 or 1) --
//                 it takes what would be the carry out of window 84.
//   g1_mul_w3     [s] P: the table {P, 2P, 3P, 4P} projective in registers, then per window 3 g1_dbl + 1 g1_add of
//                 (+/-) table[|d|] picked by selects -- d = 0 adds the identity, which the complete law of g1.cuh takes like
//                 any other point.  The shape is fixed: no lane decides anything.  255 doublings + 86 additions + 3 for the
//                 table, about 3.1 k field products per term.
//   lc_term       one term from its wire form: g1_load (coordinates < p, on the curve), scalar < r, ladder.  A base at
//                 infinity, an invalid term and a padding lane run the ladder on the identity.
//   lc_finish     a sum -> 24 output words: affine (one inversion), all-zero for infinity, all 0xFF for an invalid item.
#pragma once
#include "g1.cuh"

namespace bls {

constexpr int LC_WINDOWS = 86;               // 3-bit windows of s + C
constexpr int LC_MAX_TERMS = 16;

// sp = k + C.  Window w of C is 4, so word j of C is 0x24924924 rotated by j mod 3 (32 = 2 mod 3); C stops at bit 258.
VRF_HD void lc_recode(uint32_t sp[9], const uint32_t k[8]) {
  constexpr uint32_t CW[3] = {0x24924924u, 0x49249249u, 0x92492492u};
  uint64_t c = 0;
#pragma unroll
  for (int j = 0; j < 9; ++j) {
    const uint32_t cw = j < 8 ? CW[j % 3] : (CW[8 % 3] & 3u);          // bits 256, 257 of C: window 85 = 4 -> bit 257
    c += (uint64_t)(j < 8 ? k[j] : 0u) + cw;
    sp[j] = (uint32_t)c;
    c >>= 32;
  }
}
// d_w in [-4, 3]
VRF_HD int lc_digit(const uint32_t sp[9], int w) {
  const int bit = 3 * w, wi = bit >> 5, sh = bit & 31;
  uint32_t lo = 0, hi = 0;
#pragma unroll
  for (int j = 0; j < 9; ++j) {
    if (j == wi) lo = sp[j];
    if (j == wi + 1) hi = sp[j];
  }
  const uint32_t v = (sh ? ((lo >> sh) | (hi << (32 - sh))) : lo) & 7u;
  return (int)v - 4;
}

VRF_HD G1P g1_select(bool c, const G1P& a, const G1P& b) {
  G1P r;
  r.X = fp_select(c, a.X, b.X); r.Y = fp_select(c, a.Y, b.Y); r.Z = fp_select(c, a.Z, b.Z);
  return r;
}

// [s] P for sp = lc_recode(s); P projective, the identity included
VRF_HD G1P g1_mul_w3(const G1P& P, const uint32_t sp[9]) {
  const G1P P2 = g1_dbl(P), P3 = g1_add(P2, P), P4 = g1_dbl(P2);
  const G1P id = g1_identity();
  G1P acc = g1_select(lc_digit(sp, LC_WINDOWS - 1) == 1, P, id);     // the top window is 0 or 1
#pragma unroll 1
  for (int w = LC_WINDOWS - 2; w >= 0; --w) {
#pragma unroll 1
    for (int j = 0; j < 3; ++j) acc = g1_dbl(acc);
    const int d = lc_digit(sp, w);
    const int a = d < 0 ? -d : d;
    G1P q = g1_select(a == 1, P, id);
    q = g1_select(a == 2, P2, q);
    q = g1_select(a == 3, P3, q);
    q = g1_select(a == 4, P4, q);
    q.Y = fp_select(d < 0, fp_neg(q.Y), q.Y);
    acc = g1_add(acc, q);
  }
  return acc;
}

// words: the base, 24 words x || y; k: the scalar, 8 words.  live = false: a padding lane (its inputs are read but count
// for nothing).  Returns false for an invalid term -- a coordinate >= p, a point off the curve, a scalar >= r.
VRF_HD bool lc_term(G1P& out, const uint32_t words[24], const uint32_t k[8], bool live) {
  G1Aff A;
  bool inf;
  bool ok = g1_load(A, inf, words);
  bool lt = false, decided = false;                  // scalar < r, as k_g1_prep_msm checks it
#pragma unroll
  for (int j = 7; j >= 0; --j)
    if (!decided && k[j] != vrfk::Q32[j]) { lt = k[j] < vrfk::Q32[j]; decided = true; }
  ok = (ok && lt) || !live;
  const bool use = live && ok && !inf;
  G1P P;
  P.X = fp_select(use, A.x, FpS(fp_zero()));
  P.Y = fp_select(use, A.y, FpS(fp_one()));
  P.Z = fp_select(use, FpS(fp_one()), FpS(fp_zero()));
  uint32_t sp[9];
  lc_recode(sp, k);
  out = g1_mul_w3(P, sp);
  return ok;
}

// the item's sum -> x || y as 2 x 12 little-endian words; the codec's rule for an invalid item (g1_codec.cuh)
VRF_HD uint32_t lc_finish(uint32_t out[24], const G1P& sum, bool ok) {
  FpS x, y;
  g1_to_affine(x, y, sum);                            // the identity gives (0, 0)
  uint32_t xw[12], yw[12];
  fp_to_words(xw, x);
  fp_to_words(yw, y);
  const bool inf = g1_is_identity(sum);
#pragma unroll
  for (int j = 0; j < 12; ++j) {
    out[j] = !ok ? 0xffffffffu : (inf ? 0u : xw[j]);
    out[12 + j] = !ok ? 0xffffffffu : (inf ? 0u : yw[j]);
  }
  return ok ? PST_OK : PST_INVALID;
}

}  // namespace bls
