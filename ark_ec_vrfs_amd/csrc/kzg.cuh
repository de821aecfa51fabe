// kzg.cuh -- per-lane functions of the KZG opening check (k_kzg.hip): `KZG10::check` / `KZG10::batch_check` of
// ark-poly-commit for the plain single-point opening, the check that ends `ring::Verifier::verify`
// (src/lib.rs:14 `ring`).  An opening (C, z, v, pi) holds iff e(C - v g + z pi, h) e(-pi, beta_h) = 1.
//
// Batched, the 128-bit weights r_i go INSIDE the sums, so n openings cost three multi-scalar multiplications, one sum in
// Fr and ONE pairing -- no per-item ladder:
//     S_A = sum r_i C_i + sum (r_i z_i mod r) pi_i - (sum r_i v_i mod r) g,    S_B = -sum r_i pi_i.
// The scalar work is in Fr of BLS12-381 -- the base field of Bandersnatch, i.e. fe.cuh compiled for VRF_FIELD 0.  A weight
// is used as a PLAIN residue (its 9 limbs as they are, value < 2^128): plain x Montgomery gives a plain product, so
// r_i z_i comes out of one product ready for its canonical words, and the running sum of r_i v_i stays plain as well.
//
//   kzg_weight      r_i = SHA-512("vrfhip-kzg-rlc-v1" || seed || D || u64_le(i))[0..16], little-endian
//   kzg_prep_item   one item: both points (g1_load), z_i, v_i < r, the weight; writes the affine points and the digits of
//                   the short layout (C_i, pi_i under r_i) and of the full one (pi_i under r_i z_i); returns r_i v_i.
//                   An invalid item has zero digits everywhere and returns zero.
//   kzg_acc         a + b brought back to the strict storage form (one product by R): the lazy-limb bounds of fe.cuh do
//                   not let an unbounded running sum compile, and every round of the reductions goes through here
//   kzg_fold_finish point n of the full layout: g under -sum r_i v_i; a coordinate >= p or g off the curve sets flag[0] = 2
//   kzg_combine     the one pairing item S_A || S_B from the three sums
//   kzg_item_rows   per-item form: the rows of the linear combination A_i = 1 C_i + z_i pi_i + (r - v_i) g and B_i = -pi_i
//                   (plain word arithmetic: p - y and r - v)
// All VRF_HD: tests/hostsim_kzg compiles them for the host.
#pragma once
#include "fe.cuh"
#include "sha512.cuh"
#include "g1_digits.cuh"
#include "g1_lincomb.cuh"        // lc_finish: a sum -> 24 wire words

namespace vrf {

static_assert(VRF_FIELD == 0, "kzg.cuh needs fe.cuh as Fr of BLS12-381");
static_assert(KZG_PART_WORDS == NL, "a partial sum is one Fe");

VRF_HD bool kzg_lt_r(const uint32_t k[8]) {
  bool lt = false, decided = false;
#pragma unroll
  for (int j = 7; j >= 0; --j)
    if (!decided && k[j] != vrfk::Q32[j]) { lt = k[j] < vrfk::Q32[j]; decided = true; }
  return lt;
}

VRF_HD void kzg_weight(uint32_t r[8], const uint8_t* seed, const uint8_t* root, uint64_t index) {
  Sha512 h;
  sha512_init(h);
  constexpr char tag[] = "vrfhip-kzg-rlc-v1";
#pragma unroll
  for (int j = 0; j < 17; ++j) sha512_put_byte(h, (uint8_t)tag[j]);
  sha512_put_bytes(h, seed, 32);
  sha512_put_bytes(h, root, 32);
#pragma unroll
  for (int j = 0; j < 8; ++j) sha512_put_byte(h, (uint8_t)(index >> (8 * j)));
  sha512_final(h);
#pragma unroll
  for (int j = 0; j < 4; ++j) { r[j] = sha512_word_mem(h, j); r[4 + j] = 0; }
}

VRF_HD FeN kzg_acc(const FeN& a, const FeN& b) { return fe_mul(fe_add(a, b), fe_one()); }

// canonical words of a strict value
VRF_HD void kzg_canon_words(uint32_t w[8], const FeN& a) {
  uint32_t c[NL];
  fe_reduce_once(c, a);
  limbs_to_u256(w, c);
}

// w = m - a for 0 < a < m (N little-endian words); a = 0 gives 0
template <int N>
VRF_HD void kzg_neg_words(uint32_t* w, const uint32_t* a, const uint32_t (&m)[N]) {
  uint32_t any = 0, borrow = 0;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    any |= a[j];
    const uint64_t t = (uint64_t)m[j] - a[j] - borrow;
    w[j] = (uint32_t)t;
    borrow = (uint32_t)(t >> 63);
  }
#pragma unroll
  for (int j = 0; j < N; ++j) w[j] = any ? w[j] : 0u;
}

VRF_HD FeN kzg_prep_item(const G1MsmLayout& S, const G1MsmLayout& F, size_t i, const uint32_t cw[24], const uint32_t pw[24],
                         const uint32_t z[8], const uint32_t v[8], const uint8_t* seed, const uint8_t* root, uint8_t* status) {
  bls::G1Aff C, Pi;
  bool c_inf, p_inf;
  bool ok = bls::g1_load(C, c_inf, cw);
  ok = bls::g1_load(Pi, p_inf, pw) && ok;
  ok = kzg_lt_r(z) && kzg_lt_r(v) && ok;
  uint32_t r[8];
  kzg_weight(r, seed, root, (uint64_t)i);
  Fe<1, 1> rp;                                   // the weight as a plain residue: 2^128 < r
  u256_to_limbs(rp.v, r);
  const FeN rz = fe_mul(rp, fe_from_u256(z));    // r_i z_i, plain
  const FeN rv = fe_mul(rp, fe_from_u256(v));
  uint32_t rzw[8];
  kzg_canon_words(rzw, rz);
  g1_store_affine(S.pts + i * G1_AFF_STRIDE, C);
  g1_store_affine(S.pts + (S.n + i) * G1_AFF_STRIDE, Pi);
  g1_store_affine(F.pts + i * G1_AFF_STRIDE, Pi);
  g1_write_digits(S.digits, S.n, i, S.windows, r, !ok || c_inf);
  g1_write_digits(S.digits + (size_t)S.windows * S.n, S.n, i, S.windows, r, !ok || p_inf);
  g1_write_digits(F.digits, F.n, i, F.windows, rzw, !ok || p_inf);
  status[i] = ok ? 0 : 2;
  return fe_select(ok, rv, fe_zero());
}

// total: sum r_i v_i (strict, plain); gw: g as 24 wire words
VRF_HD void kzg_fold_finish(const G1MsmLayout& F, const FeN& total, const uint32_t gw[24], uint8_t* flag) {
  bls::G1Aff G;
  bool g_inf;
  const bool ok = bls::g1_load(G, g_inf, gw);
  uint32_t t[8], k[8];
  kzg_canon_words(t, total);
  kzg_neg_words<8>(k, t, vrfk::Q32);
  const size_t slot = F.n - 1;
  g1_store_affine(F.pts + slot * G1_AFF_STRIDE, G);
  g1_write_digits(F.digits, F.n, slot, F.windows, k, !ok || g_inf);
  if (!ok) flag[0] = 2;
}

// a sum in the wire format (x || y, all-zero = infinity; valid by construction) -> projective
VRF_HD bls::G1P kzg_sum_load(const uint32_t w[24]) {
  bls::G1Aff A;
  bool inf;
  (void)bls::g1_load(A, inf, w);
  bls::G1P P;
  P.X = bls::fp_select(!inf, A.x, bls::FpS(bls::fp_zero()));
  P.Y = bls::fp_select(!inf, A.y, bls::FpS(bls::fp_one()));
  P.Z = bls::fp_select(!inf, bls::FpS(bls::fp_one()), bls::FpS(bls::fp_zero()));
  return P;
}
// -P on the wire form of a valid point: y -> p - y (infinity stays all-zero); !ok: all-0xFF
VRF_HD void kzg_neg_point(uint32_t out[24], const uint32_t in[24], bool ok) {
  uint32_t any = 0;
#pragma unroll
  for (int j = 0; j < 24; ++j) any |= in[j];
  uint32_t y[12];
  kzg_neg_words<12>(y, in + 12, vrfk::BLS_P_WORDS);
#pragma unroll
  for (int j = 0; j < 12; ++j) {
    out[j] = !ok ? 0xffffffffu : in[j];
    out[12 + j] = !ok ? 0xffffffffu : (any ? y[j] : 0u);
  }
}
VRF_HD void kzg_combine(uint32_t out[48], const uint32_t short_a[24], const uint32_t full_a[24], const uint32_t short_b[24],
                        bool vk_ok) {
  const bls::G1P sum = bls::g1_add(kzg_sum_load(short_a), kzg_sum_load(full_a));
  (void)bls::lc_finish(out, sum, vk_ok);
  kzg_neg_point(out + 24, short_b, vk_ok);
}

// c, pi: the decoded points (valid when dec_ok).  Returns whether the item is valid.
VRF_HD bool kzg_item_rows(uint32_t bases[48], uint32_t scalars[16], uint32_t shared[8], uint32_t neg_pi[24], const uint32_t c[24],
                          const uint32_t pi[24], bool dec_ok, const uint32_t z[8], const uint32_t v[8]) {
  const bool ok = dec_ok && kzg_lt_r(z) && kzg_lt_r(v);
  uint32_t rv[8];
  kzg_neg_words<8>(rv, v, vrfk::Q32);
#pragma unroll
  for (int j = 0; j < 24; ++j) {
    bases[j] = ok ? c[j] : 0xffffffffu;
    bases[24 + j] = ok ? pi[j] : 0xffffffffu;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    scalars[j] = ok ? (j == 0 ? 1u : 0u) : 0xffffffffu;
    scalars[8 + j] = ok ? z[j] : 0xffffffffu;
    shared[j] = ok ? rv[j] : 0xffffffffu;
  }
  kzg_neg_point(neg_pi, pi, ok);
  return ok;
}

}  // namespace vrf
