// kzg_multi.cuh -- per-lane functions of the multi-commitment, multi-point KZG opening check (k_kzg_multi.hip): the shape a
// ring proof ends in.  Item i has k own commitments C_ij under s_ij, the shared bases S_0 = g, S_1 .. S_m under t_ij and p
// opening proofs pi_ij at z_ij with coefficients u_ij, and holds iff e(A_i, h) e(B_i, beta_h) = 1 with
//     A_i = sum_j s_ij C_ij + sum_{j<=m} t_ij S_j + sum_j (u_ij z_ij mod r) pi_ij,      B_i = -sum_j u_ij pi_ij.
// Batched, the 128-bit weights r_i go inside the sums as in kzg.cuh -- two multi-scalar multiplications, m + 1 sums in Fr
// and ONE pairing, no per-item ladder:
//     S_A = sum_ij (r_i s_ij) C_ij + sum_ij (r_i u_ij z_ij) pi_ij + sum_{j<=m} (sum_i r_i t_ij) S_j,   S_B = -sum_ij (r_i u_ij) pi_ij.
// Layout A (sets = 1, full windows) holds the n (k + p) own terms, item by item (commitments, then proofs), and g, S_1 .. S_m
// as its last m + 1 points; layout B the n p proofs under r_i u_ij.  A weight is a PLAIN residue (kzg.cuh): plain x
// Montgomery gives a plain product ready for its canonical words.
//
//   kzgm_weight       r_i = SHA-512("vrfhip-kzg-multi-rlc-v1" || u32_le(k) || u32_le(m) || u32_le(p) || seed || D || u64_le(i))[0..16]
//   kzgm_item_valid   all k + p decode statuses 0 and all k + (m + 1) + 2 p scalars < r
//   kzgm_col_term     r_i t_ij (plain, strict), zero for an invalid item: what the block sums and the fold add up
//   kzgm_prep_term    one own term: the affine point and digit rows of layout A (and of B for a proof); an invalid item and
//                     a point at infinity have zero digits everywhere
//   kzgm_fold_finish  shared base j as point n (k + p) + j of layout A under sum_i r_i t_ij; a coordinate >= p or a point
//                     off the curve sets flag[0] = 2
//   kzgm_combine      the one pairing item S_A || S_B = A.sums[0] || -B.sums[0] (all-0xFF under a raised flag)
//   kzgm_item_rows    per-item form: the rows of the two linear combinations A_i and B_i (scalars r - u_ij), all-0xFF for an
//                     invalid item
// All VRF_HD: tests/hostsim_kzg_multi compiles them for the host.
#pragma once
#include "kzg.cuh"

namespace vrf {

struct KzgmShape { uint32_t k, m, p; };
constexpr uint32_t KZGM_MAX_TERMS = 16;          // k + p + m + 1: the limit of k_g1_lincomb
constexpr int KZGM_WEIGHT_WORDS = 4;             // a parked weight: 128 bits

VRF_HD bool kzgm_shape_ok(KzgmShape sh) {
  return sh.p >= 1 && sh.k <= KZGM_MAX_TERMS && sh.m <= KZGM_MAX_TERMS && sh.p <= KZGM_MAX_TERMS &&
         sh.k + sh.p + sh.m + 1 <= KZGM_MAX_TERMS;
}

template <int N>
VRF_HD void kzgm_load_words(uint32_t (&w)[N], const uint8_t* p) {
  const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
#pragma unroll
  for (int j = 0; j < N; ++j) w[j] = q[j];
}
// !ok: all-0xFF
template <int N>
VRF_HD void kzgm_store_words(uint8_t* p, const uint32_t (&w)[N], bool ok) {
  uint32_t* q = reinterpret_cast<uint32_t*>(p);
#pragma unroll
  for (int j = 0; j < N; ++j) q[j] = ok ? w[j] : 0xffffffffu;
}

VRF_HD void kzgm_weight(uint32_t r[8], KzgmShape sh, const uint8_t* seed, const uint8_t* root, uint64_t index) {
  Sha512 h;
  sha512_init(h);
  constexpr char tag[] = "vrfhip-kzg-multi-rlc-v1";
  static_assert(sizeof(tag) == 24, "");
#pragma unroll
  for (int j = 0; j < 23; ++j) sha512_put_byte(h, (uint8_t)tag[j]);
  const uint32_t shape[3] = {sh.k, sh.m, sh.p};
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int j = 0; j < 4; ++j) sha512_put_byte(h, (uint8_t)(shape[a] >> (8 * j)));
  sha512_put_bytes(h, seed, 32);
  sha512_put_bytes(h, root, 32);
#pragma unroll
  for (int j = 0; j < 8; ++j) sha512_put_byte(h, (uint8_t)(index >> (8 * j)));
  sha512_final(h);
#pragma unroll
  for (int j = 0; j < 4; ++j) { r[j] = sha512_word_mem(h, j); r[4 + j] = 0; }
}

// every one of the `count` 32-byte scalars at p is < r
VRF_HD bool kzgm_all_lt_r(const uint8_t* p, uint32_t count) {
  bool ok = true;
#pragma unroll 1
  for (uint32_t j = 0; j < count; ++j) {
    uint32_t w[8];
    kzgm_load_words(w, p + (size_t)j * 32);
    ok = kzg_lt_r(w) && ok;
  }
  return ok;
}

// dec_c: n k decode statuses, dec_p: n p; s: n k scalars, t: n (m + 1), z and u: n p
VRF_HD bool kzgm_item_valid(KzgmShape sh, size_t i, const uint8_t* dec_c, const uint8_t* dec_p, const uint8_t* s, const uint8_t* t,
                            const uint8_t* z, const uint8_t* u) {
  bool ok = true;
#pragma unroll 1
  for (uint32_t j = 0; j < sh.k; ++j) ok = dec_c[i * sh.k + j] == 0 && ok;
#pragma unroll 1
  for (uint32_t j = 0; j < sh.p; ++j) ok = dec_p[i * sh.p + j] == 0 && ok;
  if (sh.k) ok = kzgm_all_lt_r(s + i * sh.k * 32, sh.k) && ok;
  ok = kzgm_all_lt_r(t + i * (sh.m + 1) * 32, sh.m + 1) && ok;
  ok = kzgm_all_lt_r(z + i * sh.p * 32, sh.p) && ok;
  ok = kzgm_all_lt_r(u + i * sh.p * 32, sh.p) && ok;
  return ok;
}

// the weight's four words as a plain residue
VRF_HD Fe<1, 1> kzgm_weight_fe(const uint32_t r4[KZGM_WEIGHT_WORDS]) {
  uint32_t r[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = j < KZGM_WEIGHT_WORDS ? r4[j] : 0u;
  Fe<1, 1> rp;
  u256_to_limbs(rp.v, r);
  return rp;
}

VRF_HD FeN kzgm_col_term(const uint32_t r4[KZGM_WEIGHT_WORDS], const uint32_t t[8], bool ok) {
  return fe_select(ok, fe_mul(kzgm_weight_fe(r4), fe_from_u256(t)), fe_zero());
}

// Own term j of item i.  pw: the decoded point; a: s_ij for a commitment (j < k), u_ij for a proof; z: z_ij (a proof's only);
// ok: the item is valid.
VRF_HD void kzgm_prep_term(const G1MsmLayout& A, const G1MsmLayout& B, KzgmShape sh, size_t i, uint32_t j, const uint32_t pw[24],
                           const uint32_t a[8], const uint32_t z[8], const uint32_t r4[KZGM_WEIGHT_WORDS], bool ok) {
  bls::G1Aff P;
  bool inf;
  const bool use = bls::g1_load(P, inf, pw) && ok && !inf;
  const Fe<1, 1> rp = kzgm_weight_fe(r4);
  const FeN am = fe_from_u256(a);
  const size_t ia = i * (sh.k + sh.p) + j;
  uint32_t w[8];
  g1_store_affine(A.pts + ia * G1_AFF_STRIDE, P);
  if (j < sh.k) {
    kzg_canon_words(w, fe_mul(rp, am));                                   // r_i s_ij
    g1_write_digits(A.digits, A.n, ia, A.windows, w, !use);
  } else {
    const size_t ib = i * sh.p + (j - sh.k);
    kzg_canon_words(w, fe_mul(rp, fe_mul(am, fe_from_u256(z))));          // r_i (u_ij z_ij)
    g1_write_digits(A.digits, A.n, ia, A.windows, w, !use);
    kzg_canon_words(w, fe_mul(rp, am));                                   // r_i u_ij
    g1_store_affine(B.pts + ib * G1_AFF_STRIDE, P);
    g1_write_digits(B.digits, B.n, ib, B.windows, w, !use);
  }
}

// total: sum_i r_i t_ij (strict, plain); bw: shared base j (j = 0: g) as 24 wire words
VRF_HD void kzgm_fold_finish(const G1MsmLayout& A, KzgmShape sh, uint32_t j, const FeN& total, const uint32_t bw[24],
                             uint8_t* flag) {
  bls::G1Aff S;
  bool inf;
  const bool ok = bls::g1_load(S, inf, bw);
  uint32_t w[8];
  kzg_canon_words(w, total);
  const size_t slot = A.n - (sh.m + 1) + j;
  g1_store_affine(A.pts + slot * G1_AFF_STRIDE, S);
  g1_write_digits(A.digits, A.n, slot, A.windows, w, !ok || inf);
  if (!ok) flag[0] = 2;
}

VRF_HD void kzgm_combine(uint32_t out[48], const uint32_t sum_a[24], const uint32_t sum_b[24], bool vk_ok) {
#pragma unroll
  for (int j = 0; j < 24; ++j) out[j] = vk_ok ? sum_a[j] : 0xffffffffu;
  kzg_neg_point(out + 24, sum_b, vk_ok);
}

// Per-item form, one item: bases_a (k + p) x 96 B = [C_i*, pi_i*], scalars_a (k + p) x 32 B = [s_i*, u_i* z_i* mod r],
// shared_a (m + 1) x 32 B = t_i*, bases_b p x 96 B = pi_i*, scalars_b p x 32 B = r - u_i*; the item's slices of every array
// are addressed here.  g1c / g1p: the decoded points, n k and n p x 96 B.
VRF_HD void kzgm_item_rows(KzgmShape sh, size_t i, bool ok, const uint8_t* g1c, const uint8_t* g1p, const uint8_t* s,
                           const uint8_t* t, const uint8_t* z, const uint8_t* u, uint8_t* bases_a, uint8_t* scalars_a,
                           uint8_t* shared_a, uint8_t* bases_b, uint8_t* scalars_b) {
  const size_t T = sh.k + sh.p;
  uint32_t pw[24], a[8], b[8], w[8];
#pragma unroll 1
  for (uint32_t j = 0; j < sh.k; ++j) {
    kzgm_load_words(pw, g1c + (i * sh.k + j) * 96);
    kzgm_load_words(a, s + (i * sh.k + j) * 32);
    kzgm_store_words(bases_a + (i * T + j) * 96, pw, ok);
    kzgm_store_words(scalars_a + (i * T + j) * 32, a, ok);
  }
#pragma unroll 1
  for (uint32_t j = 0; j < sh.p; ++j) {
    kzgm_load_words(pw, g1p + (i * sh.p + j) * 96);
    kzgm_load_words(a, u + (i * sh.p + j) * 32);
    kzgm_load_words(b, z + (i * sh.p + j) * 32);
    fe_to_u256(w, fe_mul(fe_from_u256(a), fe_from_u256(b)));             // u_ij z_ij mod r
    kzgm_store_words(bases_a + (i * T + sh.k + j) * 96, pw, ok);
    kzgm_store_words(scalars_a + (i * T + sh.k + j) * 32, w, ok);
    kzg_neg_words<8>(w, a, vrfk::Q32);                                   // r - u_ij
    kzgm_store_words(bases_b + (i * sh.p + j) * 96, pw, ok);
    kzgm_store_words(scalars_b + (i * sh.p + j) * 32, w, ok);
  }
#pragma unroll 1
  for (uint32_t j = 0; j <= sh.m; ++j) {
    kzgm_load_words(a, t + (i * (sh.m + 1) + j) * 32);
    kzgm_store_words(shared_a + (i * (sh.m + 1) + j) * 32, a, ok);
  }
}

}  // namespace vrf
