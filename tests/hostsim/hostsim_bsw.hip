// tests/hostsim -- TEST TOOLING ONLY: host build of the codec-bound functions of `suites::bandersnatch_sw` (csrc/bsw_core.cuh):
// the 33-byte decode (square root, te_sw_map, 2-descent subgroup test), the projective -> wire encode, the transcript hashes
// over 33-byte encodings and try-and-increment -- the functions k_bsw.hip composes.  Never linked into libvrfhip.so.
#include "../../ark_ec_vrfs_amd/csrc/bsw_core.cuh"
#include <cstring>
#include <vector>
using namespace vrf;
namespace {
SuiteStr make_str(const char* id, uint32_t challenge_len) {
  SuiteStr s{};
  s.challenge_len = challenge_len;
  s.suite_id_len = (uint32_t)strlen(id);
  for (uint32_t i = 0; i < s.suite_id_len; ++i) s.suite_id_w[i >> 3] |= (uint64_t)(uint8_t)id[i] << (56 - 8 * (i & 7));
  return s;
}
SqrtTables tables() {
  SqrtTables t;
  t.P = vrfk_tables::SQRT_P; t.lut = vrfk_tables::SQRT_LUT;
  t.str = make_str("Bandersnatch_SW_SHA-512_TAI", 32);
  return t;
}
FeN in(const uint8_t* b) { uint32_t w[8]; memcpy(w, b, 32); return fe_from_u256(w); }
template <int L, int V> void out(uint8_t* b, const Fe<L, V>& a) { uint32_t w[8]; fe_to_u256(w, a); memcpy(b, w, 32); }
}
#include "pedersen_c.inc"
extern "C" {
// bit 0: decodes; bit 1: the point at infinity; bit 2: in the prime-order subgroup.  te_xy / sw_xy: x || y little-endian
int hb_decode(const uint8_t* enc, uint8_t* te_xy, uint8_t* sw_xy) {
  const SqrtTables T = tables();
  FeN tx, ty, sx, sy;
  bool inf;
  const bool ok = bsw_decode<BswS>(tx, ty, sx, sy, inf, load33(enc, 0), T);
  out(te_xy, tx); out(te_xy + 32, ty); out(sw_xy, sx); out(sw_xy + 32, sy);
  const bool sub = ok && in_prime_subgroup<BswS>(tx, ty, T);
  return (ok ? 1 : 0) | (inf ? 2 : 0) | (sub ? 4 : 0);
}
// the Edwards point (x z : y z : z) -> wire
void hb_encode(const uint8_t* te_xy, const uint8_t* z_, uint8_t* enc) {
  const FeN x = in(te_xy), y = in(te_xy + 32), z = in(z_);
  PtE p;
  p.X = fe_mul(x, z); p.Y = fe_mul(y, z); p.Z = z; p.T = fe_mul(fe_mul(x, y), z);
  store33(enc, 0, bsw_encode<BswS>(p));
}
// n <= 8 points through the two-phase way in (ONE inversion for all of them, as k_bsw_verify_decode / k_bsw_rlc_decode run it):
// flags[i] as hb_decode bits 0 and 1, te_xy[i] the Edwards coordinates
void hb_decode_shared(const uint8_t* encs, int n, uint8_t* te_xy, uint8_t* flags) {
  const SqrtTables T = tables();
  uint32_t scr[8 * BSW_SLOT];
  uint32_t st[8];
  FeN run = fe_one();
  for (int p = 0; p < n; ++p) st[p] = bsw_in_a(scr + p * BSW_SLOT, run, load33(encs, p), T);
  FeN inv = fe_inv(run);
  for (int p = n - 1; p >= 0; --p) {
    FeN x, y;
    bsw_in_b(x, y, inv, scr + p * BSW_SLOT, (st[p] & BSW_A_INF) != 0);
    out(te_xy + 64 * p, x); out(te_xy + 64 * p + 32, y);
    flags[p] = (uint8_t)(((st[p] & BSW_A_OK) ? 1 : 0) | ((st[p] & BSW_A_INF) ? 2 : 0));
  }
}
// The verifier's U = s*G - c*pk and V = s*H - c*Gamma as k_bsw.hip stages them: k_bsw_verify_decode's shared-inversion way
// in with the subgroup tests of check_mask, bsw_load_cs, the Edwards suite's verify_straus_item, and the encoding of
// k_bsw_test_verify_uv_readout (bsw_frac, one inversion, bsw_encode_frac).  0, or 2 with zero bytes in u and v.
int hb_verify_uv(uint32_t challenge_len, uint32_t check_mask, const uint8_t* pk, const uint8_t* h, const uint8_t* g, const uint8_t* c,
                 const uint8_t* s, uint8_t* u, uint8_t* v) {
  static std::vector<uint32_t> g_comb;                     // the generator's fixed-base table, by the device's own builder
  if (g_comb.empty()) {
    g_comb.assign(GCOMB_WORDS, 0);
    std::vector<uint32_t> prefix((size_t)GC_SEG * NL);
    for (int w = 0; w < GC_ROWS; ++w)
      for (int seg = 0; seg < GC_SEGS; ++seg) gcomb_build_segment<BswS>(g_comb.data(), prefix.data(), BswS::gx(), BswS::gy(), w, seg);
  }
  DevTables T{};
  T.sq = tables();
  T.sq.str.challenge_len = challenge_len;
  T.g_comb = g_comb.data();
  const uint8_t* src[3] = {pk, h, g};
  std::vector<uint32_t> tabs(VERIFY_TABS * WIN_TABLE_WORDS), uv(2 * UV_WORDS);
  uint32_t scr[3 * BSW_SLOT], st[3];
  FeN run = fe_one();
  for (int p = 0; p < 3; ++p) st[p] = bsw_in_a(scr + p * BSW_SLOT, run, load33(src[p], 0), T.sq);
  FeN inv = fe_inv(run);
  bool valid = true;
  for (int p = 2; p >= 0; --p) {
    FeN x, y;
    bsw_in_b(x, y, inv, scr + p * BSW_SLOT, (st[p] & BSW_A_INF) != 0);
    valid = valid && (st[p] & BSW_A_OK) != 0;
    if ((check_mask >> p) & 1u) valid = in_prime_subgroup<BswS>(x, y, T.sq) && valid;
    build_glv_tables<BswS>(tabs.data() + p * 2 * WIN_TABLE_WORDS, x, y);
  }
  uint32_t cw[8], cr[8], sw[8];
  memcpy(cw, c, 32); memcpy(sw, s, 32);
  fr_reduce256<BswS>(cr, cw);
  const bool canon = fr_is_canonical<BswS>(sw);
  for (int j = 0; j < 8; ++j) { cr[j] = canon ? cr[j] : 0; sw[j] = canon ? sw[j] : 0; }
  verify_straus_item<BswS, 0>(uv.data(), T, tabs.data(), cr, sw);
  verify_straus_item<BswS, 1>(uv.data() + UV_WORDS, T, tabs.data(), cr, sw);
  valid = valid && canon;
  SwFrac f[2];
  FeN dens[2], di[2];
  for (int j = 0; j < 2; ++j) {
    const uint32_t* q = uv.data() + j * UV_WORDS;
    f[j] = bsw_frac<BswS>(fe_load<1, 5>(q), fe_load<1, 5>(q + NL), fe_load<1, 5>(q + 2 * NL));
    dens[j] = f[j].den;
  }
  fe_batch_inv(di, dens);
  store33(u, 0, bsw_encode_frac(f[0], di[0]), valid);
  store33(v, 0, bsw_encode_frac(f[1], di[1]), valid);
  return valid ? 0 : 2;
}
// Per-proof Pedersen verification with the challenge supplied (vrfhip_test_pedersen_verify_c) as k_bsw.hip stages it:
// bsw_ped_verify_decode's shared-inversion way in (chain order pk_com, H, Gamma, R, Ok; subgroup tests of check_mask), then
// the Edwards suite's override, ladders and finish (pedersen_c.inc).  0, 1 or 2.
int hb_pedersen_verify_c(uint32_t challenge_len, uint32_t check_mask, const uint8_t* h, const uint8_t* g, const uint8_t* pk_com,
                         const uint8_t* r, const uint8_t* ok, const uint8_t* c, const uint8_t* s, const uint8_t* sb) {
  static std::vector<uint32_t> combs[2];                   // generator, blinding base: by the device's own builder
  if (combs[0].empty()) {
    std::vector<uint32_t> prefix((size_t)GC_SEG * NL);
    for (int which = 0; which < 2; ++which) {
      combs[which].assign(GCOMB_WORDS, 0);
      for (int w = 0; w < GC_ROWS; ++w)
        for (int seg = 0; seg < GC_SEGS; ++seg)
          gcomb_build_segment<BswS>(combs[which].data(), prefix.data(), which ? BswS::bx() : BswS::gx(), which ? BswS::by() : BswS::gy(), w, seg);
    }
  }
  DevTables T{};
  T.sq = tables();
  T.sq.str.challenge_len = challenge_len;
  T.g_comb = combs[0].data(); T.b_comb = combs[1].data();
  const uint8_t* src[5] = {pk_com, h, g, r, ok};           // chain order
  const uint32_t chk[5] = {CHK_PROOF, CHK_INPUT, CHK_OUTPUT, CHK_PROOF, CHK_PROOF};
  std::vector<uint32_t> tabs(VERIFY_TABS * WIN_TABLE_WORDS), pts(PROVE_PTS_WORDS);
  uint32_t scr[5 * BSW_SLOT], st[5];
  FeN run = fe_one();
  for (int k = 0; k < 5; ++k) st[k] = bsw_in_a(scr + k * BSW_SLOT, run, load33(src[k], 0), T.sq);
  FeN inv = fe_inv(run);
  bool valid = true;
  for (int k = 4; k >= 0; --k) {
    const int p = k == 0 ? 2 : k == 1 ? 0 : k == 2 ? 1 : k;             // slot: H, Gamma, pk_com, R, Ok
    FeN x, y;
    bsw_in_b(x, y, inv, scr + k * BSW_SLOT, (st[k] & BSW_A_INF) != 0);
    valid = valid && (st[k] & BSW_A_OK) != 0;
    if (check_mask & chk[k]) valid = in_prime_subgroup<BswS>(x, y, T.sq) && valid;
    if (p < 3) {
      build_glv_tables<BswS>(tabs.data() + p * 2 * WIN_TABLE_WORDS, x, y);
    } else {
      uint32_t* dst = pts.data() + (p == 3 ? PED_R_OFF : PED_OK_OFF);
      fe_store(dst, x);
      fe_store(dst + NL, y);
    }
  }
  return (int)host_pedersen_ladders_c<BswS>(T, valid, tabs.data(), pts.data(), c, s, sb);
}
// Either prover from a given H as k_bsw.hip stages it: k_bsw_prove_prepare (its given-H branch), the Edwards suite's stage 2
// (prove_mul_item on the scalar k_prove_mul zeroes when it is not canonical, with its CT switch), k_bsw_prove_finish (bsw_frac of
// the four products, ONE fixed-shape inversion, the zeroed outputs of a refused item).  Returns the status (0, or 2).
// out: gamma 33 | c 32 | s 32 | pk (pk_com) 33 | h 33 | r 33 | ok 33 | sb 32 | blinding 32  (293 B; what a scheme lacks stays zero)
int hb_prove_cases(int pedersen, int ct, uint32_t check_mask, const uint8_t* sk_, const uint8_t* h_given, const uint8_t* ad,
                   uint32_t ad_len, uint8_t* o) {
  static std::vector<uint32_t> combs[2];                   // generator, blinding base: by the device's own builder
  if (combs[0].empty()) {
    std::vector<uint32_t> prefix((size_t)GC_SEG * NL);
    for (int which = 0; which < 2; ++which) {
      combs[which].assign(GCOMB_WORDS, 0);
      for (int w = 0; w < GC_ROWS; ++w)
        for (int seg = 0; seg < GC_SEGS; ++seg)
          gcomb_build_segment<BswS>(combs[which].data(), prefix.data(), which ? BswS::bx() : BswS::gx(), which ? BswS::by() : BswS::gy(), w, seg);
    }
  }
  DevTables T{};
  T.sq = tables();
  T.g_comb = combs[0].data(); T.b_comb = combs[1].data();
  memset(o, 0, 293);
  uint32_t sk[8], k[8], b[8] = {0}, kb[8] = {0};
  memcpy(sk, sk_, 32);
  bool valid = fr_is_canonical<BswS>(sk);
  FeN x, y;
  const Enc33 e = load33(h_given, 0);
  valid = bsw_decode<BswS>(x, y, e, T.sq) && valid;
  if (check_mask & CHK_INPUT) valid = in_prime_subgroup<BswS>(x, y, T.sq) && valid;
  const Enc33 h_enc = enc33_canonical(e);
  bsw_nonce(k, sk, h_enc);
  std::vector<uint32_t> tab(ProveLayout<BswS>::TAB_WORDS), pts(PROVE_PTS_WORDS);
  build_prove_tables<BswS>(tab.data(), x, y);
  if (pedersen) { bsw_blinding(b, sk, h_enc, ad, ad_len, T.sq.str); bsw_nonce(kb, b, h_enc); }
  for (int half = 0; half < 2; ++half) {
    uint32_t sc[8];
    memcpy(sc, half ? k : sk, 32);
    if (!fr_is_canonical<BswS>(sc)) memset(sc, 0, 32);
    const uint32_t* s2 = pedersen ? (half ? kb : b) : nullptr;
    if (ct) prove_mul_item<BswS, true>(pts.data() + half * 2 * UV_WORDS, T, tab.data(), sc, s2);
    else prove_mul_item<BswS, false>(pts.data() + half * 2 * UV_WORDS, T, tab.data(), sc, s2);
  }
  SwFrac f[4];
  FeN dens[4], inv[4];
  for (int j = 0; j < 4; ++j) {
    const uint32_t* q = pts.data() + j * UV_WORDS;
    f[j] = bsw_frac<BswS>(fe_load<1, 5>(q), fe_load<1, 5>(q + NL), fe_load<1, 5>(q + 2 * NL));
    dens[j] = f[j].den;
  }
  fe_batch_inv<true>(inv, dens);
  Enc33 en[4];
  for (int j = 0; j < 4; ++j) en[j] = bsw_encode_frac(f[j], inv[j]);
  const Enc33 cp[5] = {en[1], h_enc, en[0], en[3], en[2]};      // pk (or pk_com), H, Gamma, k*G (+ kb*B), k*H
  uint32_t c[8], cs[8], s[8], sb[8] = {0};
  bsw_challenge5(c, cp, ad, ad_len, T.sq.str);
  fr_mul<BswS>(cs, c, sk);
  fr_add<BswS>(s, cs, k);
  if (pedersen) { uint32_t cb[8]; fr_mul<BswS>(cb, c, b); fr_add<BswS>(sb, cb, kb); }
  if (!valid) { memset(c, 0, 32); memset(s, 0, 32); memset(sb, 0, 32); memset(b, 0, 32); }
  store33(o, 0, en[0], valid); store33(o + 97, 0, en[1], valid); store33(o + 130, 0, h_enc);
  if (pedersen) { store33(o + 163, 0, en[3], valid); store33(o + 196, 0, en[2], valid); memcpy(o + 229, sb, 32); memcpy(o + 261, b, 32); }
  else memcpy(o + 33, c, 32);
  memcpy(o + 65, s, 32);
  return valid ? 0 : 2;
}
void hb_canonical(const uint8_t* enc, uint8_t* o) { store33(o, 0, enc33_canonical(load33(enc, 0))); }
void hb_challenge(const uint8_t* pts, const uint8_t* ad, uint32_t ad_len, uint8_t* c) {
  Enc33 e[5];
  for (int i = 0; i < 5; ++i) e[i] = load33(pts, i);
  uint32_t w[8];
  bsw_challenge5(w, e, ad, ad_len, tables().str);
  memcpy(c, w, 32);
}
void hb_nonce(const uint8_t* sk, const uint8_t* h, uint8_t* k) {
  uint32_t s[8], w[8];
  memcpy(s, sk, 32);
  bsw_nonce(w, s, load33(h, 0));
  memcpy(k, w, 32);
}
void hb_blinding(const uint8_t* sk, const uint8_t* h, const uint8_t* ad, uint32_t ad_len, uint8_t* b) {
  uint32_t s[8], w[8];
  memcpy(s, sk, 32);
  bsw_blinding(w, s, load33(h, 0), ad, ad_len, tables().str);
  memcpy(b, w, 32);
}
void hb_output_hash(const uint8_t* g, uint8_t* o) {
  uint32_t w[16];
  bsw_output_hash(w, enc33_canonical(load33(g, 0)), tables().str);
  memcpy(o, w, 64);
}
// hash-to-curve; start = first counter tried.  ctr_hint (nullable) receives the first counter whose candidate passes the
// two halves of k_tai_find's test (the hint the kernels start from), 256 if none
void hb_hash_to_curve(const uint8_t* msg, uint32_t len, uint32_t start, uint8_t* enc, uint32_t* ctr_hint) {
  const SqrtTables T = tables();
  store33(enc, 0, bsw_encode<BswS>(bsw_hash_to_curve_tai(msg, len, T, start)));
  if (ctr_hint) {
    *ctr_hint = 256;
    for (uint32_t c = 0; c < 256; ++c) {
      FeN w;
      if (tai_attempt_candidate<SuiteBW>(w, msg, len, c, T) && fe_is_square_or_zero(w, T)) { *ctr_hint = c; break; }
    }
  }
}
}
