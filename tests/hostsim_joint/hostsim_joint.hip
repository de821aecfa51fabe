// tests/hostsim_joint -- TEST TOOLING ONLY.
// The Bandersnatch IETF verifier's joint-table path (vrf_core.cuh: build_joint_y_table, build_joint_v_table, joint_u_ladder,
// joint_v_ladder) compiled for the host and staged as k_verify.hip stages it: the decode stage with JOINT set, load_cs_reduced,
// the two verify_joint_item halves, and the encoding of k_misc.hip's readout kernel.  Never linked into libvrfhip.so.
#include "../../ark_ec_vrfs_amd/csrc/vrf_core.cuh"
#include <cstring>
#include <vector>
using namespace vrf;

namespace {
void pack_be(uint64_t* w, const uint8_t* b, size_t n) {
  for (size_t i = 0; i < n; ++i) w[i >> 3] |= (uint64_t)b[i] << (56 - 8 * (i & 7));
}
// the built-in Bandersnatch descriptor's strings
SuiteStr bandersnatch_str() {
  static const char id[] = "Bandersnatch_SHA-512_ELL2";
  static const char dst[] = "ECVRF_Bandersnatch_XMD:SHA-512_ELL2_RO_Bandersnatch_SHA-512_ELL2";
  SuiteStr s{};
  s.challenge_len = 32;
  s.suite_id_len = sizeof id - 1;
  pack_be(s.suite_id_w, (const uint8_t*)id, sizeof id - 1);
  uint8_t dp[129];
  memcpy(dp, dst, sizeof dst - 1);
  dp[sizeof dst - 1] = (uint8_t)(sizeof dst - 1);
  s.dst_prime_len = sizeof dst;
  pack_be(s.dst_prime_w, dp, sizeof dst);
  return s;
}
// the generator's fixed-base table as a context builds it (k_init_gcomb)
struct HostTables {
  std::vector<uint32_t> g_comb;
  DevTables t;
  HostTables() {
    const FeN gx = SuiteBS::gx(), gy = SuiteBS::gy();
    g_comb.assign(GCOMB_WORDS, 0);
    std::vector<uint32_t> prefix((size_t)GC_SEG * NL);
    for (int w = 0; w < GC_ROWS; ++w)
      for (int seg = 0; seg < GC_SEGS; ++seg) gcomb_build_segment<SuiteBS>(g_comb.data(), prefix.data(), gx, gy, w, seg);
    t.sq.P = vrfk_tables::SQRT_P;
    t.sq.lut = vrfk_tables::SQRT_LUT;
    t.sq.str = bandersnatch_str();
    t.g_win = nullptr;
    t.g_comb = g_comb.data();
    t.b_comb = nullptr;
  }
};
HostTables& HT() {
  static HostTables h;
  return h;
}
constexpr int REGION = VERIFY_TABS * WIN_TABLE_WORDS;

// the item's region as one of the decode forms leaves it.  form 0: compressed points (k_verify_decode); 1: H's affine x, y
// parked first, then pk and Gamma (k_verify_input_from_alpha + k_verify_decode_skip_h); 2: H and Gamma only, as the keyed
// decode (JT_Y is left empty).  Returns validity.
bool decode(int form, DevTables T, uint32_t check_mask, const uint8_t* pk, const uint8_t* h, const uint8_t* g,
            const uint8_t* c, const uint8_t* s, uint32_t* reg) {
  std::vector<uint32_t> scr(3 * DEC_SLOT);
  uint8_t flag = 0;
  if (form == 1) {
    uint32_t hw[8];
    memcpy(hw, h, 32);
    DecodeA a = decode_phase_a<SuiteBS>(hw);
    FeN dens[1] = {a.den}, dinv[1];
    fe_batch_inv(dinv, dens);
    Fe<1, 4> x;
    const bool ok = decode_phase_b<SuiteBS>(x, a, dinv[0], T.sq);
    jt_park_xy(reg + JT_HXY, x, a.y);
    verify_decode_multi<SuiteBS, 2, true, true>(1, T, 0, 1, pk, nullptr, g, reg, scr.data(), &flag, check_mask & ~2u, c, s);
    return ok && flag != 0;
  }
  if (form == 2) verify_decode_multi<SuiteBS, 2, false, true>(1, T, 0, 1, nullptr, h, g, reg, scr.data(), &flag, check_mask, c, s);
  else verify_decode_multi<SuiteBS, 3, false, true>(1, T, 0, 1, pk, h, g, reg, scr.data(), &flag, check_mask, c, s);
  return flag != 0;
}
void affine_of(uint8_t* out64, const FeP& X, const FeP& Y, const FeP& Z) {
  const FeN zi = fe_inv(fe_mul(Z, fe_one()));
  uint32_t w[8];
  fe_to_u256(w, fe_mul(X, zi));
  memcpy(out64, w, 32);
  fe_to_u256(w, fe_mul(Y, zi));
  memcpy(out64 + 32, w, 32);
}
}  // namespace

extern "C" {
void hjt_init() { (void)HT(); }

// U = s*G - c*pk and V = s*H - c*Gamma through the joint tables.  Returns 0, or 2 with zero bytes in u and v.
uint32_t hjt_verify_uv(uint32_t challenge_len, uint32_t check_mask, const uint8_t* pk, const uint8_t* h, const uint8_t* g,
                       const uint8_t* c, const uint8_t* s, uint8_t* u, uint8_t* v) {
  DevTables T = HT().t;
  T.sq.str.challenge_len = challenge_len;
  std::vector<uint32_t> reg(REGION), uv(2 * UV_WORDS);
  bool valid = decode(0, T, check_mask, pk, h, g, c, s, reg.data());
  uint32_t c2[8], s2[8];
  memcpy(c2, c, 32); memcpy(s2, s, 32);
  const bool canon = fr_is_canonical<SuiteBS>(s2);
  load_cs_reduced<SuiteBS>(c2, s2);
  verify_joint_item<SuiteBS, 0>(uv.data(), T, reg.data(), c2, s2);
  verify_joint_item<SuiteBS, 1>(uv.data() + UV_WORDS, T, reg.data(), c2, s2);
  valid = valid && canon;
  FeP zin[2] = {fe_load<1, 5>(uv.data() + 2 * NL), fe_load<1, 5>(uv.data() + UV_WORDS + 2 * NL)};
  FeN zi[2];
  fe_batch_inv(zi, zin);
  uint32_t e[2][8];
  te_encode_affine(e[0], fe_mul(fe_load<1, 5>(uv.data()), zi[0]), fe_mul(fe_load<1, 5>(uv.data() + NL), zi[0]), T.sq.str.flags);
  te_encode_affine(e[1], fe_mul(fe_load<1, 5>(uv.data() + UV_WORDS), zi[1]), fe_mul(fe_load<1, 5>(uv.data() + UV_WORDS + NL), zi[1]),
                   T.sq.str.flags);
  if (!valid) memset(e, 0, sizeof e);
  memcpy(u, e[0], 32); memcpy(v, e[1], 32);
  return valid ? 0 : 2;
}

// The 12 JT_Y and 15 JT_V entries of one item as affine x || y (canonical, little-endian), 27 * 64 bytes, and for every
// entry whether its dT word equals d * x * y * Z (bit i of the return value is set when entry i fails that).
uint32_t hjt_tables(int form, const uint8_t* pk, const uint8_t* h, const uint8_t* g, const uint8_t* c, const uint8_t* s,
                    uint8_t* out) {
  std::vector<uint32_t> reg(REGION);
  decode(form, HT().t, 0, pk, h, g, c, s, reg.data());
  uint32_t bad = 0;
  for (int i = 0; i < JT_Y_ENTRIES + JT_V_ENTRIES; ++i) {
    const PtC e = ptc_load(reg.data() + (i < JT_Y_ENTRIES ? JT_Y + i * PTC_WORDS : JT_V + (i - JT_Y_ENTRIES) * PTC_WORDS));
    affine_of(out + 64 * i, e.X, e.Y, e.Z);
    // dT * Z = d * X * Y
    const FeN lhs = fe_mul(e.dT, e.Z), rhs = fe_mul(fe_mul(e.X, e.Y), SuiteBS::d());
    if (!fe_eq(lhs, rhs)) bad |= 1u << i;
  }
  return bad;
}

// the signed radix-4 digits of a 128-bit magnitude (64 of them, least significant first)
void hjt_digits2(const uint8_t* mag16, int8_t* out64) {
  uint32_t k[4], rec[4];
  memcpy(k, mag16, 16);
  scalar_recode_signed2_128(rec, k);
  for (int w = 0; w < 64; ++w) out64[w] = (int8_t)scalar_digit2_128(rec, w);
}
// the JT_V index of bits 126..0 of four magnitudes (out[bit])
void hjt_vbits(const uint8_t* mags64, uint8_t* out127) {
  uint32_t m[4][4];
  memcpy(m, mags64, 64);
  for (int bit = 0; bit < 127; ++bit) out127[bit] = (uint8_t)joint_v_index(m, bit);
}
// joint_y_index: the index in the low byte, the negation flag in bit 8
uint32_t hjt_y_index(int a, int b) {
  bool neg;
  const int idx = joint_y_index(a, b, neg);
  return (uint32_t)idx | (neg ? 0x100u : 0u);
}
}
