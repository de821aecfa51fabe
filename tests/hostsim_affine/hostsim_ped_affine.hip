// tests/hostsim_affine -- TEST TOOLING ONLY.
// The Pedersen per-proof verifier over affine x || y inputs (pedersen_verify_decode_affine_item, vrf_core.cuh), compiled for
// the host and chained through the same Straus and finish item functions the device stages run, next to the compressed
// decode on the same points.  Never linked into libvrfhip.so.
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
// the generator and blinding-base tables a context builds (k_init_gwin / k_init_gcomb)
struct HostTables {
  std::vector<uint32_t> g_win, g_comb, b_comb;
  DevTables t;
  HostTables() {
    const FeN gx = SuiteBS::gx(), gy = SuiteBS::gy(), bx = SuiteBS::bx(), by = SuiteBS::by();
    g_win.assign(2 * WIN_TABLE_WORDS, 0);
    build_glv_tables<SuiteBS>(g_win.data(), gx, gy);
    g_comb.assign(GCOMB_WORDS, 0);
    b_comb.assign(GCOMB_WORDS, 0);
    std::vector<uint32_t> prefix((size_t)GC_SEG * NL);
    for (int which = 0; which < 2; ++which)
      for (int w = 0; w < GC_ROWS; ++w)
        for (int seg = 0; seg < GC_SEGS; ++seg)
          gcomb_build_segment<SuiteBS>(which ? b_comb.data() : g_comb.data(), prefix.data(), which ? bx : gx, which ? by : gy,
                                       w, seg);
    t.sq.P = vrfk_tables::SQRT_P;
    t.sq.lut = vrfk_tables::SQRT_LUT;
    t.sq.str = bandersnatch_str();
    t.g_win = g_win.data();
    t.g_comb = g_comb.data();
    t.b_comb = b_comb.data();
  }
};
HostTables& HT() {
  static HostTables h;
  return h;
}
uint32_t g_check_mask = 0;
// stages 2 and 3 as k_ped_verify_straus / k_ped_verify_finish run them
uint32_t straus_finish(const uint32_t c[8], const uint8_t* s_b, const uint8_t* sb_b, bool valid, const uint32_t* tabs,
                       uint32_t* pts) {
  uint32_t s[8], sb[8], s2[8], sb2[8];
  memcpy(s, s_b, 32);
  memcpy(sb, sb_b, 32);
  const bool canon = fr_is_canonical<SuiteBS>(s) && fr_is_canonical<SuiteBS>(sb);
  for (int j = 0; j < 8; ++j) { s2[j] = canon ? s[j] : 0; sb2[j] = canon ? sb[j] : 0; }
  pedersen_verify_straus_item<SuiteBS, 0>(pts, HT().t, tabs, c, s2, sb2);
  pedersen_verify_straus_item<SuiteBS, 1>(pts + UV_WORDS, HT().t, tabs, c, s2, sb2);
  return pedersen_verify_finish_item<SuiteBS>(pts, s, sb, valid);
}
}  // namespace

extern "C" {
void hpa_init() { (void)HT(); }
void hpa_set_check_mask(uint32_t m) { g_check_mask = m; }
// xy320: H | Gamma | pk_com | R | Ok, 64 bytes each (x || y little-endian; mont256: arkworks Montgomery limbs)
uint32_t hpa_pedersen_verify_affine(const uint8_t* xy320, const uint8_t* s, const uint8_t* sb, const uint8_t* ad,
                                    uint32_t ad_len, int mont256) {
  std::vector<uint32_t> tabs(VERIFY_TABS * WIN_TABLE_WORDS), pts(PROVE_PTS_WORDS);
  uint32_t c[8];
  const bool valid = pedersen_verify_decode_affine_item<SuiteBS>(c, HT().t, xy320, xy320 + 64, xy320 + 128, xy320 + 192,
                                                                 xy320 + 256, ad, ad_len, tabs.data(), pts.data(),
                                                                 g_check_mask, mont256 != 0);
  return straus_finish(c, s, sb, valid, tabs.data(), pts.data());
}
// enc160: H | Gamma | pk_com | R | Ok, 32-byte compressed encodings
uint32_t hpa_pedersen_verify(const uint8_t* enc160, const uint8_t* s, const uint8_t* sb, const uint8_t* ad, uint32_t ad_len) {
  uint32_t enc[5][8];
  for (int p = 0; p < 5; ++p) memcpy(enc[p], enc160 + 32 * p, 32);
  std::vector<uint32_t> tabs(VERIFY_TABS * WIN_TABLE_WORDS), pts(PROVE_PTS_WORDS);
  uint32_t c[8];
  const bool valid = pedersen_verify_decode_item<SuiteBS>(c, HT().t, enc, ad, ad_len, tabs.data(), pts.data(), g_check_mask);
  return straus_finish(c, s, sb, valid, tabs.data(), pts.data());
}
}
