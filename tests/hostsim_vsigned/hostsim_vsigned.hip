// tests/hostsim_vsigned -- TEST TOOLING ONLY.
// The V half of the Bandersnatch IETF verifier's joint-table path compiled for the host, piece by piece: the sign-aligned
// recoding (fr.cuh glv_recode_sac), the eight affine JT_VA entries (vrf_core.cuh build_joint_va_table, joint_va_normalise), the
// walk over them (joint_va_ladder), the inversion that rides on a point's inverse root (decode_by_inv_root_ride), and the
// entries as each decode form of k_verify.hip leaves them.  Never linked into libvrfhip.so.
#include "../../ark_ec_vrfs_amd/csrc/vrf_core.cuh"
#include <cstring>
#include <vector>
using namespace vrf;

namespace {
constexpr int REGION = VERIFY_TABS * WIN_TABLE_WORDS;
DevTables tables() {
  DevTables t{};
  t.sq.P = vrfk_tables::SQRT_P;
  t.sq.lut = vrfk_tables::SQRT_LUT;
  t.sq.str = SuiteStr{};
  t.sq.str.challenge_len = 32;
  return t;
}
FeN fe_of(const uint8_t* b32) {
  uint32_t w[8];
  memcpy(w, b32, 32);
  return fe_from_u256(w);
}
template <int L, int V>
void fe_out(uint8_t* b32, const Fe<L, V>& a) {
  uint32_t w[8];
  fe_to_u256(w, a);
  memcpy(b32, w, 32);
}
void entries_out(const uint32_t* reg, uint8_t* out) {
  for (int u = 0; u < JT_VA_ENTRIES; ++u) {
    const PtA e = pta_load(reg + JT_VA + u * JT_VA_STRIDE);
    fe_out(out + 96 * u, e.x); fe_out(out + 96 * u + 32, e.y); fe_out(out + 96 * u + 64, e.dt);
  }
}
}  // namespace

extern "C" {
// the recoding of four 128-bit magnitudes: sgn (16 bytes), u (3 x 16 bytes); returns fix
uint32_t hvs_recode(const uint8_t* mags64, uint8_t* sgn16, uint8_t* u48) {
  uint32_t m[4][4];
  memcpy(m, mags64, 64);
  SacV r;
  glv_recode_sac(r, m);
  memcpy(sgn16, r.sgn, 16);
  memcpy(u48, r.u, 48);
  for (int bit = 0; bit < 128; ++bit) {           // the accessors the ladder reads must say what the words say
    const int idx = ((r.u[0][bit >> 5] >> (bit & 31)) & 1) | (((r.u[1][bit >> 5] >> (bit & 31)) & 1) << 1) |
                    (((r.u[2][bit >> 5] >> (bit & 31)) & 1) << 2);
    if (sac_index(r, bit) != idx || sac_neg(r, bit) != (((r.sgn[bit >> 5] >> (bit & 31)) & 1) != 0)) return 0xffffffffu;
  }
  return r.fix ? 1u : 0u;
}

// V = s*H - c*Gamma from affine H and Gamma (x || y, canonical little-endian) and the proof's c, s (wire bytes): the table,
// its normalisation by a plain inversion, the walk.  v: x || y; entries: 8 x (x || y || d x y).
void hvs_v(const uint8_t* hxy, const uint8_t* gxy, const uint8_t* c32, const uint8_t* s32, uint8_t* v64, uint8_t* entries) {
  std::vector<uint32_t> reg(REGION);
  jt_park_xy(reg.data() + JT_HXY, fe_of(hxy), fe_of(hxy + 32));
  jt_park_xy(reg.data() + JT_GXY, fe_of(gxy), fe_of(gxy + 32));
  uint32_t c[8], s[8];
  memcpy(c, c32, 32); memcpy(s, s32, 32);
  load_cs_reduced<SuiteBS>(c, s);
  build_joint_va_table<SuiteBS>(reg.data(), c, s);
  joint_va_normalise<SuiteBS>(reg.data(), fe_inv(fe_load<1, 2>(reg.data() + JT_VPFX)));
  entries_out(reg.data(), entries);
  uint32_t uv[2 * UV_WORDS];
  verify_joint_item<SuiteBS, 1, true>(uv + UV_WORDS, tables(), reg.data(), c, s);
  const FeN zi = fe_inv(fe_load<1, 5>(uv + UV_WORDS + 2 * NL));
  fe_out(v64, fe_mul(fe_load<1, 5>(uv + UV_WORDS), zi));
  fe_out(v64 + 32, fe_mul(fe_load<1, 5>(uv + UV_WORDS + NL), zi));
}

// a compressed point decoded with 1 / P riding on its inverse root (P: canonical little-endian).  x, pinv: canonical
// little-endian.  Returns the verdict in bit 0 and, in bit 1, whether the same point decodes without the ride to the same
// verdict and the same x.
uint32_t hvs_ride(const uint8_t* enc32, const uint8_t* p32, uint8_t* x32, uint8_t* pinv32) {
  const DevTables T = tables();
  uint32_t enc[8];
  memcpy(enc, enc32, 32);
  const DecodeA a = decode_phase_a<SuiteBS>(enc);
  Fe<1, 4> x, x0;
  FeN pinv = fe_zero();
  const bool ok = decode_by_inv_root_ride<SuiteBS>(x, pinv, true, fe_of(p32), a, T.sq);
  const bool ok0 = decode_by_inv_root<SuiteBS>(x0, a, T.sq);
  fe_out(x32, x);
  fe_out(pinv32, pinv);
  const bool same = ok == ok0 && (!ok || fe_eq(x, x0));
  return (ok ? 1u : 0u) | (same ? 2u : 0u);
}

// the 8 JT_VA entries as one of the decode forms leaves them (forms as tests/hostsim_joint: 0 compressed points, 1 H's
// affine x, y parked first, then pk and Gamma, 2 H and Gamma only, 3 x || y inputs).  Returns validity.
uint32_t hvs_decode_entries(int form, const uint8_t* pk, const uint8_t* h, const uint8_t* g, const uint8_t* c,
                            const uint8_t* s, uint8_t* entries) {
  const DevTables T = tables();
  std::vector<uint32_t> reg(REGION), scr(3 * DEC_SLOT);
  uint8_t flag = 0;
  bool ok = true;
  if (form == 3) {
    uint32_t xy[3][16], enc[3][8], c2[8], s2[8];
    memcpy(xy[0], pk, 64); memcpy(xy[1], h, 64); memcpy(xy[2], g, 64);
    memcpy(c2, c, 32); memcpy(s2, s, 32);
    load_cs_reduced<SuiteBS>(c2, s2);
    ok = verify_decode_affine_item<SuiteBS, true, true>(enc, xy, reg.data(), T.sq, 7, false, c2, s2);
  } else if (form == 1) {
    uint32_t hw[8];
    memcpy(hw, h, 32);
    const DecodeA a = decode_phase_a<SuiteBS>(hw);
    Fe<1, 4> x;
    ok = decode_by_inv_root<SuiteBS>(x, a, T.sq);
    jt_park_xy(reg.data() + JT_HXY, x, a.y);
    verify_decode_multi<SuiteBS, 2, true, true, true>(1, T, 0, 1, pk, nullptr, g, reg.data(), scr.data(), &flag, 5, c, s);
    ok = ok && flag != 0;
  } else {
    if (form == 2) verify_decode_multi<SuiteBS, 2, false, true, true>(1, T, 0, 1, nullptr, h, g, reg.data(), scr.data(), &flag, 7, c, s);
    else verify_decode_multi<SuiteBS, 3, false, true, true>(1, T, 0, 1, pk, h, g, reg.data(), scr.data(), &flag, 7, c, s);
    ok = flag != 0;
  }
  entries_out(reg.data(), entries);
  return ok ? 1u : 0u;
}
}
