// tests/hostsim_kzg_prove -- TEST TOOLING ONLY.
// The per-lane functions of the KZG commitment and opening (kzg_prove.cuh), compiled for the host: the very code the lanes of
// k_kzg_prove.hip run.  What the kernels do across lanes is restated here with the same shape: the cut of kzg_cut, workgroups
// of KZGQ_BLOCK lanes, the suffix scan of the lanes' maps in doubling strides over two arrays (the kernel's LDS), the first
// launch that leaves every workgroup's H, the chain of the later workgroups' H that lane 0 of the second launch runs, and the
// second pass from the lane's carry.  Never linked into libvrfhip.so.  With -DHOSTSIM_KZG_PROVE_MAIN the file is a stand-alone
// program (the UBSan build, `make ubsan`).
#include "../../ark_ec_vrfs_amd/csrc/kzg_prove.cuh"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace vrf;

namespace {
G1MsmLayout host_layout(size_t n, int sets, int16_t* digits, uint8_t* flags) {
  G1MsmLayout L{};
  L.n = n; L.sets = sets; L.windows = G1_W_FULL; L.groups = 1;
  L.digits = digits; L.flags = flags;
  return L;
}

// one workgroup of k_kzg_quotient<FINAL>
void quotient_wg(bool final, const G1MsmLayout& L, uint32_t chunk, size_t g, size_t G, size_t c, const uint8_t* coeffs,
                 const uint8_t* z, uint32_t* wg_sums, const uint32_t* base_pts, uint8_t* value) {
  constexpr int B = KZGQ_BLOCK;
  const size_t len = L.n + 1;
  std::vector<KzgMap> f(B), stage(B);
  uint32_t zw[8];
  memcpy(zw, z + c * 32, 32);
  FeN zm;
  const bool z_ok = kzg_point(zm, zw);
  std::vector<uint32_t> poly(len * 8);
  memcpy(poly.data(), coeffs + c * len * 32, len * 32);
  for (int t = 0; t < B; ++t) {
    bool ok = z_ok;
    const size_t j0 = (g * B + t) * chunk;
    f[t].h = kzg_q_lane_sum(ok, poly.data(), len, j0, chunk, zm);
    f[t].a = kzg_pow(zm, chunk);
    if (!ok) L.flags[c] = 2;
  }
  for (int s = 1; s < B; s <<= 1) {
    stage = f;
    for (int t = 0; t + s < B; ++t) f[t] = kzg_compose(stage[t], stage[t + s]);
  }
  if (!final) {
    fe_store(wg_sums + (c * G + g) * NL, f[0].h);
    return;
  }
  FeN cw = fe_zero();
  for (size_t gg = G - 1; gg > g; --gg) {
    KzgMap o;
    o.a = f[0].a;
    o.h = fe_load<1, 2>(wg_sums + (c * G + gg) * NL);
    cw = kzg_apply(o, cw);
  }
  for (int t = 0; t < B; ++t) {
    const FeN carry = t + 1 < B ? kzg_apply(f[t + 1], cw) : cw;
    kzg_q_lane_emit(L, c, base_pts, poly.data(), len, (g * B + t) * chunk, chunk, zm, carry,
                    reinterpret_cast<uint32_t*>(value + c * 32));
  }
}
}  // namespace

extern "C" {
int hp_block() { return KZGQ_BLOCK; }
int hp_chunk_max() { return KZGQ_CHUNK_MAX; }
int hp_windows() { return G1_W_FULL; }
void hp_cut(size_t len, uint32_t* chunk, uint32_t* wgs) {
  const KzgCut c = kzg_cut(len);
  *chunk = c.chunk; *wgs = c.wgs;
}

// k_kzg_commit_prep: coeffs k x len x 32 B; base_inf [len] (1: the base is the point at infinity); digits [k][W][len],
// flags [k]
void hp_commit_prep(size_t k, size_t len, const uint8_t* coeffs, const uint8_t* base_inf, int16_t* digits, uint8_t* flags) {
  memset(flags, 0, k);
  const G1MsmLayout L = host_layout(len, (int)k, digits, flags);
  for (size_t i = 0; i < k * len; ++i) {
    const size_t c = i / len, j = i - c * len;
    uint32_t w[8];
    memcpy(w, coeffs + i * 32, 32);
    if (!kzg_commit_item(L, c, j, w, base_inf[j] != 0)) L.flags[c] = 2;
  }
}

// launch_kzg_open up to the digits: coeffs k x len x 32 B, z k x 32 B; base_inf [len - 1]; digits [k][W][len - 1],
// value k x 32 B (as the quotient kernel leaves it), flags [k].  Returns the number of workgroups per polynomial.
uint32_t hp_open(size_t k, size_t len, const uint8_t* coeffs, const uint8_t* z, const uint8_t* base_inf, int16_t* digits,
                 uint8_t* value, uint8_t* flags) {
  memset(flags, 0, k);
  const G1MsmLayout L = host_layout(len - 1, (int)k, digits, flags);
  std::vector<uint32_t> pts((len - 1) * G1_AFF_STRIDE + 1, 0);
  for (size_t j = 0; j + 1 < len; ++j) pts[j * G1_AFF_STRIDE + G1_SRS_INF_WORD] = base_inf[j];
  const KzgCut cut = kzg_cut(len);
  std::vector<uint32_t> wg_sums(k * cut.wgs * NL);
  for (int pass = cut.wgs > 1 ? 0 : 1; pass < 2; ++pass)
    for (size_t c = 0; c < k; ++c)
      for (size_t g = 0; g < cut.wgs; ++g)
        quotient_wg(pass == 1, L, cut.chunk, g, cut.wgs, c, coeffs, z, wg_sums.data(), pts.data(), value);
  return cut.wgs;
}
}

#ifdef HOSTSIM_KZG_PROVE_MAIN
// Stand-alone run for the sanitizer build: three polynomials over three workgroups, edge scalars, one invalid coefficient.
int main() {
  const size_t len = 2 * KZGQ_BLOCK * KZGQ_CHUNK_MAX + 5, k = 3;
  std::vector<uint8_t> coeffs(k * len * 32), z(k * 32), inf(len, 0), value(k * 32), flags(k);
  uint32_t x = 2024;
  for (size_t i = 0; i < coeffs.size(); ++i) { x = x * 1664525u + 1013904223u; coeffs[i] = (uint8_t)(x >> 24); }
  for (size_t i = 0; i < k * len; ++i) coeffs[i * 32 + 31] &= 0x3f;          // < r
  for (size_t i = 0; i < z.size(); ++i) { x = x * 1664525u + 1013904223u; z[i] = (uint8_t)(x >> 24); }
  for (size_t c = 0; c < k; ++c) z[c * 32 + 31] &= 0x3f;
  memcpy(&z[32], vrfk::Q32, 32);
  z[32] -= 1;                                                                  // z = r - 1
  memset(&coeffs[(2 * len + 77) * 32], 0xff, 32);                              // polynomial 2: a coefficient >= r
  inf[3] = 1;
  std::vector<int16_t> qd(k * G1_W_FULL * (len - 1)), cd(k * G1_W_FULL * len);
  const uint32_t wgs = hp_open(k, len, coeffs.data(), z.data(), inf.data(), qd.data(), value.data(), flags.data());
  const int open_flags = flags[0] * 100 + flags[1] * 10 + flags[2];
  hp_commit_prep(k, len, coeffs.data(), inf.data(), cd.data(), flags.data());
  std::printf("hostsim_kzg_prove: len %zu, %u workgroups, open flags %03d, commit flags %d%d%d, v[0] %02x\n", len, wgs,
              open_flags, flags[0], flags[1], flags[2], value[0]);
  return (wgs == 3 && open_flags == 2 && flags[2] == 2 && flags[0] == 0) ? 0 : 1;
}
#endif
