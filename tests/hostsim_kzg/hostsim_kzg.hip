// tests/hostsim_kzg -- TEST TOOLING ONLY.
// The per-lane functions of the KZG opening check (kzg.cuh), compiled for the host: the very code the lanes of k_kzg.hip run.
// What the kernels do across lanes is restated here with the same shape -- blocks of KZG_BLOCK items summed into one partial
// each, then 256 strided running sums and a halving tree over the partials -- with kzg_acc at every step, as on the device.
// Never linked into libvrfhip.so.  With -DHOSTSIM_KZG_MAIN the file is a stand-alone program (the UBSan build, `make ubsan`).
#include "../../ark_ec_vrfs_amd/csrc/kzg.cuh"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace vrf;

namespace {
// a layout over host memory: only the fields the prep functions touch
G1MsmLayout host_layout(size_t n, int sets, int windows, uint32_t* pts, int16_t* digits, uint8_t* flags) {
  G1MsmLayout L{};
  L.n = n; L.sets = sets; L.windows = windows; L.groups = 1;
  L.pts = pts; L.digits = digits; L.flags = flags;
  return L;
}
}  // namespace

extern "C" {
int hk_block() { return KZG_BLOCK; }
int hk_windows_short() { return G1_W_SHORT; }
int hk_windows_full() { return G1_W_FULL; }

void hk_weight(const uint8_t* seed, const uint8_t* root, uint64_t index, uint8_t* r32) {
  uint32_t r[8];
  kzg_weight(r, seed, root, index);
  memcpy(r32, r, 32);
}

// The batched form up to the digits.  c96 / p96: n decoded points; g96: the key's g.
//   short_digits [2][G1_W_SHORT][n], full_digits [G1_W_FULL][n + 1], status [n], partials [ceil(n / 128)][9] (the words as
//   stored), flag [1] (2: g invalid).  Returns the number of partials.
size_t hk_prep_fold(size_t n, const uint8_t* c96, const uint8_t* p96, const uint8_t* z, const uint8_t* v, const uint8_t* g96,
                    const uint8_t* seed, const uint8_t* root, int16_t* short_digits, int16_t* full_digits, uint8_t* status,
                    uint32_t* partials, uint8_t* flag) {
  std::vector<uint32_t> spts(2 * n * G1_AFF_STRIDE), fpts((n + 1) * G1_AFF_STRIDE);
  uint8_t flags[256] = {0};
  const G1MsmLayout S = host_layout(n, 2, G1_W_SHORT, spts.data(), short_digits, flags);
  const G1MsmLayout F = host_layout(n + 1, 1, G1_W_FULL, fpts.data(), full_digits, flags);
  const size_t n_part = kzg_partials(n);
  for (size_t b = 0; b < n_part; ++b) {
    FeN acc = fe_zero();
    for (size_t i = b * KZG_BLOCK; i < (b + 1) * KZG_BLOCK && i < n; ++i) {
      uint32_t cw[24], pw[24], zw[8], vw[8];
      memcpy(cw, c96 + 96 * i, 96); memcpy(pw, p96 + 96 * i, 96);
      memcpy(zw, z + 32 * i, 32); memcpy(vw, v + 32 * i, 32);
      acc = kzg_acc(acc, kzg_prep_item(S, F, i, cw, pw, zw, vw, seed, root, status));
    }
    fe_store(partials + b * NL, acc);
  }
  // k_kzg_fold: lane t takes the partials t, t + 256, ...; then the tree
  constexpr int T = 256;
  std::vector<FeN> lane(T, fe_zero());
  for (int t = 0; t < T; ++t)
    for (size_t j = t; j < n_part; j += T) lane[t] = kzg_acc(lane[t], fe_load<1, 2>(partials + j * NL));
  for (int s = T / 2; s >= 1; s >>= 1)
    for (int t = 0; t < s; ++t) lane[t] = kzg_acc(lane[t], lane[t + s]);
  uint32_t gw[24];
  memcpy(gw, g96, 96);
  kzg_fold_finish(F, lane[0], gw, flags);
  flag[0] = flags[0];
  return n_part;
}

void hk_combine(const uint8_t* short_a, const uint8_t* full_a, const uint8_t* short_b, int vk_ok, uint8_t* out192) {
  uint32_t a[24], f[24], b[24], o[48];
  memcpy(a, short_a, 96); memcpy(f, full_a, 96); memcpy(b, short_b, 96);
  kzg_combine(o, a, f, b, vk_ok != 0);
  memcpy(out192, o, 192);
}

// per-item form: rows of n items; dec_ok [n]
void hk_item_rows(size_t n, const uint8_t* c96, const uint8_t* p96, const uint8_t* dec_ok, const uint8_t* z, const uint8_t* v,
                  uint8_t* bases, uint8_t* scalars, uint8_t* shared, uint8_t* neg_pi, uint8_t* ok) {
  for (size_t i = 0; i < n; ++i) {
    uint32_t cw[24], pw[24], zw[8], vw[8], b[48], s[16], sh[8], np[24];
    memcpy(cw, c96 + 96 * i, 96); memcpy(pw, p96 + 96 * i, 96);
    memcpy(zw, z + 32 * i, 32); memcpy(vw, v + 32 * i, 32);
    ok[i] = kzg_item_rows(b, s, sh, np, cw, pw, dec_ok[i] != 0, zw, vw) ? 1 : 0;
    memcpy(bases + 192 * i, b, 192); memcpy(scalars + 64 * i, s, 64); memcpy(shared + 32 * i, sh, 32);
    memcpy(neg_pi + 96 * i, np, 96);
  }
}
}

#ifdef HOSTSIM_KZG_MAIN
// Stand-alone run for the sanitizer build: 300 items over the generator, infinity and invalid encodings, edge scalars.
int main() {
  static const uint8_t GEN[96] = {
      0xbb, 0xc6, 0x22, 0xdb, 0x0a, 0xf0, 0x3a, 0xfb, 0xef, 0x1a, 0x7a, 0xf9, 0x3f, 0xe8, 0x55, 0x6c, 0x58, 0xac, 0x1b, 0x17,
      0x3f, 0x3a, 0x4e, 0xa1, 0x05, 0xb9, 0x74, 0x97, 0x4f, 0x8c, 0x68, 0xc3, 0x0f, 0xac, 0xa9, 0x4f, 0x8c, 0x63, 0x95, 0x26,
      0x94, 0xd7, 0x97, 0x31, 0xa7, 0xd3, 0xf1, 0x17, 0xe1, 0xe7, 0xc5, 0x46, 0x29, 0x23, 0xaa, 0x0c, 0xe4, 0x8a, 0x88, 0xa2,
      0x44, 0xc7, 0x3c, 0xd0, 0xed, 0xb3, 0x04, 0x2c, 0xcb, 0x18, 0xdb, 0x00, 0xf6, 0x0a, 0xd0, 0xd5, 0x95, 0xe0, 0xf5, 0xfc,
      0xe4, 0x8a, 0x1d, 0x74, 0xed, 0x30, 0x9e, 0xa0, 0xf1, 0xa0, 0xaa, 0xe3, 0x81, 0xf4, 0xb3, 0x08};
  const size_t n = 300;
  std::vector<uint8_t> c(96 * n), p(96 * n), z(32 * n), v(32 * n), st(n), ok(n), dec(n);
  uint8_t rm1[32], rr[32];
  memcpy(rr, vrfk::Q32, 32);
  memcpy(rm1, vrfk::Q32, 32);
  rm1[0] -= 1;                                               // r - 1 (the low byte of r is 0x01)
  uint32_t x = 12345;
  for (size_t i = 0; i < n; ++i) {
    const int kind = (int)(i % 5);
    memcpy(&c[96 * i], GEN, 96);
    memcpy(&p[96 * i], GEN, 96);
    if (kind == 1) memset(&c[96 * i], 0, 96);               // infinity
    if (kind == 2) memset(&p[96 * i], 0, 96);
    if (kind == 3) memset(&p[96 * i], 0xff, 96);            // an invalid decode
    for (int j = 0; j < 32; ++j) {
      x = x * 1664525u + 1013904223u;
      z[32 * i + j] = (uint8_t)(x >> 24);
      x = x * 1664525u + 1013904223u;
      v[32 * i + j] = (uint8_t)(x >> 24);
    }
    z[32 * i + 31] &= 0x3f; v[32 * i + 31] &= 0x3f;         // < r
    if (i == 7) memcpy(&z[32 * i], rm1, 32);
    if (i == 8) memcpy(&v[32 * i], rm1, 32);
    if (i == 9) memcpy(&z[32 * i], rr, 32);                 // z = r: invalid
    if (i == 10) memset(&v[32 * i], 0xff, 32);              // v = 2^256 - 1: invalid
    if (i == 11) { memset(&z[32 * i], 0, 32); memset(&v[32 * i], 0, 32); }
    dec[i] = kind != 3;
  }
  uint8_t seed[32], root[32], flag[1];
  for (int j = 0; j < 32; ++j) { seed[j] = (uint8_t)j; root[j] = (uint8_t)(255 - j); }
  std::vector<int16_t> sd(2 * G1_W_SHORT * n), fd(G1_W_FULL * (n + 1));
  std::vector<uint32_t> part(kzg_partials(n) * NL);
  hk_prep_fold(n, c.data(), p.data(), z.data(), v.data(), GEN, seed, root, sd.data(), fd.data(), st.data(), part.data(), flag);
  size_t bad = 0;
  for (size_t i = 0; i < n; ++i) bad += st[i] != 0;
  uint8_t out[192], inf[96] = {0};
  hk_combine(GEN, inf, GEN, 1, out);
  hk_combine(GEN, GEN, inf, 0, out);
  std::vector<uint8_t> b(192 * n), s(64 * n), sh(32 * n), np(96 * n);
  hk_item_rows(n, c.data(), p.data(), dec.data(), z.data(), v.data(), b.data(), s.data(), sh.data(), np.data(), ok.data());
  std::printf("hostsim_kzg: %zu items, %zu invalid, flag %d, top digit of g %d\n", n, bad, (int)flag[0],
              (int)fd[(size_t)(G1_W_FULL - 1) * (n + 1) + n]);
  return (bad == 62 && flag[0] == 0) ? 0 : 1;
}
#endif
