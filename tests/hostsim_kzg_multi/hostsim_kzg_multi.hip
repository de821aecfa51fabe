// tests/hostsim_kzg_multi -- TEST TOOLING ONLY.
// The per-lane functions of the multi-point KZG opening check (kzg_multi.cuh), compiled for the host: the very code the lanes
// of k_kzg_multi.hip run.  What the kernels do across lanes is restated here with the same shape -- per column, blocks of
// KZG_BLOCK items summed into one partial each (partials[column][block]), then per column 256 strided running sums and a
// halving tree -- with kzg_acc at every step, as on the device.
// Never linked into libvrfhip.so.  With -DHOSTSIM_KZGM_MAIN the file is a stand-alone program (the UBSan build, `make ubsan`).
#include "../../ark_ec_vrfs_amd/csrc/kzg_multi.cuh"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace vrf;

namespace {
G1MsmLayout host_layout(size_t n, uint32_t* pts, int16_t* digits, uint8_t* flags) {
  G1MsmLayout L{};
  L.n = n; L.sets = 1; L.windows = G1_W_FULL; L.groups = 1;
  L.pts = pts; L.digits = digits; L.flags = flags;
  return L;
}
}  // namespace

extern "C" {
int hm_block() { return KZG_BLOCK; }
int hm_windows() { return G1_W_FULL; }
int hm_shape_ok(uint32_t k, uint32_t m, uint32_t p) { return kzgm_shape_ok(KzgmShape{k, m, p}) ? 1 : 0; }

void hm_weight(uint32_t k, uint32_t m, uint32_t p, const uint8_t* seed, const uint8_t* root, uint64_t index, uint8_t* r32) {
  uint32_t r[8];
  kzgm_weight(r, KzgmShape{k, m, p}, seed, root, index);
  memcpy(r32, r, 32);
}

// The batched form up to the digits.  c96 [n k], p96 [n p]: decoded points with their decode statuses dec_c, dec_p; bases96:
// g, S_1 .. S_m.  a_digits [G1_W_FULL][n (k + p) + m + 1], b_digits [G1_W_FULL][n p], status [n], partials
// [m + 1][ceil(n / 128)][9] (the words as stored), flag [1] (2: a shared base is invalid).  Returns the partials per column.
size_t hm_prep_fold(size_t n, uint32_t k, uint32_t m, uint32_t p, const uint8_t* c96, const uint8_t* dec_c, const uint8_t* s,
                    const uint8_t* t, const uint8_t* p96, const uint8_t* dec_p, const uint8_t* z, const uint8_t* u,
                    const uint8_t* bases96, const uint8_t* seed, const uint8_t* root, int16_t* a_digits, int16_t* b_digits,
                    uint8_t* status, uint32_t* partials, uint8_t* flag) {
  const KzgmShape sh{k, m, p};
  const size_t T = k + p, na = n * T + m + 1, nb = n * p;
  std::vector<uint32_t> apts(na * G1_AFF_STRIDE), bpts(nb * G1_AFF_STRIDE + 1), wts(n * KZGM_WEIGHT_WORDS + 1);
  uint8_t flags[256] = {0};
  const G1MsmLayout A = host_layout(na, apts.data(), a_digits, flags), B = host_layout(nb, bpts.data(), b_digits, flags);
  const size_t n_part = kzg_partials(n);
  // k_kzgm_prep_items
  for (size_t b = 0; b < n_part; ++b) {
    std::vector<FeN> acc(m + 1, fe_zero());
    for (size_t i = b * KZG_BLOCK; i < (b + 1) * KZG_BLOCK && i < n; ++i) {
      const bool ok = kzgm_item_valid(sh, i, dec_c, dec_p, s, t, z, u);
      uint32_t r[8];
      kzgm_weight(r, sh, seed, root, (uint64_t)i);
      memcpy(&wts[i * KZGM_WEIGHT_WORDS], r, 16);
      status[i] = ok ? 0 : 2;
      for (uint32_t c = 0; c <= m; ++c) {
        uint32_t tw[8];
        kzgm_load_words(tw, t + (i * (m + 1) + c) * 32);
        acc[c] = kzg_acc(acc[c], kzgm_col_term(r, tw, ok));
      }
    }
    for (uint32_t c = 0; c <= m; ++c) fe_store(partials + (c * n_part + b) * NL, acc[c]);
  }
  // k_kzgm_prep_terms
  for (size_t lane = 0; lane < n * T; ++lane) {
    const size_t i = lane / T;
    const uint32_t j = (uint32_t)(lane - i * T);
    uint32_t pw[24], a[8], zw[8] = {0}, r4[KZGM_WEIGHT_WORDS];
    if (j < k) {
      kzgm_load_words(pw, c96 + (i * k + j) * 96);
      kzgm_load_words(a, s + (i * k + j) * 32);
    } else {
      const size_t q = i * p + (j - k);
      kzgm_load_words(pw, p96 + q * 96);
      kzgm_load_words(a, u + q * 32);
      kzgm_load_words(zw, z + q * 32);
    }
    memcpy(r4, &wts[i * KZGM_WEIGHT_WORDS], 16);
    kzgm_prep_term(A, B, sh, i, j, pw, a, zw, r4, status[i] == 0);
  }
  // k_kzgm_fold, one workgroup per column: lane t takes the partials t, t + 256, ...; then the tree
  constexpr int W = 256;
  for (uint32_t c = 0; c <= m; ++c) {
    std::vector<FeN> lane(W, fe_zero());
    for (int t2 = 0; t2 < W; ++t2)
      for (size_t j = t2; j < n_part; j += W) lane[t2] = kzg_acc(lane[t2], fe_load<1, 2>(partials + (c * n_part + j) * NL));
    for (int st = W / 2; st >= 1; st >>= 1)
      for (int t2 = 0; t2 < st; ++t2) lane[t2] = kzg_acc(lane[t2], lane[t2 + st]);
    uint32_t bw[24];
    kzgm_load_words(bw, bases96 + (size_t)c * 96);
    kzgm_fold_finish(A, sh, c, lane[0], bw, flags);
  }
  flag[0] = flags[0];
  return n_part;
}

void hm_combine(const uint8_t* sum_a, const uint8_t* sum_b, int vk_ok, uint8_t* out192) {
  uint32_t a[24], b[24], o[48];
  memcpy(a, sum_a, 96); memcpy(b, sum_b, 96);
  kzgm_combine(o, a, b, vk_ok != 0);
  memcpy(out192, o, 192);
}

// per-item form: the rows of n items; ok [n]
void hm_item_rows(size_t n, uint32_t k, uint32_t m, uint32_t p, const uint8_t* c96, const uint8_t* dec_c, const uint8_t* s,
                  const uint8_t* t, const uint8_t* p96, const uint8_t* dec_p, const uint8_t* z, const uint8_t* u, uint8_t* bases_a,
                  uint8_t* scalars_a, uint8_t* shared_a, uint8_t* bases_b, uint8_t* scalars_b, uint8_t* ok) {
  const KzgmShape sh{k, m, p};
  for (size_t i = 0; i < n; ++i) {
    const bool v = kzgm_item_valid(sh, i, dec_c, dec_p, s, t, z, u);
    kzgm_item_rows(sh, i, v, c96, p96, s, t, z, u, bases_a, scalars_a, shared_a, bases_b, scalars_b);
    ok[i] = v ? 1 : 0;
  }
}
}

#ifdef HOSTSIM_KZGM_MAIN
// Stand-alone run for the sanitizer build: 300 items of shape (5, 3, 2) over the generator, infinity and invalid decodes, edge
// and invalid scalars in each array; then the shapes (0, 0, 1) and (11, 2, 2) on a few items.
static const uint8_t GEN[96] = {
    0xbb, 0xc6, 0x22, 0xdb, 0x0a, 0xf0, 0x3a, 0xfb, 0xef, 0x1a, 0x7a, 0xf9, 0x3f, 0xe8, 0x55, 0x6c, 0x58, 0xac, 0x1b, 0x17,
    0x3f, 0x3a, 0x4e, 0xa1, 0x05, 0xb9, 0x74, 0x97, 0x4f, 0x8c, 0x68, 0xc3, 0x0f, 0xac, 0xa9, 0x4f, 0x8c, 0x63, 0x95, 0x26,
    0x94, 0xd7, 0x97, 0x31, 0xa7, 0xd3, 0xf1, 0x17, 0xe1, 0xe7, 0xc5, 0x46, 0x29, 0x23, 0xaa, 0x0c, 0xe4, 0x8a, 0x88, 0xa2,
    0x44, 0xc7, 0x3c, 0xd0, 0xed, 0xb3, 0x04, 0x2c, 0xcb, 0x18, 0xdb, 0x00, 0xf6, 0x0a, 0xd0, 0xd5, 0x95, 0xe0, 0xf5, 0xfc,
    0xe4, 0x8a, 0x1d, 0x74, 0xed, 0x30, 0x9e, 0xa0, 0xf1, 0xa0, 0xaa, 0xe3, 0x81, 0xf4, 0xb3, 0x08};

static size_t run(size_t n, uint32_t k, uint32_t m, uint32_t p, int* flag_out) {
  std::vector<uint8_t> c(96 * n * k + 4), dc(n * k + 1, 0), s(32 * n * k + 4), t(32 * n * (m + 1)), pi(96 * n * p), dp(n * p, 0),
      z(32 * n * p), u(32 * n * p), bases(96 * (m + 1)), st(n), ok(n);
  uint8_t rm1[32], rr[32];
  memcpy(rr, vrfk::Q32, 32);
  memcpy(rm1, vrfk::Q32, 32);
  rm1[0] -= 1;                                               // r - 1 (the low byte of r is 0x01)
  uint32_t x = 12345;
  auto fill = [&](std::vector<uint8_t>& a, size_t count) {
    for (size_t i = 0; i < count; ++i) {
      for (int j = 0; j < 32; ++j) { x = x * 1664525u + 1013904223u; a[32 * i + j] = (uint8_t)(x >> 24); }
      a[32 * i + 31] &= 0x3f;                                // < r
    }
  };
  fill(s, n * k); fill(t, n * (m + 1)); fill(z, n * p); fill(u, n * p);
  for (size_t i = 0; i < n * k; ++i) memcpy(&c[96 * i], GEN, 96);
  for (size_t i = 0; i < n * p; ++i) memcpy(&pi[96 * i], GEN, 96);
  for (uint32_t j = 0; j <= m; ++j) memcpy(&bases[96 * j], GEN, 96);
  for (size_t i = 0; i < n; ++i) {
    const int kind = (int)(i % 5);
    if (kind == 1 && k) memset(&c[96 * (i * k + k - 1)], 0, 96);                    // infinity
    if (kind == 2) memset(&pi[96 * (i * p)], 0, 96);
    if (kind == 3) { memset(&pi[96 * (i * p + p - 1)], 0xff, 96); dp[i * p + p - 1] = 2; }   // an invalid decode
    if (i == 7) memcpy(&z[32 * i * p], rm1, 32);
    if (i == 8) memcpy(&t[32 * i * (m + 1)], rm1, 32);
    if (i == 9) memcpy(&z[32 * i * p], rr, 32);                                     // z = r: invalid
    if (i == 10) memset(&t[32 * (i * (m + 1) + m)], 0xff, 32);                      // t = 2^256 - 1: invalid
    if (i == 11) memcpy(&u[32 * (i * p + p - 1)], rr, 32);
    if (i == 12 && k) memcpy(&s[32 * i * k], rr, 32);
    if (i == 14) { memset(&u[32 * i * p], 0, 32); memset(&t[32 * i * (m + 1)], 0, 32); }
  }
  uint8_t seed[32], root[32], flag[1];
  for (int j = 0; j < 32; ++j) { seed[j] = (uint8_t)j; root[j] = (uint8_t)(255 - j); }
  const size_t T = k + p, na = n * T + m + 1, nb = n * p;
  std::vector<int16_t> ad(G1_W_FULL * na), bd(G1_W_FULL * nb);
  std::vector<uint32_t> part((m + 1) * kzg_partials(n) * NL);
  hm_prep_fold(n, k, m, p, c.data(), dc.data(), s.data(), t.data(), pi.data(), dp.data(), z.data(), u.data(), bases.data(), seed,
               root, ad.data(), bd.data(), st.data(), part.data(), flag);
  size_t bad = 0;
  for (size_t i = 0; i < n; ++i) bad += st[i] != 0;
  std::vector<uint8_t> ba(96 * n * T), sa(32 * n * T), sh(32 * n * (m + 1)), bb(96 * nb), sb(32 * nb);
  hm_item_rows(n, k, m, p, c.data(), dc.data(), s.data(), t.data(), pi.data(), dp.data(), z.data(), u.data(), ba.data(), sa.data(),
               sh.data(), bb.data(), sb.data(), ok.data());
  for (size_t i = 0; i < n; ++i) bad += (size_t)((ok[i] != 0) != (st[i] == 0)) * 1000;
  *flag_out = flag[0];
  return bad;
}

int main() {
  int flag = 0, f2 = 0, f3 = 0;
  const size_t bad = run(300, 5, 3, 2, &flag);
  const size_t bad2 = run(20, 0, 0, 1, &f2), bad3 = run(20, 11, 2, 2, &f3);
  uint8_t out[192], inf[96] = {0};
  hm_combine(GEN, inf, 1, out);
  hm_combine(GEN, GEN, 0, out);
  std::printf("hostsim_kzg_multi: 300 items of (5, 3, 2): %zu invalid, flag %d; (0, 0, 1): %zu; (11, 2, 2): %zu\n", bad, flag, bad2,
              bad3);
  // every fifth item has an invalid decode; items 9, 10, 11 and (k > 0) 12 an invalid scalar
  return (bad == 64 && bad2 == 7 && bad3 == 8 && flag == 0 && f2 == 0 && f3 == 0) ? 0 : 1;
}
#endif
