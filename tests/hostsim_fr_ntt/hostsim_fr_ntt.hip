// tests/hostsim_fr_ntt -- TEST TOOLING ONLY.
// The per-lane functions of the radix-2 transforms (fr_ntt.cuh), compiled for the host: the very code the lanes of
// k_fr_ntt.hip run.  What the kernels do across lanes is restated here with the same shape: the plan of ntt_plan, one tile
// of NTT_TILE_WORDS words per (column, tile index) in the place of LDS, the load phase of every lane, the b stages with all
// lanes of a stage before the next (the kernel's barrier), the store phase, the status byte the first pass sets and the last
// pass reads, and the scratch column between passes.  Never linked into libvrfhip.so.  -DFR_NTT_T / -DFR_NTT_LOGC build the
// same code for a smaller tile, so that plans of two and three passes occur at sizes a Python reference does in a moment.
// With -DHOSTSIM_FR_NTT_MAIN the file is a stand-alone program (the sanitizer build, `make asan`).
#include "../../ark_ec_vrfs_amd/csrc/fr_ntt.cuh"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace vrf;

namespace {
// one workgroup of k_fr_ntt_pass
void pass_wg(const NttDomain& D, const NttPass& P, uint32_t tix, const uint32_t* s, uint32_t* d, uint8_t* status1) {
  std::vector<uint32_t> tile(NTT_TILE_WORDS, 0xdeadbeefu);
  const uint32_t elems = ntt_tile_elems(P);
  bool bad = false;
  for (uint32_t t = 0; t < elems; ++t) bad = !ntt_load_lane(tile.data(), D, P, tix, t, s) || bad;
  const bool refused = P.first ? bad : status1[0] != 0;
  if (P.first && refused) status1[0] = 2;
  for (uint32_t st = 0; st < P.b; ++st)
    for (uint32_t t = 0; t < elems / 2; ++t) ntt_bfly_lane(tile.data(), D, P, st, t);
  for (uint32_t t = 0; t < elems; ++t) ntt_store_lane(tile.data(), D, P, tix, t, d, P.last && refused);
}
}  // namespace

extern "C" {
int hn_t() { return NTT_T; }
int hn_logc() { return NTT_LOGC; }
int hn_max_log() { return NTT_MAX_LOG; }
int hn_block() { return NTT_BLOCK; }
int hn_tile_words() { return (int)NTT_TILE_WORDS; }
int hn_plan(int log_n, int* bits) {
  const NttPlan p = ntt_plan(log_n);
  for (int i = 0; i < p.passes; ++i) bits[i] = p.bits[i];
  return p.passes;
}

// k_fr_domain_consts + k_fr_domain_fill: w, off, offi n x 9 words (off = offi = NULL with offset32 = NULL), consts 27 words.
// Returns 1, or 0 for an offset that is zero or >= r.
int hn_domain(uint32_t log_n, const uint8_t* offset32, uint32_t* w, uint32_t* off, uint32_t* offi, uint32_t* consts) {
  uint32_t ow[8];
  if (offset32) memcpy(ow, offset32, 32);
  if (!ntt_domain_consts(consts, log_n, offset32 ? ow : nullptr)) return 0;
  for (size_t i = 0; i < ((size_t)1 << log_n); ++i) ntt_domain_entry(w, off, offi, consts, log_n, (uint32_t)i);
  return 1;
}

// launch_fr_ntt: in, out k x n x 32 B (may be the same array); status [k]
void hn_ntt(uint32_t log_n, size_t k, int inverse, const uint32_t* w, const uint32_t* off, const uint32_t* offi,
            const uint32_t* consts, const uint8_t* in, uint8_t* out, uint8_t* status) {
  NttDomain D{};
  D.log_n = log_n; D.w = w; D.off = off; D.offi = offi; D.ninv = consts;
  const NttPlan pl = ntt_plan((int)log_n);
  const size_t n = (size_t)1 << log_n;
  std::vector<uint32_t> scratch(pl.passes > 1 ? k * n * 8 : 0), src(k * n * 8);
  memcpy(src.data(), in, k * n * 32);              // the caller's arrays need no alignment here
  std::vector<uint32_t> dst(k * n * 8, 0xeeeeeeeeu);
  memset(status, 0, k);
  for (int p = 0; p < pl.passes; ++p) {
    const NttPass P = ntt_pass(pl, p, inverse != 0);
    const uint32_t tiles = ntt_tiles(P);
    for (size_t c = 0; c < k; ++c)
      for (uint32_t tix = 0; tix < tiles; ++tix)
        pass_wg(D, P, tix, (P.first ? src.data() : scratch.data()) + c * n * 8,
                (P.last ? dst.data() : scratch.data()) + c * n * 8, status + c);
  }
  memcpy(out, dst.data(), k * n * 32);
}

// the butterflies' arithmetic alone: a, b 9 exact limbs (< 2q) -> (a + b) mod 2q, (a - b) mod 2q
void hn_addsub(const uint32_t* a, const uint32_t* b, uint32_t* sum, uint32_t* dif) {
  const FeN x = fe_load<1, 2>(a), y = fe_load<1, 2>(b);
  fe_store(sum, ntt_add(x, y));
  fe_store(dif, ntt_sub(x, y));
}
}

#ifdef HOSTSIM_FR_NTT_MAIN
// Stand-alone run for the sanitizer build: the smallest size of every pass count, plain and coset, forward then inverse;
// exact-size heap arrays, so an index past a column, a table or the tile is reported.
int main() {
  int fails = 0;
  const int sizes[] = {0, 1, NTT_T, NTT_T + 1, 2 * NTT_PASS_BITS + 1 <= NTT_MAX_LOG ? 2 * NTT_PASS_BITS + 1 : NTT_MAX_LOG};
  for (int log_n : sizes) {
    const size_t n = (size_t)1 << log_n, k = 2;
    std::vector<uint32_t> w(n * NL), off(n * NL), offi(n * NL), consts(3 * NL);
    uint8_t offset[32] = {7};
    if (!hn_domain((uint32_t)log_n, offset, w.data(), off.data(), offi.data(), consts.data())) ++fails;
    std::vector<uint8_t> in(k * n * 32), mid(k * n * 32), back(k * n * 32), st(k);
    uint32_t x = 77 + (uint32_t)log_n;
    for (size_t i = 0; i < in.size(); ++i) { x = x * 1664525u + 1013904223u; in[i] = (uint8_t)(x >> 24); }
    for (size_t i = 0; i < k * n; ++i) in[i * 32 + 31] &= 0x3f;               // < r
    for (int coset = 0; coset < 2; ++coset) {
      const uint32_t *o = coset ? off.data() : nullptr, *oi = coset ? offi.data() : nullptr;
      hn_ntt((uint32_t)log_n, k, 0, w.data(), o, oi, consts.data(), in.data(), mid.data(), st.data());
      hn_ntt((uint32_t)log_n, k, 1, w.data(), o, oi, consts.data(), mid.data(), mid.data(), st.data());
      if (memcmp(in.data(), mid.data(), in.size()) != 0 || st[0] || st[1]) ++fails;
    }
    std::printf("hostsim_fr_ntt: log_n %d, %d passes, fails %d\n", log_n, ntt_plan(log_n).passes, fails);
  }
  return fails ? 1 : 0;
}
#endif
