// tests/hostsim_g1lincomb -- TEST TOOLING ONLY.
// The per-lane functions of the BLS12-381 G1 linear combinations (g1_lincomb.cuh: lc_recode / lc_digit, lc_term,
// lc_finish), compiled for the host: the very code a lane of k_g1_lincomb runs.  What the kernel does across lanes -- the
// butterfly of g1_add over an item's group -- is here a sequential g1_add over the terms.  Never linked into libvrfhip.so.
#include "../../ark_ec_vrfs_amd/csrc/g1_lincomb.cuh"
#include <cstring>
using namespace bls;

extern "C" {
int hl_windows() { return LC_WINDOWS; }
// n scalars (32-byte little-endian) -> n x LC_WINDOWS signed digits, window 0 first
void hl_recode(size_t n, const uint8_t* scalars, int8_t* digits) {
  for (size_t i = 0; i < n; ++i) {
    uint32_t k[8], sp[9];
    memcpy(k, scalars + 32 * i, 32);
    lc_recode(sp, k);
    for (int w = 0; w < LC_WINDOWS; ++w) digits[i * LC_WINDOWS + w] = (int8_t)lc_digit(sp, w);
  }
}
// n items of t terms each: bases n x t x 96 B, scalars n x t x 32 B -> out n x 96 B, status n bytes
void hl_lincomb(size_t n, uint32_t t, const uint8_t* bases, const uint8_t* scalars, uint8_t* out, uint8_t* status) {
  for (size_t i = 0; i < n; ++i) {
    G1P sum = g1_identity();
    bool ok = true;
    for (uint32_t j = 0; j < t; ++j) {
      uint32_t w[24], k[8];
      memcpy(w, bases + (i * t + j) * 96, 96);
      memcpy(k, scalars + (i * t + j) * 32, 32);
      G1P term;
      ok = lc_term(term, w, k, true) && ok;
      sum = g1_add(sum, term);
    }
    uint32_t o[24];
    status[i] = (uint8_t)lc_finish(o, sum, ok);
    memcpy(out + 96 * i, o, 96);
  }
}
}
