// tests/hostsim_g1codec -- TEST TOOLING ONLY.
// The item functions of the BLS12-381 G1 codec (g1_codec.cuh: fp_sqrt, g1_decode_item, g1_validate_item, g1_encode_item),
// compiled for the host: the very code the kernels of k_g1_codec.hip run, one call per point.  Never linked into
// libvrfhip.so.
#include "../../ark_ec_vrfs_amd/csrc/g1_codec.cuh"
#include <cstring>
using namespace bls;

extern "C" {
// a: 48-byte little-endian integer < p.  Returns 1 and the root (48-byte little-endian canonical) if a is a square, else
// 0 and the candidate a^((p+1)/4); -1 if a >= p.
int hg_fp_sqrt(const uint8_t a[48], uint8_t root[48]) {
  uint32_t w[12], r[12];
  memcpy(w, a, 48);
  FpS x, y;
  if (!fp_from_words(x, w)) return -1;
  const bool ok = fp_sqrt(&y, &x);
  fp_to_words(r, y);
  memcpy(root, r, 48);
  return ok ? 1 : 0;
}
// n items: in n x 48 B, out n x 96 B, status n bytes
void hg_decode(size_t n, const uint8_t* in, int check_subgroup, uint8_t* out, uint8_t* status) {
  for (size_t i = 0; i < n; ++i) {
    uint32_t w[12], o[24];
    memcpy(w, in + 48 * i, 48);
    status[i] = (uint8_t)(check_subgroup ? g1_decode_item<true>(o, w) : g1_decode_item<false>(o, w));
    memcpy(out + 96 * i, o, 96);
  }
}
void hg_validate(size_t n, const uint8_t* in, uint8_t* status) {
  for (size_t i = 0; i < n; ++i) {
    uint32_t w[24];
    memcpy(w, in + 96 * i, 96);
    status[i] = (uint8_t)g1_validate_item(w);
  }
}
void hg_encode(size_t n, const uint8_t* in, uint8_t* out, uint8_t* status) {
  for (size_t i = 0; i < n; ++i) {
    uint32_t w[24], o[12];
    memcpy(w, in + 96 * i, 96);
    status[i] = (uint8_t)g1_encode_item(o, w);
    memcpy(out + 48 * i, o, 48);
  }
}
}
