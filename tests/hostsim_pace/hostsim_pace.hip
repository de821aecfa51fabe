// tests/hostsim_pace -- TEST TOOLING ONLY.
// The evenly paced divsteps rounds of fe.cuh (jac_steps_paced under jacobi_limbs and fe_inv<false>) and the decompression
// by inverse root of vrf_core.cuh (decode_by_inv_root) compiled for the host as a stand-alone program, once per base field
// and once more with the undefined-behaviour sanitizer (tests/test_hostsim_pace.py).  Never linked into libvrfhip.so.
//
//   hostsim_pace jac < values > out     per 32-byte little-endian integer below 2^256 (canonical inputs are < 2q):
//                                       the symbol as a signed byte (2 = gave up) and the rounds it took
//   hostsim_pace inv < values > out     per value: 1 / value (mod q) as 32 bytes, 0 -> 0, and the rounds (255 = the
//                                       exponentiation fallback answered)
//   hostsim_pace dec FLAGS < encodings > out
//                                       per compressed point (y, sign flag in bit 255) of the field's Edwards curve: one
//                                       byte, 1 = accepted, and x as 32 bytes (zero when rejected).  FLAGS: SuiteStr::flags
//                                       (1 = the sign flag is x mod 2)
#include "../../ark_ec_vrfs_amd/csrc/vrf_core.cuh"
#include <cstdio>
#include <cstdlib>
#include <cstring>
using namespace vrf;

#if VRF_FIELD == 0
using SX = SuiteBS;
#elif VRF_FIELD == 1
using SX = SuiteED;
#else
using SX = SuiteBJ;
#endif

int main(int argc, char** argv) {
  const char* mode = argc >= 2 ? argv[1] : "";
  const bool jac = !strcmp(mode, "jac") && argc == 2, inv = !strcmp(mode, "inv") && argc == 2;
  const bool dec = !strcmp(mode, "dec") && argc == 3;
  if (!jac && !inv && !dec) {
    fprintf(stderr, "usage: %s jac|inv|dec FLAGS < values > results\n", argv[0]);
    return 2;
  }
  SqrtTables T{};
  T.P = vrfk_tables::SQRT_P;
  T.lut = vrfk_tables::SQRT_LUT;
  if (dec) T.str.flags = (uint32_t)strtoul(argv[2], nullptr, 0);
  uint8_t rec[32];
  while (fread(rec, 1, 32, stdin) == 32) {
    uint32_t w[8], o[8];
    memcpy(w, rec, 32);
    int rounds = 0;
    if (inv) {
      uint8_t out[33];
      const FeN r = fe_inv<false>(fe_from_u256(w), &rounds);
      fe_to_u256(o, r);
      memcpy(out, o, 32);
      out[32] = rounds < 0 ? 255 : (uint8_t)rounds;
      fwrite(out, 1, 33, stdout);
    } else if (jac) {
      uint32_t x[NL];
      u256_to_limbs(x, w);
      const int j = jacobi_limbs(x, &rounds);
      const uint8_t out[2] = {(uint8_t)(int8_t)j, (uint8_t)rounds};
      fwrite(out, 1, 2, stdout);
    } else {
      uint8_t out[33] = {0};
      const DecodeA a = decode_phase_a<SX>(w);
      Fe<1, 4> x;
      if (decode_by_inv_root<SX>(x, a, T)) {
        out[0] = 1;
        fe_to_u256(o, x);
        memcpy(out + 1, o, 32);
      }
      fwrite(out, 1, 33, stdout);
    }
  }
  return 0;
}
