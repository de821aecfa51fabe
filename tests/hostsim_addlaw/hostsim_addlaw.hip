// tests/hostsim_addlaw -- TEST TOOLING ONLY.
// fe_mul2 (fe.cuh) on raw lazy limbs, and the two addition laws of te.cuh on projective inputs, compiled for the host for
// the base field VRF_FIELD names: the very code a lane runs.  Never linked into libvrfhip.so.
#include "../../ark_ec_vrfs_amd/csrc/fe.cuh"
#if VRF_FIELD != 3
#include "../../ark_ec_vrfs_amd/csrc/te.cuh"
#endif
#include <cstring>
using namespace vrf;

template <int L, int V> static constexpr int vbound(const Fe<L, V>&) { return V; }

// n items of four operands (4 x 9 raw limbs each, taken as they are: the caller keeps them inside the operand types'
// bounds) -> n x 9 raw limbs of a*b + c*d; returns the value bound V of the result type
template <int L1, int V1, int L2, int V2, int L3, int V3, int L4, int V4>
static int mul2_raw(size_t n, const uint32_t* in, uint32_t* out) {
  int v = 0;
  for (size_t i = 0; i < n; ++i) {
    const uint32_t* m = in + i * 4 * NL;
    const auto r = fe_mul2(fe_load<L1, V1>(m), fe_load<L2, V2>(m + NL), fe_load<L3, V3>(m + 2 * NL), fe_load<L4, V4>(m + 3 * NL));
    fe_store(out + i * NL, r);
    v = vbound(r);
  }
  return v;
}

#if VRF_FIELD != 3
static FeN in(const uint8_t* b) { uint32_t w[8]; memcpy(w, b, 32); return fe_from_u256(w); }
template <int L, int V> static void out(uint8_t* b, const Fe<L, V>& a) { uint32_t w[8]; fe_to_u256(w, a); memcpy(b, w, 32); }

template <class C>
static int add_one(int affine, int neg, int need_t, const uint8_t* pxy, const uint8_t* pz, const uint8_t* qxy, const uint8_t* qz,
                   uint8_t* oxy) {
  const FeN x1 = in(pxy), y1 = in(pxy + 32), z1 = in(pz), x2 = in(qxy), y2 = in(qxy + 32), z2 = in(qz);
  PtE p;
  p.X = fe_mul(x1, z1); p.Y = fe_mul(y1, z1); p.Z = z1; p.T = fe_mul(fe_mul(x1, y1), z1);
  PtE r;
  if (affine) {
    PtA q;
    q.x = x2; q.y = y2; q.dt = fe_mul(fe_mul(x2, y2), C::d());
    r = te_add_affine<C>(p, q, neg != 0);
    need_t = 1;
  } else {
    PtE qe;
    qe.X = fe_mul(x2, z2); qe.Y = fe_mul(y2, z2); qe.Z = z2; qe.T = fe_mul(fe_mul(x2, y2), z2);
    r = te_add_cached<C>(p, te_to_cached<C>(qe), neg != 0, need_t != 0);
  }
  if (fe_is_zero(r.Z)) return -1;
  const FeN zi = fe_inv(r.Z);
  out(oxy, fe_mul(r.X, zi)); out(oxy + 32, fe_mul(r.Y, zi));
  // T Z = X Y where T was asked for, T = 0 where it was not
  return need_t ? (fe_eq(fe_mul(r.T, r.Z), fe_mul(r.X, r.Y)) ? 1 : 0) : (fe_is_zero(r.T) ? 1 : 0);
}

#endif

extern "C" {
int ha_field_kind() { return vrfk::FIELD_KIND; }
// combo 0: E of the addition laws, and H for a = -1, +1   (1,5)(1,5) + (1,5)(2,8)
// combo 1: H for a = -5                                  (1,5)(1,5) + (1,25)(2,8): the largest V sum te.cuh forms
// combo 2: the primitive's own limit L1 L2 + L3 L4 = 6   (2,8)(2,8) + (1,25)(2,8)
int ha_mul2(int combo, size_t n, const uint32_t* in, uint32_t* out) {
  switch (combo) {
    case 0: return mul2_raw<1, 5, 1, 5, 1, 5, 2, 8>(n, in, out);
    case 1: return mul2_raw<1, 5, 1, 5, 1, 25, 2, 8>(n, in, out);
    case 2: return mul2_raw<2, 8, 2, 8, 1, 25, 2, 8>(n, in, out);
  }
  return -1;
}

#if VRF_FIELD != 3
// P = (x1, y1) scaled by z1, Q = (x2, y2) scaled by z2 (cached form) or affine; all 32-byte little-endian canonical integers.
// curve: 0 = Bandersnatch / Ed25519 / Baby-JubJub by the field, 1 = JubJub (field 0).  Writes the affine sum x || y;
// returns 1 if the T coordinate is what the call promised, 0 if not, -1 if Z came out zero.
int ha_add(int curve, int affine, int neg, int need_t, const uint8_t* pxy, const uint8_t* pz, const uint8_t* qxy, const uint8_t* qz,
           uint8_t* oxy) {
#if VRF_FIELD == 0
  if (curve == 1) return add_one<CurveJJ>(affine, neg, need_t, pxy, pz, qxy, qz, oxy);
  return add_one<CurveBS>(affine, neg, need_t, pxy, pz, qxy, qz, oxy);
#elif VRF_FIELD == 1
  return add_one<CurveED>(affine, neg, need_t, pxy, pz, qxy, qz, oxy);
#else
  return add_one<CurveBJ>(affine, neg, need_t, pxy, pz, qxy, qz, oxy);
#endif
}
#endif
}
