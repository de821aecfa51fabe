// kzg_prove.cuh -- per-lane functions of the KZG prover side (k_kzg_prove.hip): `KZG10::commit` and the non-hiding
// `KZG10::open` of ark-poly-commit over a base set that stays on the device (vrfhip_g1_srs).
//
// A commitment is one multi-scalar multiplication per column over shared bases: the prep lane of (column c, index j) only
// range-tests its scalar and writes its signed digits into set c of a G1MsmLayout (column = set); the points are the resident
// Montgomery affine slots, never copied.
//
// An opening of p (len coefficients, monomial basis) at z is v = p(z) and pi = sum_j q_j srs[j] with q = (p - v) / (X - z).
// With y_j = q_{j-1} (y_0 = v, y_len = 0) the synthetic division is one recurrence,
//     y_j = p_j + z y_{j+1},
// a chain of affine maps x -> p_j + z x, so it scans.  A polynomial is cut into chunks of m consecutive coefficients, one
// chunk per lane, KZGQ_BLOCK lanes per workgroup (kzg_cut):
//   kzg_q_lane_sum   Horner over the lane's chunk from the top with incoming carry 0: H = sum_i p_{j0+i} z^i
//   kzg_pow          z^m; with H the lane's map x -> H + z^m x
//   kzg_compose      f o g of two such maps: the suffix scan over the lanes of a workgroup (k_kzg_quotient restates it through
//                    LDS, tests/hostsim_kzg_prove over arrays) gives lane t the map S_t = f_t o f_{t+1} o ...; S_0 is the
//                    workgroup's map, and the carry into workgroup g is the Horner chain of the later workgroups' H
//   kzg_apply        a map at a carry: lane t starts its second pass from S_{t+1}(carry of the workgroup)
//   kzg_q_lane_emit  second pass over the chunk: every y_j; v = y_0, and the DIGITS of q_{j-1} = y_j go straight into the
//                    layout (g1_write_digits) -- the quotient is never stored as field elements.
// Forms: z and the powers z^m are Montgomery images, coefficients, carries and H are PLAIN residues (kzg.cuh: plain x
// Montgomery gives a plain product), so a coefficient enters as its 9 limbs and a y_j leaves through one product by R and
// one conditional subtraction.  Every accumulation passes through a product and comes back to the storage form FeN, as
// kzg_acc does: the lazy-limb bounds of fe.cuh do not let an open-ended running sum compile.  All values are exact residues,
// so the digits equal those of the sequential recurrence bit for bit.
// A scalar >= r (coefficient or z) is replaced by 0 and reported; the caller zeroes the outputs of that polynomial.
// All VRF_HD: tests/hostsim_kzg_prove compiles them for the host.
#pragma once
#include "kzg.cuh"

namespace vrf {

// commit prep, one (column, index): the scalar's digits into set `set`; a base at infinity takes no part.  False: k >= r.
VRF_HD bool kzg_commit_item(const G1MsmLayout& L, size_t set, size_t j, const uint32_t k[8], bool base_inf) {
  const bool ok = kzg_lt_r(k);
  g1_write_digits(L.digits + set * (size_t)L.windows * L.n, L.n, j, L.windows, k, !ok || base_inf);
  return ok;
}

// a scalar from 8 little-endian words as a plain residue; >= r: zero and false
VRF_HD bool kzg_plain(Fe<1, 1>& p, const uint32_t w[8]) {
  const bool ok = kzg_lt_r(w);
  uint32_t k[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) k[i] = ok ? w[i] : 0u;
  u256_to_limbs(p.v, k);
  return ok;
}
// z as a Montgomery image; >= r: zero and false
VRF_HD bool kzg_point(FeN& zm, const uint32_t w[8]) {
  const bool ok = kzg_lt_r(w);
  uint32_t k[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) k[i] = ok ? w[i] : 0u;
  zm = fe_from_u256(k);
  return ok;
}

using KzgLazy = Fe<2, 3>;                         // a product plus a coefficient: what the next product takes
// one step of the recurrence, x <- p + z x
VRF_HD KzgLazy kzg_step(const FeN& zm, const KzgLazy& x, const Fe<1, 1>& p) { return fe_add(fe_mul(zm, x), p); }
VRF_HD FeN kzg_strict(const KzgLazy& x) { return fe_mul(x, fe_one()); }

struct KzgMap { FeN a, h; };                      // x -> h + a x: a Montgomery, h plain
VRF_HD KzgMap kzg_compose(const KzgMap& f, const KzgMap& g) {          // f o g
  KzgMap r;
  r.h = kzg_acc(f.h, fe_mul(f.a, g.h));
  r.a = fe_mul(f.a, g.a);
  return r;
}
VRF_HD FeN kzg_apply(const KzgMap& f, const FeN& x) { return kzg_acc(f.h, fe_mul(f.a, x)); }

VRF_HD FeN kzg_pow(const FeN& zm, uint32_t m) {
  FeN r = fe_one();
#pragma unroll 1
  for (uint32_t i = 0; i < m; ++i) r = fe_mul(r, zm);
  return r;
}

VRF_HD void kzg_load8(uint32_t w[8], const uint32_t* p) {
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i] = p[i];
}

// poly: the len coefficients of one polynomial, 8 words each; the lane's chunk is [j0, j0 + m).  Indices past the end count
// as zero coefficients: the running value is still 0 there, so they are skipped.  ok is cleared by a coefficient >= r.
VRF_HD FeN kzg_q_lane_sum(bool& ok, const uint32_t* poly, size_t len, size_t j0, uint32_t m, const FeN& zm) {
  KzgLazy x = fe_zero();
#pragma unroll 1
  for (uint32_t i = m; i-- > 0;) {
    const size_t j = j0 + i;
    if (j >= len) continue;
    uint32_t w[8];
    kzg_load8(w, poly + j * 8);
    Fe<1, 1> p;
    ok = kzg_plain(p, w) && ok;
    x = kzg_step(zm, x, p);
  }
  return kzg_strict(x);
}

// L: set `set` receives the digits of q_0 .. q_{len-2} (L.n = len - 1 points); base_pts: the resident slots of those points
// (word G1_SRS_INF_WORD of a slot != 0: the base is the point at infinity and its digits are zero); v: 8 words, written by
// the lane that owns index 0.  carry: y_{j0 + m}.
VRF_HD void kzg_q_lane_emit(const G1MsmLayout& L, size_t set, const uint32_t* base_pts, const uint32_t* poly, size_t len,
                            size_t j0, uint32_t m, const FeN& zm, const FeN& carry, uint32_t* v) {
  KzgLazy x = carry;
#pragma unroll 1
  for (uint32_t i = m; i-- > 0;) {
    const size_t j = j0 + i;
    if (j >= len) continue;                       // the carry into the tail is 0
    uint32_t w[8];
    kzg_load8(w, poly + j * 8);
    Fe<1, 1> p;
    (void)kzg_plain(p, w);
    x = kzg_step(zm, x, p);
    uint32_t y[8];
    kzg_canon_words(y, kzg_strict(x));
    if (j == 0) {
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = y[q];
    } else {
      const bool inf = base_pts[(j - 1) * G1_AFF_STRIDE + G1_SRS_INF_WORD] != 0;
      g1_write_digits(L.digits + set * (size_t)L.windows * L.n, L.n, j - 1, L.windows, y, inf);
    }
  }
}

}  // namespace vrf
