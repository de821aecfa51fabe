// fr_ntt.cuh -- per-lane functions of the radix-2 transforms over Fr of BLS12-381 (k_fr_ntt.hip): `fft` / `ifft` /
// `coset_fft` / `coset_ifft` of ark-poly's Radix2EvaluationDomain, natural order on both sides.
//
// The plan.  A column of n = 2^log_n scalars is transformed in P passes; pass p does b_p bits of the index inside one
// workgroup, on a tile of 2^NTT_T elements at most that lies in LDS.  log_n <= NTT_T is ONE pass over the whole column.
// Above, the index is cut as in the four-step algorithm, j = (j_1, j_2, .., j_P) with j_1 the most significant digit:
//   pass p < P   view the column as [H][n_p][M], H = n_1 .. n_{p-1} done, M = n_{p+1} .. n_P to come.  A tile is one h and
//                NTT_C consecutive m: n_p rows of NTT_C contiguous scalars.  It transforms over j_p (DFT of size n_p), then
//                multiplies entry (i, m) by the inter-pass twiddle w^(H m i), and writes back to the places it read.
//   pass P       view [H][n_P]: a row is contiguous.  A tile is NTT_C rows whose first digit i_1 is consecutive, the other
//                digits equal; the result of row (i_1, i_2) for frequency i goes to i_1 + n_1 i_2 + H i: runs of NTT_C
//                contiguous scalars.  This transposing pass is the bit (digit) reversal; no permutation kernel runs.
// Inside a tile the DFT over the b bits of j is decimation in frequency (sum, then difference times twiddle) and leaves
// frequency i at position rev_b(i); the store phase reads it from there.
//
// Forms and the bound contract.  Data are PLAIN residues, twiddles MONTGOMERY images (table w[i] = w^i R, canonical), so
// a product twiddle x datum is plain (kzg.cuh) and nothing is converted on the way in or out.  Every value in a tile and
// between passes is an FeN with EXACT limbs (each < 2^29 but the top one) and value < 2q:
//   - a scalar enters through kzg_plain (< q) and u256_to_limbs, exact by construction;
//   - fe_mul leaves exact limbs and, for operands < 2q, a value < q (1 + 4 * 0.0142) < 2q;
//   - ntt_add / ntt_sub take two such values and return (a + b) mod 2q / (a - b) mod 2q: one exact carry pass and ONE
//     conditional subtraction (addition) of 2q, ~60 32-bit operations, against the three products kzg_acc would cost.
//     a + b < 4q and a - b > -2q, so one correction suffices, and 4q < 2^257 keeps the top limb far below 2^29.
// The lazy types of fe.cuh cannot express this (a sum is Fe<2, 4>, and an element that is never the multiplied operand
// would grow by 2q a stage), hence the two functions below work on limbs and re-enter the type system as FeN.
// A value < 2q < 2^256 is written between passes as its 8 words; the last pass reduces once more to [0, q).
//
// Scalings are folded into phases that multiply anyway or touch the element once: a coset's offset^j multiplies the scalar
// as the first pass loads it; the inverse's n^-1 (coset: n^-1 offset^-i) multiplies as the last pass stores.  No sweep.
// The inverse uses the same table: w^-k = w^(n - k).
//
// LDS: element e lies at word NL * (e + (e >> 5) + (e >> 10)).  The odd stride NL maps consecutive elements to distinct
// banks; the two padding terms do the same for lanes a power of two elements apart (the row-major fill of the transposing
// pass, the bit-reversed reads of the store phase), which would otherwise put a wave on one or two banks.
// All VRF_HD: tests/hostsim_fr_ntt compiles them for the host and restates the kernel's loops over arrays.
#pragma once
#include "kzg_prove.cuh"

namespace vrf {

#ifndef FR_NTT_T
#define FR_NTT_T 11          // 2^11 elements: 74 KiB of LDS, two workgroups per CU
#endif
#ifndef FR_NTT_LOGC
#define FR_NTT_LOGC 3        // rows of 8 scalars = 256 B in the passes of a multi-pass plan
#endif
constexpr int NTT_T = FR_NTT_T;
constexpr int NTT_LOGC = FR_NTT_LOGC;
constexpr int NTT_C = 1 << NTT_LOGC;
constexpr int NTT_PASS_BITS = NTT_T - NTT_LOGC;           // bits per pass of a multi-pass plan
constexpr int NTT_MAX_PASSES = 3;
constexpr int NTT_MAX_LOG = NTT_MAX_PASSES * NTT_PASS_BITS < 20 ? NTT_MAX_PASSES * NTT_PASS_BITS : 20;
constexpr int NTT_BLOCK = (1 << NTT_T) / 4 < 64 ? 64 : (1 << NTT_T) / 4;      // lanes per workgroup (512)
constexpr uint32_t NTT_TILE_WORDS = (uint32_t)NL * ((1u << NTT_T) + (1u << NTT_T >> 5) + (1u << NTT_T >> 10) + 1);
static_assert(NTT_LOGC >= 1 && NTT_PASS_BITS >= NTT_LOGC, "a pass must hold the rows of the transposing pass");

struct NttPlan { int log_n, passes, bits[NTT_MAX_PASSES]; };
VRF_HD NttPlan ntt_plan(int log_n) {
  NttPlan p{};
  p.log_n = log_n;
  if (log_n <= NTT_T) { p.passes = 1; p.bits[0] = log_n; return p; }
  p.passes = (log_n + NTT_PASS_BITS - 1) / NTT_PASS_BITS;
  for (int i = 0; i < p.passes; ++i) p.bits[i] = log_n / p.passes + (i < log_n % p.passes ? 1 : 0);
  return p;
}

// what the kernels read of a domain handle
struct NttDomain {
  uint32_t log_n;
  const uint32_t* w;        // [n][NL]  w^i
  const uint32_t* off;      // [n][NL]  offset^j          (nullptr: the plain domain)
  const uint32_t* offi;     // [n][NL]  n^-1 offset^-i    (nullptr: the plain domain)
  const uint32_t* ninv;     // [NL]     n^-1
};
// one pass of a plan
struct NttPass {
  uint32_t log_n, b, logc;  // the pass transforms b bits on rows of 2^logc scalars (single pass: logc = 0)
  uint32_t log_h;           // bits of the passes before it
  uint32_t log_n1;          // bits of the first pass
  uint32_t first, last, inverse;
};
VRF_HD NttPass ntt_pass(const NttPlan& pl, int p, bool inverse) {
  NttPass P{};
  P.log_n = (uint32_t)pl.log_n;
  P.b = (uint32_t)pl.bits[p];
  P.logc = pl.passes > 1 ? NTT_LOGC : 0;
  for (int i = 0; i < p; ++i) P.log_h += (uint32_t)pl.bits[i];
  P.log_n1 = pl.passes > 1 ? (uint32_t)pl.bits[0] : 0;
  P.first = p == 0;
  P.last = p == pl.passes - 1;
  P.inverse = inverse;
  return P;
}
VRF_HD uint32_t ntt_tile_elems(const NttPass& P) { return 1u << (P.b + P.logc); }
VRF_HD uint32_t ntt_tiles(const NttPass& P) { return 1u << ((P.last ? P.log_h : P.log_n - P.b) - P.logc); }

VRF_HD uint32_t ntt_slot(uint32_t e) { return (uint32_t)NL * (e + (e >> 5) + (e >> 10)); }
VRF_HD uint32_t ntt_brev(uint32_t x, uint32_t bits) { return bits ? __builtin_bitreverse32(x) >> (32 - bits) : 0u; }

// ------------------------------------------------------------------ arithmetic on exact limbs, values < 2q
VRF_HD FeN ntt_add(const FeN& a, const FeN& b) {
  uint32_t x[NL], d[NL], c = 0;
#pragma unroll
  for (int i = 0; i < NL - 1; ++i) {
    const uint32_t t = a.v[i] + b.v[i] + c;
    x[i] = t & LMASK;
    c = t >> LW;
  }
  x[NL - 1] = a.v[NL - 1] + b.v[NL - 1] + c;
  uint32_t borrow = 0;
#pragma unroll
  for (int i = 0; i < NL; ++i) {
    const uint32_t t = x[i] - vrfk::FR_TWOQ29[i] - borrow;
    borrow = t >> 31;
    d[i] = (i < NL - 1) ? (t & LMASK) : t;
  }
  FeN r;
#pragma unroll
  for (int i = 0; i < NL; ++i) r.v[i] = borrow ? x[i] : d[i];
  return r;
}
VRF_HD FeN ntt_sub(const FeN& a, const FeN& b) {
  uint32_t x[NL], y[NL];
  int32_t c = 0;
#pragma unroll
  for (int i = 0; i < NL - 1; ++i) {
    const int32_t t = (int32_t)a.v[i] - (int32_t)b.v[i] + c;
    x[i] = (uint32_t)t & LMASK;
    c = t >> LW;                                   // arithmetic: -1 on a borrow
  }
  const int32_t top = (int32_t)a.v[NL - 1] - (int32_t)b.v[NL - 1] + c;
  x[NL - 1] = (uint32_t)top;
  uint32_t cc = 0;
#pragma unroll
  for (int i = 0; i < NL - 1; ++i) {
    const uint32_t t = x[i] + vrfk::FR_TWOQ29[i] + cc;
    y[i] = t & LMASK;
    cc = t >> LW;
  }
  y[NL - 1] = (uint32_t)(top + (int32_t)vrfk::FR_TWOQ29[NL - 1] + (int32_t)cc);
  FeN r;
#pragma unroll
  for (int i = 0; i < NL; ++i) r.v[i] = top < 0 ? y[i] : x[i];
  return r;
}

// ------------------------------------------------------------------ the tables of a domain
VRF_HD FeN ntt_pow(const FeN& x, uint32_t e) {
  FeN r = fe_one();
#pragma unroll 1
  for (int i = e ? 31 - __builtin_clz(e) : -1; i >= 0; --i) {
    r = fe_sqr(r);
    if ((e >> i) & 1) r = fe_mul(r, x);
  }
  return r;
}
// group_gen of the domain of size 2^log_n: TWO_ADIC_ROOT_OF_UNITY^(2^(32 - log_n))
VRF_HD FeN ntt_group_gen(uint32_t log_n) {
  FeN w = fe_const(vrfk::FR_TWO_ADIC_ROOT_M);
#pragma unroll 1
  for (uint32_t i = log_n; i < (uint32_t)vrfk::FR_TWO_ADICITY; ++i) w = fe_sqr(w);
  return w;
}
VRF_HD void ntt_store_canon(uint32_t* p, const FeN& x) {
  uint32_t c[NL];
  fe_reduce_once(c, x);
#pragma unroll
  for (int i = 0; i < NL; ++i) p[i] = c[i];
}
// consts: n^-1 | offset | offset^-1, NL words each (Montgomery).  offset32 nullable; a zero offset or one >= r: false.
VRF_HD bool ntt_domain_consts(uint32_t* consts, uint32_t log_n, const uint32_t* offset32) {
  ntt_store_canon(consts, ntt_pow(fe_const(vrfk::FR_INV2_M), log_n));
  FeN o = fe_one();
  bool ok = true;
  if (offset32) {
    uint32_t w[8], any = 0;
    kzg_load8(w, offset32);
#pragma unroll
    for (int i = 0; i < 8; ++i) any |= w[i];
    ok = kzg_point(o, w) && any != 0;
    if (!ok) o = fe_one();
  }
  ntt_store_canon(consts + NL, o);
  ntt_store_canon(consts + 2 * NL, fe_inv(o));
  return ok;
}
// entry i of the tables: w^i; for a coset offset^i and n^-1 offset^-i (off / offi nullable together)
VRF_HD void ntt_domain_entry(uint32_t* w, uint32_t* off, uint32_t* offi, const uint32_t* consts, uint32_t log_n, uint32_t i) {
  ntt_store_canon(w + (size_t)i * NL, ntt_pow(ntt_group_gen(log_n), i));
  if (!off) return;
  ntt_store_canon(off + (size_t)i * NL, ntt_pow(fe_load<1, 2>(consts + NL), i));
  ntt_store_canon(offi + (size_t)i * NL, fe_mul(fe_load<1, 2>(consts), ntt_pow(fe_load<1, 2>(consts + 2 * NL), i)));
}

// ------------------------------------------------------------------ the three phases of a pass, one lane each
// lane t of the load phase -> tile element e and index g of the column
VRF_HD void ntt_load_index(const NttPass& P, uint32_t tix, uint32_t t, uint32_t& e, size_t& g) {
  if (P.last) {                                    // NTT_C rows (i_1 consecutive), each contiguous: lanes run along a row
    const uint32_t r = t >> P.b, j = t & ((1u << P.b) - 1);
    const uint32_t lr = P.log_h - P.log_n1;        // bits of the digits between the first and this pass
    const uint32_t rest = tix & ((1u << lr) - 1), i1 = ((tix >> lr) << P.logc) + r;
    e = (j << P.logc) | r;
    g = (((((size_t)i1 << lr) | rest) << P.b) | j);
  } else {                                         // n_p rows of NTT_C contiguous scalars: lanes run along the rows
    const uint32_t log_m = P.log_n - P.log_h - P.b, lmb = log_m - P.logc;
    const uint32_t mblk = tix & ((1u << lmb) - 1), h = tix >> lmb;
    const uint32_t j = t >> P.logc, r = t & ((1u << P.logc) - 1);
    e = t;
    g = (((((size_t)h << P.b) | j) << log_m) | ((size_t)mblk << P.logc) | r);
  }
}
// src: the column, 8 words per scalar.  False: a scalar of the first pass is >= r (it counts as 0).
VRF_HD bool ntt_load_lane(uint32_t* tile, const NttDomain& D, const NttPass& P, uint32_t tix, uint32_t t, const uint32_t* src) {
  uint32_t e, w[8];
  size_t g;
  ntt_load_index(P, tix, t, e, g);
  kzg_load8(w, src + g * 8);
  bool ok = true;
  FeN x;
  if (P.first) {
    Fe<1, 1> p;
    ok = kzg_plain(p, w);
    x = p;
    if (D.off && !P.inverse) x = fe_mul(fe_load<1, 2>(D.off + g * NL), x);
  } else {
    u256_to_limbs(x.v, w);                         // < 2q, as the pass before left it
  }
  fe_store(tile + ntt_slot(e), x);
  return ok;
}

// lane t < elems / 2 of stage s < b: the pair at distance 2^(b - 1 - s) rows
VRF_HD void ntt_bfly_lane(uint32_t* tile, const NttDomain& D, const NttPass& P, uint32_t s, uint32_t t) {
  const uint32_t hl = P.b - 1 - s, dl = hl + P.logc, dm = (1u << dl) - 1;
  const uint32_t lo = ((t & ~dm) << 1) | (t & dm), hi = lo + (1u << dl);
  const FeN a = fe_load<1, 2>(tile + ntt_slot(lo)), b = fe_load<1, 2>(tile + ntt_slot(hi));
  fe_store(tile + ntt_slot(lo), ntt_add(a, b));
  FeN d = ntt_sub(a, b);
  if (hl != 0) {                                   // the last stage's twiddles are all 1
    const uint32_t jl = (lo >> P.logc) & ((1u << hl) - 1);
    size_t k = (size_t)jl << (s + P.log_n - P.b);  // w_{n_p}^(jl 2^s) = w^k, k < n / 2
    if (P.inverse && k) k = ((size_t)1 << P.log_n) - k;
    d = fe_mul(fe_load<1, 2>(D.w + k * NL), d);
  }
  fe_store(tile + ntt_slot(hi), d);
}

// lane t of the store phase: frequency i = t >> logc of row r.  dst: 8 words per scalar.  zero: the column is refused.
VRF_HD void ntt_store_lane(const uint32_t* tile, const NttDomain& D, const NttPass& P, uint32_t tix, uint32_t t, uint32_t* dst,
                           bool zero) {
  const uint32_t r = t & ((1u << P.logc) - 1), i = t >> P.logc;
  FeN x = fe_load<1, 2>(tile + ntt_slot((ntt_brev(i, P.b) << P.logc) | r));
  uint32_t w[8];
  size_t g;
  if (!P.last) {
    const uint32_t log_m = P.log_n - P.log_h - P.b, lmb = log_m - P.logc;
    const uint32_t mblk = tix & ((1u << lmb) - 1), h = tix >> lmb;
    const size_t m = ((size_t)mblk << P.logc) | r;
    g = (((((size_t)h << P.b) | i) << log_m) | m);
    size_t k = (m * i) << P.log_h;                 // the inter-pass twiddle w^(H m i), H m i < n
    if (P.inverse && k) k = ((size_t)1 << P.log_n) - k;
    x = fe_mul(fe_load<1, 2>(D.w + k * NL), x);
    limbs_to_u256(w, x.v);
  } else {
    const uint32_t lr = P.log_h - P.log_n1;
    const uint32_t rest = tix & ((1u << lr) - 1), i1 = ((tix >> lr) << P.logc) + r;
    g = (size_t)i1 + ((size_t)rest << P.log_n1) + ((size_t)i << P.log_h);
    if (P.inverse) x = fe_mul(fe_load<1, 2>(D.offi ? D.offi + g * NL : D.ninv), x);
    uint32_t c[NL];
    fe_reduce_once(c, x);
    limbs_to_u256(w, c);
  }
#pragma unroll
  for (int q = 0; q < 8; ++q) dst[g * 8 + q] = zero ? 0u : w[q];
}

// after a commitment or an opening from evaluations: a column whose transform was refused (ntt_status != 0) keeps status 2
// and gets zeroed outputs, as a coefficient >= r does in launch_kzg_commit / launch_kzg_open.  value, out_xy nullable.
VRF_HD void ntt_merge_status(size_t c, const uint8_t* ntt_status, uint8_t* out48, uint8_t* out_xy, uint8_t* value,
                             uint8_t* status) {
  if (ntt_status[c] == 0) return;
  uint32_t* o = reinterpret_cast<uint32_t*>(out48 + c * 48);
  for (int j = 0; j < 12; ++j) o[j] = 0;
  if (out_xy) {
    uint32_t* x = reinterpret_cast<uint32_t*>(out_xy + c * 96);
    for (int j = 0; j < 24; ++j) x[j] = 0;
  }
  if (value) {
    uint32_t* v = reinterpret_cast<uint32_t*>(value + c * 32);
    for (int j = 0; j < 8; ++j) v[j] = 0;
  }
  status[c] = 2;
}

}  // namespace vrf
