// k_msm.hip -- variable-base multi-scalar multiplication on the suite curve (SURVEY.md section 8
// row a14).  Replaces ark_ec::scalar_mul::VariableBaseMSM::msm for twisted-Edwards affine bases
// (named in BASELINE.json north_star; reached from /root/reference through `reexports`,
// src/lib.rs:14).
//
// Pippenger with signed 11-bit windows (msm.cuh).
//   k_msm_prep    : bases -> Montgomery affine-cached (x, y, d*x*y); scalars -> signed digits
//   k_msm_buckets : one workgroup per (window, point-group); the 1024 buckets of the window live in LDS.
//                   The bucket pass of msm_buckets.cuh with two buckets per lane: counting sort by bucket, the sorted
//                   list cut into 512 equal chunks, heads merged, sum_j j*B_j inside the workgroup.
//   k_msm_final   : sums the groups of every window, shifts window w by 11*w doublings (one DPP quad per
//                   window, the quad's lanes share each doubling), tree-sums the windows, encodes.
#include "kernels.h"
#include "msm.cuh"
#include <cstdlib>

VRF_NS_BEGIN

// ------------------------------------------------------------------------------- prep
template <class S>
__global__ void __launch_bounds__(BLOCK) k_msm_prep(size_t n, const uint8_t* xy, const uint8_t* scalars,
                                                     uint32_t* pts, int16_t* digits, uint8_t* flags, int mont256) {
  size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint32_t* p = reinterpret_cast<const uint32_t*>(xy + i * 64);
  uint32_t xw[8], yw[8], k[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { xw[j] = p[j]; yw[j] = p[8 + j]; }
  load32(k, scalars, i);
  bool ok = !u256_ge(xw, vrfk::Q32) && !u256_ge(yw, vrfk::Q32) && fr_is_canonical<S>(k);
  PtA a;
  uint32_t cw[8];
  a.x = fe_from_abi(cw, xw, mont256 != 0);
  a.y = fe_from_abi(cw, yw, mont256 != 0);
  a.dt = fe_mul(fe_mul(a.x, a.y), S::d());
  // on-curve check: a*x^2 + y^2 == 1 + d*x^2*y^2  <=>  y^2 - ANEG x^2 - 1 - (d x y) * (x y) == 0
  FeN x2 = fe_sqr(a.x), y2 = fe_sqr(a.y), xy_ = fe_mul(a.x, a.y);
  auto lhs = te_curve_lhs<S>(x2, y2);
  ok = ok && fe_eq(lhs, fe_mul(a.dt, xy_));
  pta_store(pts + i * MSM_PTA_STRIDE, a);
  if (!ok) flags[0] = 1;
  msm_write_digits<S>(digits, n, i, k, false, !ok);
}

// ------------------------------------------------------------------------------- buckets
VRF_HD void lds_store_pt(uint32_t* dst, const PtE& p) {
  fe_store(dst, p.X); fe_store(dst + NL, p.Y); fe_store(dst + 2 * NL, p.Z); fe_store(dst + 3 * NL, p.T);
}
VRF_HD PtE lds_load_pt(const uint32_t* src) {
  PtE p;
  p.X = fe_load<1, 5>(src); p.Y = fe_load<1, 5>(src + NL); p.Z = fe_load<1, 5>(src + 2 * NL);
  p.T = fe_load<1, 5>(src + 3 * NL);
  return p;
}

// the twisted-Edwards instantiation of msm_bucket_pass (msm_buckets.cuh): extended accumulators, affine-cached inputs, two
// buckets per lane.  TeMsmShape is what the host side needs of it.
struct TeMsmShape {
  static constexpr int BLOCK = MSM_BLOCK, BPL = MSM_BPL, PT_WORDS = MSM_PT_WORDS, AFF_STRIDE = MSM_PTA_STRIDE, IDX_BITS = MSM_IDX_BITS;
  static constexpr int HIST_LOADS = 4, SCATTER_LOADS = 4;
};
template <class S>
struct TeMsm : TeMsmShape {
  using Acc = PtE;
  using Aff = PtA;
  static VRF_HD PtE identity() { return te_identity(); }
  static VRF_HD PtE load(const uint32_t* src) { return lds_load_pt(src); }
  static VRF_HD void store(uint32_t* dst, const PtE& p) { lds_store_pt(dst, p); }
  static VRF_HD PtA aff_load(const uint32_t* src) { return pta_load(src); }
  static VRF_HD PtA aff_identity() { return pta_identity(); }
  static VRF_HD PtE madd(const PtE& p, const PtA& q, bool neg) { return te_add_affine<S>(p, q, neg); }
  static VRF_HD PtE add(const PtE& p, const PtE& q) { return te_add<S>(p, q); }
  static VRF_HD PtE dbl(const PtE& p) { return te_dbl<S>(p, true); }
};

template <class S>
__global__ void __launch_bounds__(MSM_BLOCK) k_msm_buckets(MsmLayout L) {
  extern __shared__ uint32_t lds[];
  // low windows (all points) first, then the high windows (only the points with full-size scalars)
  // GROUP-major: consecutive workgroups are the windows of ONE point group, so the workgroups that run at the same time
  // gather from the same few slices of the point array and find each other's lines in the Infinity Cache / L2 (window-major
  // order streamed the whole array from HBM once per window: 16.6 GB per batched-Pedersen launch, 2.2 TB/s of random 128-B
  // reads -- the bound behind the 0.72 of the issue slots)
  const int wg = blockIdx.x;
  const int n_lo_wgs = MSM_W_SHORT * L.groups;
  const bool low = wg < n_lo_wgs;
  const int w = low ? wg % MSM_W_SHORT : MSM_W_SHORT + (wg - n_lo_wgs) % (MSM_W - MSM_W_SHORT);
  const int g = low ? wg / MSM_W_SHORT : (wg - n_lo_wgs) / (MSM_W - MSM_W_SHORT);
  const size_t span = low ? L.per_group : L.per_group_hi, end = low ? L.n : L.n_long;
  const size_t lo = (size_t)g * span;
  const size_t hi = lo + span < end ? lo + span : end;
  MsmBucketJob job;
  job.digits = L.digits + (size_t)w * L.n + lo;
  job.pts = L.pts + lo * MSM_PTA_STRIDE;
  job.count = lo < hi ? (uint32_t)(hi - lo) : 0u;
  job.list = L.lists + (size_t)wg * L.list_cap;
  job.heads = L.heads + (size_t)wg * MSM_BLOCK * MSM_PT_WORDS;
  job.out = L.part + ((size_t)w * L.groups + g) * MSM_PT_WORDS;
  msm_bucket_pass<TeMsm<S>>(job, lds);
}

// ------------------------------------------------------------------------------- final
// Quad-parallel point arithmetic: the four lanes of a DPP quad hold the same point and share one
// doubling -- the four squarings, then the four products, of dbl-2008-hwcd run one per lane, and the
// results travel inside the quad by DPP quad_perm broadcasts (VALU moves, no LDS).  The critical path of
// a doubling drops from 4S + 4M to 1S + 1M; that path (242 doublings for the top window) is the whole
// run time of this single-workgroup kernel.
template <int K>
VRF_HD uint32_t quad_bcast_u32(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, K * 0x55, 0xf, 0xf, false);   // quad_perm:[K,K,K,K]
#else
  return v;
#endif
}
template <int K, int L, int V>
VRF_HD Fe<L, V> quad_bcast(const Fe<L, V>& a) {
  Fe<L, V> r;
#pragma unroll
  for (int i = 0; i < NL; ++i) r.v[i] = quad_bcast_u32<K>(a.v[i]);
  return r;
}
// bounds of the operands are proved per call site; the typed multiplier is bypassed
template <int L, int V>
VRF_HD const Fe<1, 1>& fe_unchecked(const Fe<L, V>& a) { return reinterpret_cast<const Fe<1, 1>&>(a); }
template <int LO, int VO, int L, int V>
VRF_HD const Fe<LO, VO>& fe_assume(const Fe<L, V>& a) { return reinterpret_cast<const Fe<LO, VO>&>(a); }

// 2P with the work split over the quad; q = lane index inside the quad.  In: every lane holds (X, Y, Z).
// Out: every lane holds (X, Y, Z, T) of 2P.
template <class C>
VRF_HD PtE te_dbl_quad(const PtE& p, int q) {
  // lane q squares one of X, Y, X+Y, Z                              operand bound (2,10)
  Fe<2, 10> xy = fe_add(p.X, p.Y), opnd = xy;
#pragma unroll
  for (int i = 0; i < NL; ++i) opnd.v[i] = q == 0 ? p.X.v[i] : q == 1 ? p.Y.v[i] : q == 2 ? xy.v[i] : p.Z.v[i];
  auto sq = fe_sqr(opnd);                                            // typed (1,3) for the widest operand
  // lanes 0, 1, 3 squared a coordinate (value < 5q): their squares are < 2q, as in te_dbl
  const FeN A = fe_assume<1, 2>(quad_bcast<0>(sq)), B = fe_assume<1, 2>(quad_bcast<1>(sq)),
            ZZ = fe_assume<1, 2>(quad_bcast<3>(sq));
  const auto Sx = quad_bcast<2>(sq);                                 // (X+Y)^2              (1,3)
  // lane 0: X = E*F, lane 1: Y = G*H, lane 2: Z = F*G, lane 3: T = E*H.  All four factors are normalised
  // (L = 1) and each product obeys the value bounds of te_dbl, so the result fits FeP.
  Fe<1, 1> lhs, rhs;
  auto place = [&](const auto& E, const auto& F, const auto& G, const auto& H) {
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      lhs.v[i] = (q == 0 || q == 3) ? E.v[i] : q == 1 ? G.v[i] : F.v[i];
      rhs.v[i] = q == 0 ? F.v[i] : q == 2 ? G.v[i] : H.v[i];
    }
  };
  if constexpr (C::A_PLUS_ONE) {
    auto G = fe_norm(fe_add(A, B));                                    // A + B                (1,4)
    auto E = fe_norm(fe_sub(Sx, G));                                   // S - A - B = 2XY      (1,11)
    auto F = fe_norm(fe_sub(G, fe_dbl(ZZ)));                           // G - 2Z^2             (1,12)
    auto H = fe_norm(fe_sub(A, B));                                    // A - B                (1,6)
    static_assert(mul_v(11, 12) <= 5 && mul_v(4, 6) <= 5 && mul_v(12, 4) <= 5 && mul_v(11, 6) <= 5,
                  "quad doubling: products must stay inside FeP");
    place(E, F, G, H);
  } else {
    auto E = fe_norm(fe_sub(fe_add(A, B), Sx));                        // A + B - S            (1,8)
    auto aA = C::mul_aneg(A);
    auto H = fe_norm(fe_add(aA, B));                                   // -a*A + B             (1,12)
    auto G = fe_norm(fe_sub(aA, B));                                   // -a*A - B             (1,14)
    auto F = fe_norm(fe_add(G, fe_dbl(ZZ)));                           // G + 2Z^2             (1,18)
    static_assert(mul_v(8, 18) <= 5 && mul_v(14, 12) <= 5 && mul_v(18, 14) <= 5 && mul_v(8, 12) <= 5,
                  "quad doubling: products must stay inside FeP");
    place(E, F, G, H);
  }
  FeP prod = fe_mul(fe_unchecked(lhs), fe_unchecked(rhs));
  PtE r;
  r.X = quad_bcast<0>(prod); r.Y = quad_bcast<1>(prod); r.Z = quad_bcast<2>(prod); r.T = quad_bcast<3>(prod);
  return r;
}

constexpr int MSM_FINAL_BLOCK = 128;     // 23 windows x 4 lanes = 92 active lanes in two waves

template <class S>
__global__ void __launch_bounds__(MSM_FINAL_BLOCK) k_msm_final(const uint32_t* part, int groups, int groups_hi,
                                                               uint8_t* out_enc, uint8_t* out_xy,
                                                               const uint8_t* flags, uint8_t* status,
                                                               uint8_t* fail_flag, uint32_t sflags) {
  __shared__ uint32_t stage[32 * MSM_PT_WORDS];
  const int t = threadIdx.x, w = t >> 2, q = t & 3;
  // quad w < 23: R_w = sum over the groups (lane q takes groups q, q+4, ...; two butterfly steps join
  // them), then 2^(11 w) * R_w by 11 w quad-parallel doublings.  Quads run in lockstep: the critical path
  // is the top window's 242 doublings instead of a serial 253-doubling Horner.
  PtE acc = te_identity();
  if (w < MSM_W) {
    const int ng = w < MSM_W_SHORT ? groups : groups_hi;
    for (int g = q; g < ng; g += 4)
      acc = te_add<S>(acc, lds_load_pt(part + ((size_t)w * groups + g) * MSM_PT_WORDS));
  }
#pragma unroll 1
  for (int step = 1; step <= 2; step <<= 1) {
    PtE o;
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      o.X.v[i] = __shfl_xor(acc.X.v[i], step, 64); o.Y.v[i] = __shfl_xor(acc.Y.v[i], step, 64);
      o.Z.v[i] = __shfl_xor(acc.Z.v[i], step, 64); o.T.v[i] = __shfl_xor(acc.T.v[i], step, 64);
    }
    acc = te_add<S>(acc, o);
  }
  // one representation for the whole quad (a + b and b + a agree only modulo q)
  acc.X = quad_bcast<0>(acc.X); acc.Y = quad_bcast<0>(acc.Y); acc.Z = quad_bcast<0>(acc.Z); acc.T = quad_bcast<0>(acc.T);
  const int nd = w < MSM_W ? MSM_C * w : 0;
#pragma unroll 1
  for (int j = 0; j < MSM_C * (MSM_W - 1); ++j)
    if (j < nd) acc = te_dbl_quad<S>(acc, q);
  // tree-sum of the 23 window results through LDS
  __syncthreads();
  if (q == 0 && w < 32) lds_store_pt(stage + w * MSM_PT_WORDS, acc);     // quads 23..31 hold the identity
  __syncthreads();
  if (t < 32) acc = lds_load_pt(stage + t * MSM_PT_WORDS);
#pragma unroll 1
  for (int s = 16; s >= 1; s >>= 1) {
    __syncthreads();
    if (t < 32) lds_store_pt(stage + t * MSM_PT_WORDS, acc);
    __syncthreads();
    if (t < s) acc = te_add<S>(acc, lds_load_pt(stage + (t + s) * MSM_PT_WORDS));
  }
  if (t == 0) {
    const bool bad = flags[0] != 0;
    if (!out_enc && !out_xy) {
      // verdict only (batched verification): the neutral element is X == 0, Y == Z; no inversion
      const bool neutral = fe_is_zero(acc.X) && fe_eq(acc.Y, acc.Z);
      if (fail_flag && (!neutral || bad)) fail_flag[0] = 1;
      if (status) status[0] = bad ? ST_INVALID_DATA : ST_OK;
      return;
    }
    FeN x, y;
    te_to_affine(x, y, acc);
    uint32_t e[8], xw[8], yw[8];
    te_encode_affine(e, x, y, sflags);
    fe_to_u256(xw, x); fe_to_u256(yw, y);
    // neutral element: x == 0 and y == 1
    uint32_t nz = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) nz |= xw[j] | (yw[j] ^ (j == 0 ? 1u : 0u));
    if (fail_flag && (nz != 0 || bad)) fail_flag[0] = 1;
    if (bad) {
#pragma unroll
      for (int j = 0; j < 8; ++j) { e[j] = 0; xw[j] = 0; yw[j] = 0; }
    }
    if (out_enc) store32(out_enc, 0, e);
    if (out_xy) {
      uint32_t* p = reinterpret_cast<uint32_t*>(out_xy);
#pragma unroll
      for (int j = 0; j < 8; ++j) { p[j] = xw[j]; p[8 + j] = yw[j]; }
    }
    if (status) status[0] = bad ? ST_INVALID_DATA : ST_OK;
  }
}

// ------------------------------------------------------------------------------- host
// high-window groups for `groups` low-window groups: proportional to the share of full-size scalars
static int msm_groups_hi(size_t n, size_t n_long, int groups) {
  if (n_long >= n) return groups;
  int gh = (int)(((double)n_long / (double)n) * groups + 0.5);
  size_t min_g = (n_long + MSM_MAX_PER_GROUP - 1) / MSM_MAX_PER_GROUP;
  if ((size_t)gh < min_g) gh = (int)min_g;
  return gh < 1 ? 1 : gh;
}

int msm_groups(size_t n, size_t n_long, int cus) {
  // Workgroups = MSM_W_SHORT g + (MSM_W - MSM_W_SHORT) g_hi, as many per CU as their LDS allows (one with 1024 buckets):
  // aim at one full round of the chip for mid-sized inputs and two for large ones (the dispatcher evens out the tails), at
  // least 16 points per lane and group, never more than 2^21 points per group.
  const int slots = cus;                          // 1024 buckets x 144 B: one workgroup per CU
  const int rounds = n >= (size_t(1) << 22) ? 2 : 1;
  const double share = n ? (double)n_long / (double)n : 1.0;
  int g = (int)(rounds * slots / (MSM_W_SHORT + (MSM_W - MSM_W_SHORT) * share));
  if (g < 1) g = 1;
  while (g > 1 && MSM_W_SHORT * g + (MSM_W - MSM_W_SHORT) * msm_groups_hi(n, n_long, g) > rounds * slots) --g;
  size_t max_g = (n + 8191) / 8192;
  if ((size_t)g > max_g) g = (int)max_g;
  if (g < 1) g = 1;
  size_t min_g = (n + MSM_MAX_PER_GROUP - 1) / MSM_MAX_PER_GROUP;
  if ((size_t)g < min_g) g = (int)min_g;
  return g;
}

// the regions of an MSM over n points in `groups` groups, sized for the worst case groups_hi == groups
static void msm_carve(MsmCarve& c, MsmLayout& L, size_t n, int groups) {
  L.per_group = (n + groups - 1) / groups;
  L.list_cap = L.per_group + MSM_BLOCK;
  const MsmRegions r = msm_carve_regions<TeMsmShape>(c, n, MSM_W, n, (size_t)MSM_W * groups, L.list_cap);
  L.pts = r.pts; L.digits = r.digits; L.lists = r.lists; L.heads = r.heads; L.part = r.part;
  L.flags = c.take<uint8_t>(256);
}

size_t msm_workspace_bytes(size_t n, int groups) {
  MsmLayout L;
  MsmCarve c(nullptr);
  msm_carve(c, L, n, groups);
  return c.off;
}

MsmLayout msm_layout(size_t n, size_t n_long, int groups, void* ws) {
  MsmLayout L;
  MsmCarve c(ws);
  msm_carve(c, L, n, groups);
  L.sflags = 0;
  L.n = n;
  L.n_long = n_long < n ? n_long : n;
  L.groups = groups;
  L.groups_hi = msm_groups_hi(n, L.n_long, groups);
  if (L.groups_hi > groups) L.groups_hi = groups;
  L.per_group_hi = (L.n_long + L.groups_hi - 1) / L.groups_hi;
  // groups_hi rounds to nearest, so a high-window group can be slightly larger than a low-window one;
  // the list capacity was sized for per_group: keep within it
  while (L.per_group_hi > L.per_group && L.groups_hi < groups) {
    ++L.groups_hi;
    L.per_group_hi = (L.n_long + L.groups_hi - 1) / L.groups_hi;
  }
  return L;
}

template <class S>
static void launch_msm_core_t(const MsmLayout& L, uint8_t* out_enc, uint8_t* out_xy, uint8_t* status,
                              uint8_t* fail_flag, hipStream_t st, hipEvent_t* ev) {
  const size_t lds_bytes = msm_bucket_lds_bytes<TeMsm<S>>();   // 155,712 B of 160 KiB
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_msm_buckets<S>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    attr_set = true;
  }
  const int wgs = MSM_W_SHORT * L.groups + (MSM_W - MSM_W_SHORT) * L.groups_hi;
  hipLaunchKernelGGL(k_msm_buckets<S>, dim3(wgs), dim3(MSM_BLOCK), lds_bytes, st, L);
  if (ev) (void)hipEventRecord(ev[0], st);
  hipLaunchKernelGGL(k_msm_final<S>, dim3(1), dim3(MSM_FINAL_BLOCK), 0, st, L.part, L.groups, L.groups_hi, out_enc, out_xy, L.flags,
                     status, fail_flag, L.sflags);
  if (ev) { (void)hipEventRecord(ev[1], st); (void)hipEventRecord(ev[2], st); }
}

void launch_msm_core(int suite, const MsmLayout& L, uint8_t* out_enc, uint8_t* out_xy, uint8_t* status,
                     uint8_t* fail_flag, hipStream_t st, hipEvent_t* ev) {
  VRF_DISPATCH_SUITE(suite, launch_msm_core_t<S>(L, out_enc, out_xy, status, fail_flag, st, ev));
}

// mont256 != 0: the bases' coordinates are Montgomery images x 2^256 mod q (VRFHIP_FLAG_COORDS_MONT256); out_xy stays
// canonical here (api.hip converts it with launch_xy_to_mont256)
void launch_msm_coords(int suite, size_t n, const uint8_t* xy, const uint8_t* scalars, uint8_t* out_enc,
                       uint8_t* out_xy, uint8_t* status, void* ws, int groups, int mont256, uint32_t sflags,
                       hipStream_t st) {
  MsmLayout L = msm_layout(n, n, groups, ws);
  L.sflags = sflags;
  (void)hipMemsetAsync(L.flags, 0, 256, st);
  VRF_DISPATCH_SUITE(suite, hipLaunchKernelGGL(k_msm_prep<S>, grid_for(n), dim3(BLOCK), 0, st, n, xy, scalars,
                                               L.pts, L.digits, L.flags, mont256));
  launch_msm_core(suite, L, out_enc, out_xy, status, nullptr, st);
}
void launch_msm(int suite, size_t n, const uint8_t* xy, const uint8_t* scalars, uint8_t* out_enc,
                uint8_t* out_xy, uint8_t* status, void* ws, int groups, hipStream_t st) {
  launch_msm_coords(suite, n, xy, scalars, out_enc, out_xy, status, ws, groups, 0, 0, st);
}

VRF_NS_END
