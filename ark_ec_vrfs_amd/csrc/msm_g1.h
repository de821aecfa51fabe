// msm_g1.h -- launch interface of the BLS12-381 G1 multi-scalar multiplication (k_msm_g1.hip) for api.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace vrf {

constexpr int G1_C = 10;                       // signed window bits: 512 buckets x 168 B = 84 KiB of LDS
constexpr int G1_BUCKETS = 1 << (G1_C - 1);
constexpr int G1_BLOCK = 512;                  // lanes per workgroup = buckets
constexpr int G1_W_FULL = 26;                  // windows of a 255-bit scalar (260 bits)
constexpr int G1_W_SHORT = 13;                 // windows of a 128-bit weight (130 bits)
constexpr int G1_PT_WORDS = 42;                // projective (X, Y, Z), 14 limbs each
constexpr int G1_AFF_WORDS = 28;               // Montgomery affine (x, y)
constexpr int G1_AFF_STRIDE = 32;              // words between the points of L.pts: 112 B in a 128-B slot (one cache line per gather)
constexpr int G1_IDX_BITS = 21;
constexpr size_t G1_MAX_PER_GROUP = size_t(1) << G1_IDX_BITS;

// Device layout of one call: `sets` point sets (1 = plain MSM, 2 = the A and B sides of a batched pairing check)
// that share nothing but the schedule.
struct G1MsmLayout {
  size_t n;
  int sets, windows, groups;
  size_t per_group, list_cap;
  uint32_t* pts;      // [sets][n][G1_AFF_STRIDE]  Montgomery affine coordinates
  int16_t* digits;    // [sets][windows][n]        signed digits in [-511, 512]; 0 = the point takes no part
  uint32_t* lists;    // [sets*windows*groups][list_cap] bucket-sorted entries, lane-transposed
  uint32_t* heads;    // [sets*windows*groups][G1_BLOCK][G1_PT_WORDS] first-run partial sums
  uint32_t* part;     // [sets][windows][groups][G1_PT_WORDS] per-workgroup window sums
  uint8_t* sums;      // [sets][96]  results in the wire format (x || y, 48-byte little-endian; all-zero = infinity)
  uint8_t* flags;     // [256]  flags[0] != 0: an input of the plain MSM was invalid
};
int g1_msm_groups(size_t n, int sets, int windows, int cus);
size_t g1_msm_workspace_bytes(size_t n, int sets, int windows, int groups);
G1MsmLayout g1_msm_layout(size_t n, int sets, int windows, int groups, void* ws);

// Batched pairing check, G1 side: validates the 2n points (g1: n x 192 B), derives the 128-bit weights
// z_i = SHA-512("vrfhip-pairing-rlc-v2" || seed || d_root[32] || u64_le(index0 + i))[0..16] (d_root: the batch digest of
// digest.cuh over the g1 items, device memory), writes status[i] in {0, 2} and leaves
// (sum z_i A_i, sum z_i B_i) in L.sums -- exactly one g1 item for the pairing kernel.  L: sets = 2, windows = 13.
// ev (nullable, 3 events): after prep, after buckets, after final.
void launch_g1_rlc(const G1MsmLayout& L, const uint8_t* g1, const uint8_t seed[32], const uint8_t* d_root, uint64_t index0,
                   uint8_t* status,
                   hipStream_t st, hipEvent_t* ev = nullptr);
// `VariableBaseMSM::msm` on G1: bases n x 96 B, scalars n x 32 B little-endian (< r); result in L.sums[0..96],
// status1[0] = 0 / 2 (a coordinate >= p, a point off the curve or a scalar >= r).  L: sets = 1, windows = 26.
void launch_g1_msm(const G1MsmLayout& L, const uint8_t* bases, const uint8_t* scalars, uint8_t* status1, hipStream_t st);
// The two kernels behind both calls above, for a prep kernel of another unit (k_kzg.hip): the bucket sums of every
// (set, window, group) of a filled layout, then L.sums.
// shared_pts: every set reads the SAME n points at L.pts (the columns of a commitment over resident bases) instead of its own
// n at L.pts + set * n * G1_AFF_STRIDE; a second instantiation of the kernel, the first one is untouched.
void launch_g1_buckets(const G1MsmLayout& L, hipStream_t st, bool shared_pts = false);
void launch_g1_final(const G1MsmLayout& L, hipStream_t st);

// G1 codec (k_g1_codec.hip, g1_codec.cuh), one lane per point, no workspace; all arrays 4-byte aligned device memory.
// points48: n x 48 B compressed (zcash / ark-bls12-381 form); g1_xy: n x 96 B affine as above; status[i] = 0 / 2.
constexpr size_t G1_CODEC_CHUNK = size_t(1) << 20;       // items per launch
void launch_g1_decode(size_t n, const uint8_t* points48, bool check_subgroup, uint8_t* g1_xy, uint8_t* status, hipStream_t st);
void launch_g1_validate(size_t n, const uint8_t* g1_xy, uint8_t* status, hipStream_t st);
void launch_g1_encode(size_t n, const uint8_t* g1_xy, uint8_t* points48, uint8_t* status, hipStream_t st);

// Per-item linear combinations (k_g1_lincomb.hip, g1_lincomb.cuh), one lane per term, no workspace:
// out[i] = sum_{j<k} scalars[i][j] bases[i][j] + sum_{j<m} shared_scalars[i][j] shared_bases[j], 1 <= k + m <= 16.
// bases: n x k x 96 B, scalars: n x k x 32 B, shared_bases: m x 96 B, shared_scalars: n x m x 32 B (an array whose count is
// 0 is not read); the result of item i: 96 B at out + i * out_stride; status[i] = 0 / 2.  All arrays 4-byte aligned.
constexpr size_t G1_LINCOMB_CHUNK = size_t(1) << 20;     // items per launch
constexpr int G1_LINCOMB_BLOCK = 128;                    // lanes per workgroup: a multiple of every group size 1 .. 16
void launch_g1_lincomb(size_t n, uint32_t k, const uint8_t* bases, const uint8_t* scalars, uint32_t m,
                       const uint8_t* shared_bases, const uint8_t* shared_scalars, uint8_t* out, size_t out_stride,
                       uint8_t* status, hipStream_t st);

// KZG openings (k_kzg.hip, kzg.cuh).  g1c / g1p: the decoded commitments and proofs, n x 96 B (launch_g1_decode; an invalid
// one is all-0xFF); z, v: n x 32 B little-endian; vk: g (96 B) || h || beta_h (192 B each).  All arrays 4-byte aligned.
constexpr int KZG_BLOCK = 128;                           // items per workgroup of the prep kernel = one partial sum
constexpr int KZG_PART_WORDS = 9;                        // one Fr partial sum (fe.cuh limbs)
constexpr size_t KZG_ITEM_CHUNK = size_t(1) << 20;       // items per launch group of the per-item form
// Per-item form: for every item the rows of launch_g1_lincomb(k = 2, m = 1, shared base g) whose result is
// A_i = C_i - v_i g + z_i pi_i -- bases n x 192 B, scalars n x 64 B, shared_scalars n x 32 B -- and B_i = -pi_i at
// items + i * 192 + 96.  dec_status: the 2n decode statuses (commitments, then proofs).  An item with an invalid point or
// with z_i >= r or v_i >= r gets all-0xFF rows and B_i, so that it ends with status 2 in the lincomb and pairing launches.
void launch_kzg_item_rows(size_t n, const uint8_t* g1c, const uint8_t* g1p, const uint8_t* dec_status, const uint8_t* z,
                          const uint8_t* v, uint8_t* bases, uint8_t* scalars, uint8_t* shared_scalars, uint8_t* items,
                          hipStream_t st);
// Batched form: r_i = SHA-512("vrfhip-kzg-rlc-v1" || seed || d_root[32] || u64_le(i))[0..16]; fills S (sets = 2, windows =
// G1_W_SHORT, n points: C_i and pi_i under r_i) and F (sets = 1, windows = G1_W_FULL, n + 1 points: pi_i under r_i z_i mod r
// and g under -sum r_i v_i mod r), runs both multi-scalar multiplications and writes the one pairing item
// S_A || S_B = (S.sums[0] + F.sums[0]) || -S.sums[1] to item192 (all-0xFF if g is invalid).  status[i] = 0 / 2.
// partials: kzg_partials(n) * KZG_PART_WORDS words.  ev (nullable, 3 events): after prep + fold,
// after the buckets of both layouts, after final + combine.
inline size_t kzg_partials(size_t n) { return (n + KZG_BLOCK - 1) / KZG_BLOCK; }
void launch_kzg_rlc(const G1MsmLayout& S, const G1MsmLayout& F, const uint8_t* g1c, const uint8_t* g1p, const uint8_t* z,
                    const uint8_t* v, const uint8_t* vk, const uint8_t seed[32], const uint8_t* d_root, uint32_t* partials,
                    uint8_t* status, uint8_t* item192, hipStream_t st, hipEvent_t* ev = nullptr);

// Multi-commitment, multi-point KZG openings (k_kzg_multi.hip, kzg_multi.cuh), shape (k, m, p) per call: k own commitments,
// the shared bases g, S_1 .. S_m and p proofs per item, k + p + m + 1 <= 16, p >= 1.  The arrays of n items, 4-byte aligned:
struct KzgMultiArrays {
  const uint8_t* g1c;             // n k x 96 B decoded commitments (launch_g1_decode; an invalid one is all-0xFF)
  const uint8_t* scalars;         // n k x 32 B        s_ij
  const uint8_t* shared_scalars;  // n (m + 1) x 32 B  t_i0 (for g), t_i1 .. t_im
  const uint8_t* g1p;             // n p x 96 B decoded proofs
  const uint8_t* points;          // n p x 32 B        z_ij
  const uint8_t* coefs;           // n p x 32 B        u_ij
  const uint8_t *dec_c, *dec_p;   // the n k and n p decode statuses
};
// Per-item form: the rows of two launch_g1_lincomb calls.  A_i: bases_a n (k + p) x 96 B = [C_i*, pi_i*] under scalars_a
// = [s_ij, u_ij z_ij mod r], shared terms [g, S_*] under shared_a = t_i*; B_i: bases_b n p x 96 B = pi_i* under scalars_b
// = r - u_ij.  An item with an invalid point or a scalar >= r gets all-0xFF rows in all five arrays.
void launch_kzg_multi_item_rows(size_t n, uint32_t k, uint32_t m, uint32_t p, const KzgMultiArrays& a, uint8_t* bases_a,
                                uint8_t* scalars_a, uint8_t* shared_a, uint8_t* bases_b, uint8_t* scalars_b, hipStream_t st);
// Batched form: r_i = SHA-512("vrfhip-kzg-multi-rlc-v1" || u32_le(k) || u32_le(m) || u32_le(p) || seed || d_root[32] ||
// u64_le(i))[0..16]; fills A (sets = 1, windows = G1_W_FULL, n (k + p) + m + 1 points: the own terms item by item under
// r_i s_ij and r_i u_ij z_ij, then g, S_1 .. S_m under sum_i r_i t_ij) and B (sets = 1, windows = G1_W_FULL, n p points: pi_ij
// under r_i u_ij), runs both multi-scalar multiplications and writes the one pairing item A.sums || -B.sums to item192
// (all-0xFF if g or a shared base is invalid).  status[i] = 0 / 2.  g: 96 B; shared_bases: m x 96 B (not read for m = 0).
// weights: n * 4 words; partials: (m + 1) * kzg_partials(n) * KZG_PART_WORDS words.  ev (nullable, 3 events): after prep + fold,
// after the buckets of both layouts, after final + combine.
void launch_kzg_multi_rlc(const G1MsmLayout& A, const G1MsmLayout& B, size_t n, uint32_t k, uint32_t m, uint32_t p,
                          const KzgMultiArrays& a, const uint8_t* g, const uint8_t* shared_bases, const uint8_t seed[32],
                          const uint8_t* d_root, uint32_t* weights, uint32_t* partials, uint8_t* status, uint8_t* item192,
                          hipStream_t st, hipEvent_t* ev = nullptr);

// KZG commitments and openings over a resident base set (k_kzg_prove.hip, kzg_prove.cuh).
// A resident base: Montgomery affine (x, y) in a G1_AFF_STRIDE slot as k_g1_buckets gathers it, word G1_SRS_INF_WORD != 0 for
// the point at infinity (its digits are written as zero, its coordinates are never read).
constexpr int G1_SRS_INF_WORD = G1_AFF_WORDS;
constexpr size_t G1_SRS_MAX = size_t(1) << 20;           // points of a base set
constexpr int KZGQ_BLOCK = 256;                          // lanes per workgroup of k_kzg_quotient
constexpr int KZGQ_CHUNK_MAX = 16;                       // coefficients per lane before a polynomial takes more workgroups
// how a polynomial of len coefficients is cut: `chunk` coefficients per lane, `wgs` workgroups of KZGQ_BLOCK lanes.  Up to
// KZGQ_BLOCK coefficients one per lane; the chunk grows to KZGQ_CHUNK_MAX, then the workgroups multiply (16 at len = 2^16).
struct KzgCut { uint32_t chunk, wgs; };
inline KzgCut kzg_cut(size_t len) {
  KzgCut c;
  size_t m = (len + KZGQ_BLOCK - 1) / KZGQ_BLOCK;
  if (m < 1) m = 1;
  if (m > (size_t)KZGQ_CHUNK_MAX) m = KZGQ_CHUNK_MAX;
  c.chunk = (uint32_t)m;
  const size_t per_wg = m * KZGQ_BLOCK;
  c.wgs = (uint32_t)(len ? (len + per_wg - 1) / per_wg : 1);
  return c;
}
constexpr size_t KZG_PROVE_GROUP_SCALARS = size_t(1) << 20;   // a launch group: at most this many scalars ...
constexpr size_t KZG_PROVE_GROUP_COLUMNS = 64;                // ... and this many columns (at least one)
// xy / status: n decoded points and their statuses (launch_g1_decode) -> n slots; an invalid point leaves a zeroed slot
void launch_g1_srs_fill(size_t n, const uint8_t* g1_xy, const uint8_t* status, uint32_t* slots, hipStream_t st);
// A layout of `sets` columns over n SHARED points (pts: the first slot), windows = G1_W_FULL, without a point region:
// digits | lists | heads | part | wg_sums (sets x q_wgs x KZG_PART_WORDS words) | sums (sets x 96 B) | flags (one byte per set).
// [digits, sums) holds functions of the scalars alone: the callers wipe it (g1_shared_secret_bytes from L.digits).
size_t g1_shared_workspace_bytes(size_t n, int sets, int groups, size_t q_wgs);
G1MsmLayout g1_shared_layout(size_t n, int sets, int groups, size_t q_wgs, void* ws, uint32_t* pts, uint32_t** wg_sums);
size_t g1_shared_secret_bytes(const G1MsmLayout& L);
// ev (nullable, 5 events): start | prep or quotient | buckets | final | encode.
// Commit: out[c] = sum_j coeffs[c][j] pts[j], c < L.sets, j < L.n; coeffs: sets x n x 32 B.  out48: sets x 48 B compressed,
// out_xy (nullable): sets x 96 B, status[c] = 0 / 2 (a scalar >= r: the column's outputs are zeroed).  L.n = 0: infinity.
void launch_kzg_commit(const G1MsmLayout& L, const uint8_t* coeffs, uint8_t* out48, uint8_t* out_xy, uint8_t* status,
                       hipStream_t st, hipEvent_t* ev = nullptr);
// Open: L.sets polynomials of len = L.n + 1 coefficients (coeffs: sets x len x 32 B) at z (sets x 32 B): value (sets x 32 B),
// proof48 / proof_xy / status as above (status 2 also for z >= r; value is zeroed too).
void launch_kzg_open(const G1MsmLayout& L, uint32_t* wg_sums, const uint8_t* coeffs, const uint8_t* z, uint8_t* value,
                     uint8_t* proof48, uint8_t* proof_xy, uint8_t* status, hipStream_t st, hipEvent_t* ev = nullptr);

// Radix-2 transforms over Fr on a resident domain (k_fr_ntt.hip, fr_ntt.cuh).  The tables of a domain of size n = 2^log_n,
// 9-limb Montgomery images: w [n] = w^i; for a coset off [n] = offset^i and offi [n] = n^-1 offset^-i (both nullptr for the
// plain domain); consts: n^-1 | offset | offset^-1.
struct FrNttTables {
  uint32_t log_n;
  uint32_t *w, *off, *offi, *consts;
};
int fr_ntt_passes(uint32_t log_n);                        // launches of one transform
int fr_ntt_max_log();
size_t fr_ntt_table_words(uint32_t log_n);                // words of one table
size_t fr_ntt_const_words();
// d_offset32 (device, nullable = 1): 32 bytes little-endian, nonzero and < r (the caller has checked)
void launch_fr_domain_fill(const FrNttTables& T, const uint8_t* d_offset32, hipStream_t st);
// k columns of n scalars (32 B little-endian), natural order in and out; in == out allowed.  scratch: k n 32 B, read and
// written only by a plan of more than one pass (it then holds functions of the columns: the callers wipe it).
// status[c] = 0 / 2 (a scalar >= r: the column's output is zero).  k * tiles < 2^31.
void launch_fr_ntt(const FrNttTables& T, size_t k, bool inverse, const uint8_t* in, uint8_t* out, uint8_t* scratch,
                   uint8_t* status, hipStream_t st);
// after launch_kzg_commit / launch_kzg_open on the inverse transforms of k columns: a column with ntt_status != 0 gets
// status 2 and zeroed outputs (out_xy, value nullable)
void launch_fr_ntt_merge(size_t k, const uint8_t* ntt_status, uint8_t* out48, uint8_t* out_xy, uint8_t* value, uint8_t* status,
                         hipStream_t st);

}  // namespace vrf
