// launchers.inc -- the launch interface of ONE base field's kernel objects (field.h).  Included by kernels.h inside the
// field's inline namespace, and by api.hip once per field namespace, so that the C ABI can reach the three builds.
// launchers (each defined next to its kernels)
// generator tables: GCOMB_WORDS words each; prefix: 2 * GC_ROWS * GC_SEGS * GC_SEG * 9 words of build scratch.
// gb_xy (device, 128 B): the descriptor's generator and blinding base, x || y little-endian; mont (device, 36 words)
// receives their Montgomery coordinates, flags (device, 2 B) 1 = valid point of the prime-order subgroup.
void launch_init_tables(int suite, uint32_t* g_win, uint32_t* g_comb, uint32_t* b_comb, uint32_t* prefix,
                        const uint8_t* gb_xy, uint32_t* mont, uint8_t* flags, SqrtTables T, hipStream_t st);
// ev: optional 5 events recorded on `st` before stage 1 and after stages 1, 2a, 2b, 3 (profiling)
void launch_ietf_verify(const VerifyArgs& a, hipStream_t st, hipEvent_t* ev = nullptr);
void launch_verify_input_from_alpha(int suite, size_t n, BytesView msg, uint8_t* enc, uint32_t* tabs, DevTables T,
                                    hipStream_t st, uint8_t* tai_ctr = nullptr, unsigned long long* queue = nullptr);
void launch_ietf_prove(const ProveArgs& a, hipStream_t st, hipEvent_t* ev = nullptr);
void launch_pedersen_verify(const PedersenVerifyArgs& a, hipStream_t st, hipEvent_t* ev = nullptr);
void launch_hash_to_curve(int suite, size_t n, BytesView msg, uint8_t* points, DevTables T, hipStream_t st,
                          uint8_t* tai_ctr = nullptr, unsigned long long* queue = nullptr);
void launch_output_hash(int suite, size_t n, const uint8_t* gamma, uint8_t* hash, DevTables T, hipStream_t st);
void launch_secret_from_seed(int suite, size_t n, const uint8_t* seeds, uint32_t seed_len, uint8_t* sk,
                             uint8_t* pk, DevTables T, hipStream_t st);
// key sets: decode + validate the keys (xy: [n][18] Montgomery words), then build one comb per key.
// prefix: [n_keys * 32][255][9] words of scratch for the build.
void launch_keyset_build(int suite, size_t n_keys, const uint8_t* pks, uint32_t* xy, uint8_t* valid, uint32_t* combs,
                         uint32_t* prefix, DevTables T, hipStream_t st);
void launch_point_validate(int suite, size_t n, const uint8_t* pts, uint8_t* xy, uint8_t* status,
                           uint32_t* tabs, DevTables T, hipStream_t st);
// MSM: ws must hold msm_workspace_bytes(n, groups) bytes; groups = msm_groups(n, n, #CUs)  (msm.cuh)
void launch_msm(int suite, size_t n, const uint8_t* xy, const uint8_t* scalars, uint8_t* out_enc,
                uint8_t* out_xy, uint8_t* status, void* ws, int groups, hipStream_t st);
void launch_fq_mul(size_t n, const uint8_t* a, const uint8_t* b, uint8_t* r, hipStream_t st);
// test primitives: group law, variable-base scalar multiplication (tabs: 2 * WIN_TABLE_WORDS words per item), hashes
void launch_test_point_add(int suite, size_t n, const uint8_t* a, const uint8_t* b, uint8_t* out, uint8_t* status,
                           DevTables T, hipStream_t st);
void launch_test_scalar_mul(int suite, size_t n, const uint8_t* k, const uint8_t* p, uint8_t* out, uint8_t* status,
                            uint32_t* tabs, DevTables T, hipStream_t st);
// the verifier's U and V as the ladders left them in a.ws.pts (launch_ietf_verify with a.u_out set runs this in place of its
// finish stage): one inversion, te_encode_affine with the suite's flags -> a.u_out, a.v_out, a.status
void launch_test_verify_uv_readout(const VerifyArgs& a, hipStream_t st);
void launch_test_hash(int suite, size_t n, BytesView msg, uint8_t* out, int which, DevTables T, hipStream_t st);
// host copies of the field's square-root tables and the built-in descriptor points (constants*.gen.h), for the C ABI
const uint32_t* field_sqrt_p(size_t* bytes);
const uint8_t* field_sqrt_lut(size_t* bytes);
// suite: SUITE_* (vrf_types.h); g_xy / b_xy receive the default generator and Pedersen blinding base (x || y, 32-byte LE)
bool field_default_points(int suite, uint8_t g_xy[64], uint8_t b_xy[64]);
// ---- MSM on the VRF curves and the batched Pedersen verifier (msm.cuh, k_msm.hip, k_rlc.hip) ----
// buckets + final over prepared points / digits.  out_enc: 32 B compressed sum (nullable); out_xy: 64 B
// affine (nullable); status: 1 byte (nullable; 0 ok, 2 if flags[0] is set); fail_flag: 1 byte (nullable),
// set to 1 unless the sum is the neutral element (never cleared here: callers OR several MSMs into it).
// ev (nullable): ev[0] recorded after the bucket kernel, ev[1] and ev[2] after the final kernel.
void launch_msm_core(int suite, const MsmLayout& L, uint8_t* out_enc, uint8_t* out_xy, uint8_t* status,
                     uint8_t* fail_flag, hipStream_t st, hipEvent_t* ev = nullptr);

// enqueues decode + MSM; fail_flag[0] becomes 1 if the batch equation does not hold.
// ev (nullable, 5 events): start | decode | buckets | final | final.
void launch_pedersen_rlc(const RlcArgs& a, uint8_t* fail_flag, hipStream_t st, hipEvent_t* ev = nullptr);
// n x 64 B affine x || y -> n x 32 B compressed encodings
void launch_affine_compress(size_t n, const uint8_t* xy, uint8_t* enc, uint32_t sflags, hipStream_t st);
// VRFHIP_FLAG_COORDS_MONT256: k_msm.hip takes the bases in Montgomery-256 form; k_misc.hip converts x || y outputs in place
void launch_msm_coords(int suite, size_t n, const uint8_t* xy, const uint8_t* scalars, uint8_t* out_enc, uint8_t* out_xy,
                       uint8_t* status, void* ws, int groups, int mont256, uint32_t sflags, hipStream_t st);
void launch_xy_to_mont256(size_t n, uint8_t* xy, hipStream_t st);
void launch_xy_from_mont256(size_t n, uint8_t* xy, hipStream_t st);
