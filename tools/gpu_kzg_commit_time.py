"""Time of KZG commitments and openings over a resident base set on the device (vrfhip_kzg_commit_batch_dev,
vrfhip_kzg_open_batch_dev) against what committed k columns before: k calls of vrfhip_g1_msm_dev on one stream, taken from
the PARENT commit's library, which re-reads, converts and curve-tests the 96-byte bases in every call.
Both libraries are loaded into one process and alternate: per shape one warm-up each, then ROUNDS timed rounds (a) (b) (a) (b)
..., hip events around the calls, inputs resident in HBM.  Reported per shape: median, min and max of each, and the spread of
each = (max - min) / median over the rounds of the same code -- the yardstick: (a) counts as slower than (b) only if
median(a) - median(b) exceeds the larger spread.  The results of (a) and (b) must be equal.
  (a) one vrfhip_kzg_commit_batch_dev over (k, len);
  (b) k x vrfhip_g1_msm_dev(len) of the parent library.
Openings have nothing to be compared with: one vrfhip_kzg_open_batch_dev per shape, the call and its stages from the context's
profiling events: quotient | buckets | final | encode (the wipe of the workspace is the rest of the call).  The stages of the
commitment are reported the same way (prep | buckets | final | encode).
Bases: 2^16 distinct points [j + 1] G from the oracle's additions, compressed by vrfhip_g1_encode_batch, tiled for len = 2^20
(the scalars differ per index, so the bucket loads are those of distinct terms).  One JSON line per shape on stdout.
usage: timeout 900 python tools/gpu_kzg_commit_time.py PARENT/libvrfhip.so [k:log2len ...]      default 3:11 8:16 1:20"""
import ctypes, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from ark_ec_vrfs_amd import Context
from oracle import bls_oracle as bls
from oracle import c_oracle as co

ROUNDS = 7
parent_path = sys.argv[1]
shapes = [tuple(int(x) for x in a.split(":")) for a in sys.argv[2:]] or [(3, 11), (8, 16), (1, 20)]
w48 = lambda x: int(x).to_bytes(48, "little")
G96 = w48(bls.G1[0]) + w48(bls.G1[1])

ctx = Context(0)
# the parent library: its own context, raw ctypes (the binding of this tree belongs to this tree's library)
old = ctypes.CDLL(os.path.abspath(parent_path))
V, Z = ctypes.c_void_p, ctypes.c_size_t
old.vrfhip_ctx_create.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(V)]
old.vrfhip_g1_msm_dev.argtypes = [V, Z, V, V, V, V, V]
old.vrfhip_ctx_destroy.argtypes = [V]
old.vrfhip_ctx_destroy.restype = None
old_ctx = V()
assert old.vrfhip_ctx_create(ctx.suite.SUITE_ENUM, 0, ctypes.byref(old_ctx)) == 0
assert old.vrfhip_abi_version() == ctx._lib.vrfhip_abi_version()

DISTINCT = 1 << 16
pts, acc = [], G96
for _ in range(DISTINCT):
    pts.append(acc)
    acc = co.g1_add(acc, G96)
xy_small = np.frombuffer(b"".join(pts), np.uint8).reshape(DISTINCT, 96)
enc_small, st = ctx.g1_encode_batch(xy_small)
assert not st.any()
rng = np.random.default_rng(7)
u8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, device="cuda")


def once(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); call(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(t):
    m = statistics.median(t)
    return {"median_ms": round(m, 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4), "spread": round((max(t) - min(t)) / m, 4)}


def staged(call):
    ctx.profile(True)
    total = once(call)
    ms, groups = ctx.profile_read()
    ctx.profile(False)
    return total, [round(x, 4) for x in ms], groups


for k, lg in shapes:
    n = 1 << lg
    reps = (n + DISTINCT - 1) // DISTINCT
    xy = np.tile(xy_small, (reps, 1))[:n]
    srs = ctx.g1_srs_create(np.tile(enc_small, (reps, 1))[:n])
    d_xy = torch.from_numpy(np.ascontiguousarray(xy)).cuda()
    sc = rng.integers(0, 256, (k, n, 32), dtype=np.uint8)
    sc[:, :, 31] &= 0x3F                                        # < 2^254 < r
    d_sc = torch.from_numpy(sc).cuda()
    d_z = torch.from_numpy(sc[:, 0, :].copy()).cuda()
    out48, out_xy, st_a = u8(k, 48), u8(k, 96), u8(k)
    out_b, st_b = u8(k, 96), u8(k)
    val, pr48, st_o = u8(k, 32), u8(k, 48), u8(k)
    stream = torch.cuda.current_stream().cuda_stream

    def call_a():
        ctx.kzg_commit_batch_dev(srs, d_sc, out48, st_a, out_xy=out_xy)

    def call_b():
        for c in range(k):
            rc = old.vrfhip_g1_msm_dev(old_ctx, n, d_xy.data_ptr(), d_sc[c].data_ptr(), out_b[c].data_ptr(), st_b[c:].data_ptr(), stream)
            assert rc == 0

    def call_o():
        ctx.kzg_open_batch_dev(srs, d_sc, d_z, val, pr48, st_o)

    once(call_a); once(call_b); once(call_o)
    ta, tb, to = [], [], []
    for _ in range(ROUNDS):
        ta.append(once(call_a)); tb.append(once(call_b)); to.append(once(call_o))
    assert not st_a.cpu().numpy().any() and not st_b.cpu().numpy().any() and not st_o.cpu().numpy().any(), "invalid input"
    assert (out_xy.cpu().numpy() == out_b.cpu().numpy()).all(), "(a) and (b) disagree"
    a, b, o = stats(ta), stats(tb), stats(to)
    bar = max(a["spread"], b["spread"]) * b["median_ms"]
    tot_c, st_c, g_c = staged(call_a)
    tot_o, st_op, g_o = staged(call_o)
    print(json.dumps({
        "shape": {"k": k, "len": n}, "rounds": ROUNDS,
        "commit_batch_dev": a, "parent_g1_msm_dev_x_k": b, "b_over_a": round(b["median_ms"] / a["median_ms"], 3),
        "a_minus_b_ms": round(a["median_ms"] - b["median_ms"], 4), "spread_bar_ms": round(bar, 4),
        "a_slower_beyond_spread": a["median_ms"] - b["median_ms"] > bar,
        "commit_stages_ms": {"call": round(tot_c, 4), "prep": st_c[0], "buckets": st_c[1], "final": st_c[2], "encode": st_c[3],
                             "launch_groups": g_c},
        "open_batch_dev": o,
        "open_stages_ms": {"call": round(tot_o, 4), "quotient": st_op[0], "buckets": st_op[1], "final": st_op[2],
                           "encode": st_op[3], "launch_groups": g_o},
        "results_equal": True}), flush=True)
    srs.close()
    del d_xy, d_sc
old.vrfhip_ctx_destroy(old_ctx)
ctx.close()
