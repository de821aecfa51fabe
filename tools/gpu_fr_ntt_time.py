"""Time of the radix-2 transforms over Fr on the device (vrfhip_fr_ntt_batch_dev, forward and inverse, plain domain and the
coset of GENERATOR) and of commitments and openings from evaluations (vrfhip_kzg_commit_evals_batch_dev,
vrfhip_kzg_open_evals_batch_dev), beside what they feed: vrfhip_kzg_commit_batch_dev / vrfhip_kzg_open_batch_dev of this tree
and of the PARENT commit's library, loaded into the same process.  What matters is the share of a commitment from evaluations
that the transform takes.
Per shape every call is warmed up once, then ROUNDS timed rounds alternate over all calls; a timed window is REPS back-to-back
calls between two hip events (one transform of 2^11 lasts some ten microseconds), reported per call.  Per call: median, min,
max and spread = (max - min) / median over the rounds.  Inputs are resident in HBM.  The bytes a transform moves are counted
from the shape: every pass reads and writes the columns once (64 B per scalar) and reads one 36-byte twiddle per butterfly
with a non-trivial twiddle and per inter-pass product; `GBps_counted` is that sum over the median time of the whole call.
Bases: 2^16 distinct points [j + 1] G from the oracle's additions, tiled for 2^20 as tools/gpu_kzg_commit_time.py does.
One JSON line per shape on stdout.
usage: timeout 900 python tools/gpu_fr_ntt_time.py PARENT/libvrfhip.so [k:log2n ...]      default 8:11 8:16 1:20"""
import ctypes, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from ark_ec_vrfs_amd import Context
from oracle import bls_oracle as bls
from oracle import c_oracle as co

ROUNDS = 7
parent_path = sys.argv[1]
shapes = [tuple(int(x) for x in a.split(":")) for a in sys.argv[2:]] or [(8, 11), (8, 16), (1, 20)]
w48 = lambda x: int(x).to_bytes(48, "little")
G96 = w48(bls.G1[0]) + w48(bls.G1[1])

ctx = Context(0)
old = ctypes.CDLL(os.path.abspath(parent_path))
V, Z = ctypes.c_void_p, ctypes.c_size_t
old.vrfhip_ctx_create.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(V)]
old.vrfhip_g1_srs_create.argtypes = [V, Z, V, V, ctypes.POINTER(V)]
old.vrfhip_g1_srs_destroy.argtypes = [V]
old.vrfhip_g1_srs_destroy.restype = None
old.vrfhip_kzg_commit_batch_dev.argtypes = [V, V, Z, Z, Z, V, V, V, V, V]
old.vrfhip_kzg_open_batch_dev.argtypes = [V, V, Z, Z, V, V, V, V, V, V, V]
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
enc_small, st = ctx.g1_encode_batch(np.frombuffer(b"".join(pts), np.uint8).reshape(DISTINCT, 96))
assert not st.any()
rng = np.random.default_rng(11)
u8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, device="cuda")


def window(call, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def stats(t):
    m = statistics.median(t)
    return {"median_ms": round(m, 5), "min_ms": round(min(t), 5), "max_ms": round(max(t), 5), "spread": round((max(t) - min(t)) / m, 4)}


def counted_bytes(k, lg, passes, coset):
    """columns in and out per pass, one twiddle per butterfly of all but each pass's last stage, one per inter-pass product,
    one coset factor per scalar"""
    n = 1 << lg
    per_pass = lg / passes
    tw = (n // 2) * (lg - passes) + n * (passes - 1) + (n if coset else 0)
    return k * (passes * n * 64 + tw * 36), per_pass


for k, lg in shapes:
    n = 1 << lg
    reps_tile = (n + DISTINCT - 1) // DISTINCT
    enc = np.tile(enc_small, (reps_tile, 1))[:n]
    srs = ctx.g1_srs_create(enc)
    old_srs = V()
    assert old.vrfhip_g1_srs_create(old_ctx, n, enc.ctypes.data, None, ctypes.byref(old_srs)) == 0
    dom, cos = ctx.fr_domain_create(lg), ctx.fr_domain_create(lg, 7)
    passes = ctx.fr_ntt_passes(lg)
    sc = rng.integers(0, 256, (k, n, 32), dtype=np.uint8)
    sc[:, :, 31] &= 0x3F                                        # < 2^254 < r
    d_sc = torch.from_numpy(sc).cuda()
    d_z = torch.from_numpy(sc[:, 0, :].copy()).cuda()
    d_out, d_co, st_n = u8(k, n, 32), u8(k, n, 32), u8(k)
    o48, st_c, val, p48, st_o = u8(k, 48), u8(k), u8(k, 32), u8(k, 48), u8(k)
    b48, st_b, bval, bp48, st_bo = u8(k, 48), u8(k), u8(k, 32), u8(k, 48), u8(k)
    stream = torch.cuda.current_stream().cuda_stream
    ctx.fr_ntt_batch_dev(dom, d_sc, d_co, st_n, inverse=True)   # the coefficients the plain calls get
    torch.cuda.synchronize()

    def parent_commit():
        assert old.vrfhip_kzg_commit_batch_dev(old_ctx, old_srs, k, n, 0, d_co.data_ptr(), b48.data_ptr(), None, st_b.data_ptr(), stream) == 0

    def parent_open():
        assert old.vrfhip_kzg_open_batch_dev(old_ctx, old_srs, k, n, d_co.data_ptr(), d_z.data_ptr(), bval.data_ptr(), bp48.data_ptr(),
                                             None, st_bo.data_ptr(), stream) == 0

    calls = {
        "ntt_forward": lambda: ctx.fr_ntt_batch_dev(dom, d_sc, d_out, st_n),
        "ntt_inverse": lambda: ctx.fr_ntt_batch_dev(dom, d_sc, d_out, st_n, inverse=True),
        "ntt_coset_forward": lambda: ctx.fr_ntt_batch_dev(cos, d_sc, d_out, st_n),
        "ntt_coset_inverse": lambda: ctx.fr_ntt_batch_dev(cos, d_sc, d_out, st_n, inverse=True),
        "commit_evals": lambda: ctx.kzg_commit_evals_batch_dev(srs, dom, d_sc, o48, st_c),
        "open_evals": lambda: ctx.kzg_open_evals_batch_dev(srs, dom, d_sc, d_z, val, p48, st_o),
        "commit_coeffs": lambda: ctx.kzg_commit_batch_dev(srs, d_co, o48, st_c),
        "open_coeffs": lambda: ctx.kzg_open_batch_dev(srs, d_co, d_z, val, p48, st_o),
        "parent_commit_coeffs": parent_commit,
        "parent_open_coeffs": parent_open,
    }
    reps = {name: (max(1, (1 << 21) // (k * n)) if name.startswith("ntt") else 1 if lg >= 16 else 4) for name in calls}
    times = {name: [] for name in calls}
    for name, call in calls.items():
        window(call, 1)
    for _ in range(ROUNDS):
        for name, call in calls.items():
            times[name].append(window(call, reps[name]))
    # the evals forms and the parent's coefficient forms must give the same bytes
    calls["commit_evals"](); calls["open_evals"](); parent_commit(); parent_open(); torch.cuda.synchronize()
    equal = bool((o48.cpu() == b48.cpu()).all() and (val.cpu() == bval.cpu()).all() and (p48.cpu() == bp48.cpu()).all())
    assert equal and not st_c.cpu().numpy().any() and not st_o.cpu().numpy().any() and not st_b.cpu().numpy().any()
    res = {name: stats(t) for name, t in times.items()}
    med = lambda name: res[name]["median_ms"]
    by_plain, _ = counted_bytes(k, lg, passes, False)
    by_coset, _ = counted_bytes(k, lg, passes, True)
    print(json.dumps({
        "shape": {"k": k, "log_n": lg}, "passes": passes, "rounds": ROUNDS, "calls_per_window": reps, **res,
        "ntt_inverse_share_of_commit_evals": round(med("ntt_inverse") / med("commit_evals"), 4),
        "ntt_inverse_share_of_open_evals": round(med("ntt_inverse") / med("open_evals"), 4),
        "commit_evals_minus_parent_commit_ms": round(med("commit_evals") - med("parent_commit_coeffs"), 5),
        "open_evals_minus_parent_open_ms": round(med("open_evals") - med("parent_open_coeffs"), 5),
        "counted_bytes_forward": by_plain, "counted_bytes_coset_forward": by_coset,
        "GBps_counted_forward": round(by_plain / med("ntt_forward") / 1e6, 1),
        "butterflies": k * (n // 2) * lg,
        "butterflies_per_us_forward": round(k * (n // 2) * lg / med("ntt_forward") / 1e3, 1),
        "results_equal": equal}), flush=True)
    dom.close(); cos.close(); srs.close()
    old.vrfhip_g1_srs_destroy(old_srs)
    del d_sc, d_co, d_out
old.vrfhip_ctx_destroy(old_ctx)
ctx.close()
