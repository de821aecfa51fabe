"""Per-proof Pedersen verification at 2^20: compressed encodings vs affine x || y inputs, with the checked decode and with
VRFHIP_FLAG_PREVALIDATED_ALL, on JubJub, bandersnatch_sw and secp256r1 (device-pointer forms, device events, warm-up, then
alternating repetitions; median reported), plus the per-stage split of one call of each (vrfhip_ctx_profile).  Then the IETF
multi-context host entry points on one Bandersnatch context at 2^20: vrfhip_ietf_verify_batch_multi vs its x || y form.
The statuses of both forms are compared on every timed batch.  Prints one JSON line per measurement."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from ark_ec_vrfs_amd import (BandersnatchSha512Ell2, BandersnatchSwSha512Tai, Context, JubJubSha512Tai, Secp256r1Sha256Tai, _lib,
                             ietf_verify_batch_affine_multi, ietf_verify_batch_multi)

LOGN = int(os.environ.get("AFFINE_TIME_LOGN", "20"))
REPS = 5
dev = torch.device("cuda:0")
lib = _lib.load()


def cur():
    return torch.cuda.current_stream().cuda_stream


def make_proofs(ctx, n):
    """(compressed points, affine points, s, sb) of n Pedersen proofs made on the device; every 1000th s tampered."""
    seeds = torch.arange(n, dtype=torch.int64, device=dev).view(torch.uint8).reshape(n, 8)
    sk = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    _lib.check(lib.vrfhip_secret_from_seed_batch_dev(ctx.handle, n, seeds.data_ptr(), 8, sk.data_ptr(), None, cur()), "seed")
    msg = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    pw = ctx.point_bytes()
    res = {}
    for flags, w in ((0, pw), (ctx.PROVE_POINTS_AFFINE, 64)):
        ctx.set_flags(flags)
        mk = lambda width: torch.empty((n, width), dtype=torch.uint8, device=dev)
        out, pkc, r, ok, s, sb, hh = mk(w), mk(w), mk(w), mk(w), mk(32), mk(32), mk(pw)
        st = torch.empty(n, dtype=torch.uint8, device=dev)
        ctx.pedersen_prove_batch_dev(sk, msg, 32, out, pkc, r, ok, s, sb, None, hh, st)
        torch.cuda.synchronize()
        assert int(st.sum()) == 0
        res[flags] = (hh, out, pkc, r, ok, s, sb)
    ctx.set_flags(0)
    hh = res[0][0]
    h_xy = torch.empty((n, 64), dtype=torch.uint8, device=dev)
    vst = torch.empty(n, dtype=torch.uint8, device=dev)
    _lib.check(lib.vrfhip_point_validate_batch_dev(ctx.handle, n, hh.data_ptr(), h_xy.data_ptr(), vst.data_ptr(), cur()), "validate")
    torch.cuda.synchronize()
    assert int(vst.sum()) == 0
    comp = list(res[0][:5])
    aff = [h_xy] + list(res[ctx.PROVE_POINTS_AFFINE][1:5])
    s, sb = res[0][5].clone(), res[0][6]
    s[::1000, 1] ^= 2
    return comp, aff, s, sb


def time_call(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stages(ctx, fn):
    ctx.profile(True)
    fn()
    torch.cuda.synchronize()
    ms, launches = ctx.profile_read()
    ctx.profile(False)
    return [round(m, 3) for m in ms]


def pedersen(suite, name):
    desc_kw = {} if suite is BandersnatchSha512Ell2 else {"test_blinding_base": True}
    ctx = Context(0, suite, **desc_kw)
    n = 1 << LOGN
    comp, aff, s, sb = make_proofs(ctx, n)
    st_c = torch.empty(n, dtype=torch.uint8, device=dev)
    st_a = torch.empty(n, dtype=torch.uint8, device=dev)
    run_c = lambda: ctx.pedersen_verify_batch_dev(*comp, s, sb, st_c)
    run_a = lambda: ctx.pedersen_verify_batch_affine_dev(*aff, s, sb, st_a)
    for mode, flags in (("checked", 0), ("prevalidated", ctx.PREVALIDATED_ALL)):
        ctx.set_flags(flags)
        for f in (run_c, run_a):
            f()
        torch.cuda.synchronize()
        tc, ta = [], []
        for _ in range(REPS):
            tc.append(time_call(run_c))
            ta.append(time_call(run_a))
        sc, sa = st_c.cpu().numpy(), st_a.cpu().numpy()
        assert (sc == sa).all(), (name, mode, np.nonzero(sc != sa)[0][:10])
        assert int((sc != 0).sum()) == len(range(0, n, 1000))
        print(json.dumps({"suite": name, "n": n, "mode": mode,
                          "compressed_ms": round(statistics.median(tc), 3), "affine_ms": round(statistics.median(ta), 3),
                          "compressed_stages_ms": stages(ctx, run_c), "affine_stages_ms": stages(ctx, run_a),
                          "stage_names": ["decode", "straus_0", "straus_1", "finish"], "statuses_equal": True}), flush=True)
    ctx.close()


def ietf_multi():
    ctx = Context(0, BandersnatchSha512Ell2)
    n = 1 << LOGN
    seeds = torch.arange(n, dtype=torch.int64, device=dev).view(torch.uint8).reshape(n, 8)
    sk = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    _lib.check(lib.vrfhip_secret_from_seed_batch_dev(ctx.handle, n, seeds.data_ptr(), 8, sk.data_ptr(), None, cur()), "seed")
    msg = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    outs = {}
    for flags, w in ((0, 32), (ctx.PROVE_POINTS_AFFINE, 64)):
        ctx.set_flags(flags)
        mk = lambda width: torch.empty((n, width), dtype=torch.uint8, device=dev)
        out, c, s, pk, hh = mk(w), mk(32), mk(32), mk(w), mk(32)
        st = torch.empty(n, dtype=torch.uint8, device=dev)
        ctx.ietf_prove_batch_dev(sk, msg, 32, out, c, s, pk_out=pk, input_out=hh, status=st)
        torch.cuda.synchronize()
        assert int(st.sum()) == 0
        outs[flags] = [t.cpu().numpy() for t in (pk, hh, out, c, s)]
    ctx.set_flags(0)
    pk, hh, out, c, s = outs[0]
    vst, h_xy = ctx.point_validate_batch(hh, want_xy=True)
    assert (vst == 0).all()
    pk_xy, _, out_xy, _, _ = outs[ctx.PROVE_POINTS_AFFINE]
    s = s.copy()
    s[::1000, 1] ^= 2
    run_c = lambda: ietf_verify_batch_multi([ctx], pk, hh, out, c, s)
    run_a = lambda: ietf_verify_batch_affine_multi([ctx], pk_xy, h_xy, out_xy, c, s)
    run_c(); run_a()
    tc, ta = [], []
    for _ in range(REPS):
        t = time.perf_counter(); sc = run_c(); tc.append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter(); sa = run_a(); ta.append((time.perf_counter() - t) * 1e3)
    assert (sc == sa).all() and int((sc != 0).sum()) == len(range(0, n, 1000))
    print(json.dumps({"suite": "bandersnatch", "n": n, "call": "ietf_verify_batch_multi (1 ctx, host arrays, wall clock)",
                      "compressed_ms": round(statistics.median(tc), 3), "affine_ms": round(statistics.median(ta), 3),
                      "statuses_equal": True}), flush=True)
    ctx.close()


if __name__ == "__main__":
    for suite, name in ((JubJubSha512Tai, "jubjub"), (BandersnatchSwSha512Tai, "bandersnatch_sw"), (Secp256r1Sha256Tai, "secp256r1")):
        pedersen(suite, name)
    ietf_multi()
