"""Time of the per-item G1 linear combinations on the device (vrfhip_g1_lincomb_batch_dev): hip events around the _dev
call, one warm-up, then the median of 5 calls.  Shapes: (k, m) = (8, 4) at n = 2^14 and 2^18 (the A_i of a KZG opening), (2, 0)
at 2^14 (the B_i).  Then the baseline at n = 256, (k, m) = (12, 0): one lincomb call against 256 sequential
vrfhip_g1_msm_dev calls of 12 points each -- the only way to compute the same sums without this entry point.  The kernel has
no per-lane control flow, so a batch tiles 64 distinct (base, scalar) pairs; the results are checked against the C oracle on
the first items.  One run, under a time limit:
usage: timeout 600 python tools/gpu_g1_lincomb_time.py"""
import os, random, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from ark_ec_vrfs_amd import Context, _lib
from oracle import bls_oracle as bls
from oracle import c_oracle as co

rnd = random.Random(21)
G = bls.G1[0].to_bytes(48, "little") + bls.G1[1].to_bytes(48, "little")
PTS = [co.g1_mul(rnd.randrange(1, bls.R), G) for _ in range(64)]
SCS = [rnd.randrange(bls.R) for _ in range(64)]
ctx = Context(0)


def tiled(n, k, m):
    """device arrays of n items whose term (i, j) is pair (i * (k + m) + j) mod 64 (shared bases: pairs 0 .. m - 1)"""
    idx = (np.arange(n)[:, None] * (k + m) + np.arange(k + m)[None, :]) % 64
    pts = np.frombuffer(b"".join(PTS), np.uint8).reshape(64, 96)
    scs = np.frombuffer(b"".join(s.to_bytes(32, "little") for s in SCS), np.uint8).reshape(64, 32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    b = dev(pts[idx[:, :k]]) if k else None
    s = dev(scs[idx[:, :k]]) if k else None
    sb = dev(pts[:m]) if m else None
    ss = dev(scs[idx[:, k:]]) if m else None
    return idx, b, s, sb, ss


def oracle_item(idx_row, k, m):
    acc = bytes(96)
    for j, t in enumerate(idx_row):
        acc = co.g1_add(acc, co.g1_mul(SCS[t], PTS[t] if j < k else PTS[j - k]))
    return acc


def timed(name, n, call, unit="items"):
    call(); torch.cuda.synchronize()
    ms = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record(); torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    med = statistics.median(ms)
    print(f"{name:44s} n={n:7d}: median {med:9.3f} ms  (min {min(ms):.3f}, max {max(ms):.3f})  {n / med * 1e3:.3e} {unit}/s",
          flush=True)
    return med


def lincomb_case(n, k, m):
    idx, b, s, sb, ss = tiled(n, k, m)
    out = torch.empty((n, 96), dtype=torch.uint8, device="cuda")
    st = torch.empty(n, dtype=torch.uint8, device="cuda")
    med = timed(f"lincomb (k, m) = ({k}, {m})", n, lambda: ctx.g1_lincomb_batch_dev(b, s, sb, ss, out, st))
    assert not bool(st.any()), "invalid items"
    head = out[:3].cpu().numpy()
    assert [bytes(r) for r in head] == [oracle_item(idx[i], k, m) for i in range(3)], "lincomb differs from the oracle"
    return med, (idx, b, s, out)


t_a14, _ = lincomb_case(1 << 14, 8, 4)
lincomb_case(1 << 18, 8, 4)
t_b14, _ = lincomb_case(1 << 14, 2, 0)
print(f"A_i + B_i at 2^14: {t_a14 + t_b14:.3f} ms", flush=True)

# the baseline: the same 256 sums of 12 terms by the entry point that existed before, one call per item
n, k = 256, 12
t_lc, (idx, b, s, out) = lincomb_case(n, k, 0)
lib, h = _lib.load(), ctx._h
msm_out = torch.empty((n, 96), dtype=torch.uint8, device="cuda")
msm_st = torch.empty(n, dtype=torch.uint8, device="cuda")
stream = torch.cuda.current_stream().cuda_stream
bp, sp, op, tp = b.data_ptr(), s.data_ptr(), msm_out.data_ptr(), msm_st.data_ptr()


def msm_loop():
    for i in range(n):
        _lib.check(lib.vrfhip_g1_msm_dev(h, k, bp + i * k * 96, sp + i * k * 32, op + i * 96, tp + i, stream), "vrfhip_g1_msm_dev")


t_msm = timed(f"{n} x vrfhip_g1_msm_dev of {k} points", n, msm_loop)
assert bool((msm_out == out).all()) and not bool(msm_st.any()), "the MSM loop and lincomb disagree"
print(f"lincomb is {t_msm / t_lc:.1f} x the speed of {n} sequential MSM calls ({t_msm:.3f} ms / {t_lc:.3f} ms)")
ctx.close()
