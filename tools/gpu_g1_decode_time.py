"""Time of the BLS12-381 G1 codec on the device: decode (subgroup test on / off), validate, encode, 2^20 points per call,
hip events around the _dev call, one warm-up, then the median of 5 calls.  The kernels have no per-lane control flow, so the
batch tiles 64 distinct subgroup points (both sort flags).  One run, under a time limit:
usage: timeout 300 python tools/gpu_g1_decode_time.py [log2 n, default 20]"""
import os, random, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from ark_ec_vrfs_amd import Context
from oracle import bls_oracle as bls

n = 1 << (int(sys.argv[1]) if len(sys.argv) > 1 else 20)
rnd = random.Random(20)
acc, encs = bls.g1_mul(rnd.randrange(1, bls.R), bls.G1), []
for i in range(64):
    acc = bls.g1_add(acc, bls.G1)
    pt = acc if i & 1 else bls.g1_neg(acc)
    b = bytearray(pt[0].to_bytes(48, "big"))
    b[0] |= 0x80 | (0x20 if pt[1] > bls.P - pt[1] else 0)
    encs.append(bytes(b))
ctx = Context(0)
comp = torch.from_numpy(np.frombuffer(b"".join(encs), np.uint8).reshape(64, 48).copy()).cuda().repeat(n // 64, 1).contiguous()
xy = torch.empty((n, 96), dtype=torch.uint8, device="cuda")
back = torch.empty((n, 48), dtype=torch.uint8, device="cuda")
st = torch.empty(n, dtype=torch.uint8, device="cuda")


def timed(name, call):
    call(); torch.cuda.synchronize()
    ms = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record(); torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    med = statistics.median(ms)
    print(f"{name:28s} n={n}: median {med:9.3f} ms  (min {min(ms):.3f}, max {max(ms):.3f})  {n / med * 1e3:.3e} points/s  "
          f"invalid={int((st != 0).sum())}", flush=True)
    return med


t_on = timed("decode, subgroup test on", lambda: ctx.g1_decode_batch_dev(comp, xy, st, check_subgroup=True))
t_off = timed("decode, subgroup test off", lambda: ctx.g1_decode_batch_dev(comp, xy, st, check_subgroup=False))
t_val = timed("validate", lambda: ctx.g1_validate_batch_dev(xy, st))
t_enc = timed("encode", lambda: ctx.g1_encode_batch_dev(xy, back, st))
assert bool((back == comp).all()), "encode o decode is not the identity"
print(f"decode off < decode on: {t_off < t_on};  validate <= decode on: {t_val <= t_on}")
ctx.close()
