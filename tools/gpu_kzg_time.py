"""Time of the batched KZG opening check on the device (vrfhip_kzg_check_batch_rlc_dev) against the chain of calls that
computes the same verdict without it.  Inputs resident in HBM, hip events around the calls, one warm-up each, then 5 timed
rounds in which the two alternate; medians.
  (a) vrfhip_kzg_check_batch_rlc_dev on (C_i, z_i, v_i, pi_i) as they come from the wire;
  (b) two vrfhip_g1_decode_batch_dev calls over the 2n points [C_i, -pi_i], the bases of the linear combination, n points
      each (the caller negates pi_i by flipping the sort flag of the encoding, on the host and not timed), a strided copy of
      the decoded -pi_i into the B half of the item array, vrfhip_g1_lincomb_batch_dev (k = 2, m = 1):
      A_i = 1 C_i + (r - z_i)(-pi_i) + (r - v_i) g, written into the A half, and vrfhip_pairing_check_batch_rlc_dev.  The
      scalar rows are prepared beforehand and left out of the timing.  Every point is decoded once, as in (a).
  (b1) the same chain with ONE decode call over all 2n points, which the interleaved layout of the bases allows: one launch
      less, which counts where a launch is all latency.
The items are honest openings under a toy secret, 64 distinct ones tiled over the batch (the weights differ per index, so the
bucket loads are those of distinct items).  The statuses and verdicts of (a) and (b) must agree.  The stages of (a) come from
the context's profiling events: decode | digest, prep, fold | buckets | final, combine; the pairing is the rest of the call.
One size per run, each run under its own time limit:
usage: timeout 300 python tools/gpu_kzg_time.py 14 && timeout 600 python tools/gpu_kzg_time.py 18"""
import os, random, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from ark_ec_vrfs_amd import Context
from oracle import bls_oracle as bls
from oracle import c_oracle as co

P, R = bls.P, bls.R
log2n = int(sys.argv[1]) if len(sys.argv) > 1 else 14
n = 1 << log2n
rnd = random.Random(31)
w48 = lambda x: int(x).to_bytes(48, "little")
le32 = lambda x: int(x).to_bytes(32, "little")
TAU = rnd.randrange(1, R)
G = co.g1_mul(rnd.randrange(1, R), w48(bls.G1[0]) + w48(bls.G1[1]))
H = b"".join(w48(x) for x in (bls.G2[0].a, bls.G2[0].b, bls.G2[1].a, bls.G2[1].b))
VK = G + H + co.g2_mul(TAU, H)


def compress(b96, negate=False):
    x, y = int.from_bytes(b96[:48], "little"), int.from_bytes(b96[48:], "little")
    if negate:
        y = P - y
    out = bytearray(x.to_bytes(48, "big"))
    out[0] |= 0x80 | (0x20 if y > P - y else 0)
    return bytes(out)


rows = []
for _ in range(64):
    c, p, z = rnd.randrange(1, R), rnd.randrange(1, R), rnd.randrange(R)
    C, PI = co.g1_mul(c, G), co.g1_mul(p, G)
    rows.append((compress(C), z, (c - p * (TAU - z)) % R, compress(PI), compress(PI, negate=True)))
idx = np.arange(n) % 64
col = lambda f, w: np.frombuffer(b"".join(f(r) for r in rows), np.uint8).reshape(64, w)[idx]
dev = lambda a: torch.from_numpy(np.array(a)).cuda()
c48, z32, v32, pi48 = dev(col(lambda r: r[0], 48)), dev(col(lambda r: le32(r[1]), 32)), dev(col(lambda r: le32(r[2]), 32)), dev(col(lambda r: r[3], 48))
pair48 = dev(np.stack([col(lambda r: r[0], 48), col(lambda r: r[4], 48)], axis=1))                  # (n, 2, 48): C_i, -pi_i
scal = dev(np.stack([col(lambda r: le32(1), 32), col(lambda r: le32((R - r[1]) % R), 32)], axis=1))  # (n, 2, 32): 1, r - z_i
shsc = dev(col(lambda r: le32((R - r[2]) % R), 32)).view(n, 1, 32)                                   # r - v_i
d_vk = dev(np.frombuffer(VK, np.uint8))
d_g, d_g2 = d_vk[:96].view(1, 96), d_vk[96:]
seed = bytes(range(32))
ctx = Context(0)
u8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, device="cuda")
st_a, verdict_a, sums = u8(n), u8(1), u8(192)
bases, items = u8(n, 2, 96), u8(n, 192)
dst2, st_l, st_b, verdict_b = u8(2 * n), u8(n), u8(n), u8(1)


def call_a():
    ctx.kzg_check_batch_rlc_dev(c48, z32, v32, pi48, d_vk, st_a, verdict_a, seed, sums=sums)


def call_b(one_decode=False):
    p48, xy = pair48.view(2 * n, 48), bases.view(2 * n, 96)
    if one_decode:
        ctx.g1_decode_batch_dev(p48, xy, dst2)
    else:
        ctx.g1_decode_batch_dev(p48[:n], xy[:n], dst2[:n])
        ctx.g1_decode_batch_dev(p48[n:], xy[n:], dst2[n:])
    items[:, 96:] = bases[:, 1]
    ctx.g1_lincomb_batch_dev(bases, scal, d_g, shsc, items, st_l, out_stride=192)
    ctx.pairing_check_batch_rlc_dev(items, d_g2, st_b, verdict_b, seed)


def once(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); call(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1)


call_b1 = lambda: call_b(one_decode=True)
once(call_a); once(call_b); once(call_b1)
ta, tb, tb1 = [], [], []
for _ in range(5):
    ta.append(once(call_a)); tb.append(once(call_b)); tb1.append(once(call_b1))
ma, mb, mb1 = statistics.median(ta), statistics.median(tb), statistics.median(tb1)
print(f"n = 2^{log2n}", flush=True)
print(f"(a) kzg_check_batch_rlc_dev            : median {ma:9.3f} ms  (min {min(ta):.3f}, max {max(ta):.3f})  {n / ma * 1e3:.3e} openings/s")
print(f"(b) decode x2, lincomb (2, 1), pairing rlc: median {mb:9.3f} ms  (min {min(tb):.3f}, max {max(tb):.3f})  {n / mb * 1e3:.3e} openings/s")
print(f"(b1) the same with one decode call of 2n  : median {mb1:9.3f} ms  (min {min(tb1):.3f}, max {max(tb1):.3f})  {n / mb1 * 1e3:.3e} openings/s")
print(f"(b) / (a) = {mb / ma:.2f}, (b1) / (a) = {mb1 / ma:.2f}", flush=True)
sa, sb = st_a.cpu().numpy(), st_b.cpu().numpy()
assert not sa.any() and not sb.any() and not st_l.cpu().numpy().any(), "invalid items"
assert (sa == sb).all() and int(verdict_a.cpu()[0]) == 0 and int(verdict_b.cpu()[0]) == 0, "(a) and (b) disagree"
print("statuses and verdicts of (a) and (b) agree: all 0, verdict 0")
ctx.profile(True)
total = once(call_a)
ms, groups = ctx.profile_read()
ctx.profile(False)
print(f"stages of (a), one call of {total:.3f} ms: decode {ms[0]:.3f} | digest, prep, fold {ms[1]:.3f} | buckets {ms[2]:.3f} | "
      f"final, combine {ms[3]:.3f} | pairing (the rest) {total - sum(ms):.3f} ms  ({groups} launch group)")
ctx.close()
