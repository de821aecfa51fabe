"""Time of the batched multi-point KZG opening check on the device (vrfhip_kzg_multi_check_batch_rlc_dev) for the ring-proof
shape (k, m, p) = (5, 3, 2) against the chain of calls a caller has to use without it.  Inputs resident in HBM, hip events
around the calls, one warm-up each, then 5 timed rounds in which the two alternate; medians.
  (a) vrfhip_kzg_multi_check_batch_rlc_dev on the arrays as they come from the wire;
  (b) two checked vrfhip_g1_decode_batch_dev calls (the n k commitments, the n p proofs), two strided copies that lay the
      decoded points out item by item as the bases of A_i (those of B_i are the decoded proofs as they lie),
      vrfhip_g1_lincomb_batch_dev for A_i (k + p own terms under [s_ij, u_ij z_ij mod r], m + 1 shared terms [g, S_*] under
      t_i*) and for B_i (p terms under r - u_ij), both written into the item array, and vrfhip_pairing_check_batch_rlc_dev.
      The caller's scalar rows are prepared beforehand and left out of the timing.
The items are honest openings under a toy secret, 64 distinct ones tiled over the batch (the weights differ per index, so the
bucket loads are those of distinct items).  The statuses and verdicts of (a) and (b) must agree.  The stages of (a) come from
the context's profiling events: decode | digest, prep, fold | buckets | final, combine; the pairing is the rest of the call.
One size per run, each run under its own time limit:
usage: timeout 300 python tools/gpu_kzg_multi_time.py 14 && timeout 600 python tools/gpu_kzg_multi_time.py 18"""
import os, random, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from ark_ec_vrfs_amd import Context
from oracle import bls_oracle as bls
from oracle import c_oracle as co

P, R = bls.P, bls.R
K, M, NP = 5, 3, 2
log2n = int(sys.argv[1]) if len(sys.argv) > 1 else 14
n = 1 << log2n
rnd = random.Random(31)
w48 = lambda x: int(x).to_bytes(48, "little")
le32 = lambda x: int(x).to_bytes(32, "little")
TAU = rnd.randrange(1, R)
G = co.g1_mul(rnd.randrange(1, R), w48(bls.G1[0]) + w48(bls.G1[1]))
H = b"".join(w48(x) for x in (bls.G2[0].a, bls.G2[0].b, bls.G2[1].a, bls.G2[1].b))
VK = G + H + co.g2_mul(TAU, H)
SIGMA = [rnd.randrange(1, R) for _ in range(M)]
SHARED = b"".join(co.g1_mul(s, G) for s in SIGMA)


def compress(b96):
    x, y = int.from_bytes(b96[:48], "little"), int.from_bytes(b96[48:], "little")
    out = bytearray(x.to_bytes(48, "big"))
    out[0] |= 0x80 | (0x20 if y > P - y else 0)
    return bytes(out)


rows = []                 # (c48 x K, s x K, t x (M + 1), pi48 x NP, z x NP, u x NP)
for _ in range(64):
    c, q = [rnd.randrange(1, R) for _ in range(K)], [rnd.randrange(1, R) for _ in range(NP)]
    s, u, z = ([rnd.randrange(1, R) for _ in range(cnt)] for cnt in (K, NP, NP))
    t = [0] + [rnd.randrange(R) for _ in range(M)]
    t[0] = -(sum(a * b for a, b in zip(s, c)) + sum(a * b for a, b in zip(t[1:], SIGMA)) +
             sum(a * b * d for a, b, d in zip(u, z, q)) - TAU * sum(a * b for a, b in zip(u, q))) % R
    rows.append(([compress(co.g1_mul(x, G)) for x in c], s, t, [compress(co.g1_mul(x, G)) for x in q], z, u))
idx = np.arange(n) % 64
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()


def col(f, cnt, w):
    return np.frombuffer(b"".join(x for r in rows for x in f(r)), np.uint8).reshape(64, cnt, w)[idx]


c48, s32, t32 = dev(col(lambda r: r[0], K, 48)), dev(col(lambda r: map(le32, r[1]), K, 32)), dev(col(lambda r: map(le32, r[2]), M + 1, 32))
pi48, z32, u32 = dev(col(lambda r: r[3], NP, 48)), dev(col(lambda r: map(le32, r[4]), NP, 32)), dev(col(lambda r: map(le32, r[5]), NP, 32))
# the chain's scalar rows, prepared by the caller: [s_ij, u_ij z_ij mod r] and r - u_ij
scal_a = dev(col(lambda r: [le32(x) for x in r[1]] + [le32(a * b % R) for a, b in zip(r[5], r[4])], K + NP, 32))
scal_b = dev(col(lambda r: [le32((R - x) % R) for x in r[5]], NP, 32))
d_vk = dev(np.frombuffer(VK, np.uint8))
d_shared = dev(np.frombuffer(SHARED, np.uint8).reshape(M, 96))
d_gs = torch.cat([d_vk[:96].view(1, 96), d_shared])          # g, S_1 .. S_m: the shared bases of the chain's A_i
d_g2 = d_vk[96:]
seed = bytes(range(32))
ctx = Context(0)
u8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, device="cuda")
st_a, verdict_a, sums = u8(n), u8(1), u8(192)
bases_a, items = u8(n, K + NP, 96), u8(n, 192)
xy_c, xy_p, dst_c, dst_p = u8(n, K, 96), u8(n, NP, 96), u8(n * K), u8(n * NP)
st_la, st_lb, st_b, verdict_b = u8(n), u8(n), u8(n), u8(1)


def call_a():
    ctx.kzg_multi_check_batch_rlc_dev(c48, s32, d_shared, t32, pi48, z32, u32, d_vk, st_a, verdict_a, seed, sums=sums)


def call_b():
    ctx.g1_decode_batch_dev(c48.view(n * K, 48), xy_c.view(n * K, 96), dst_c)
    ctx.g1_decode_batch_dev(pi48.view(n * NP, 48), xy_p.view(n * NP, 96), dst_p)
    bases_a[:, :K] = xy_c
    bases_a[:, K:] = xy_p
    ctx.g1_lincomb_batch_dev(bases_a, scal_a, d_gs, t32, items, st_la, out_stride=192)
    ctx.g1_lincomb_batch_dev(xy_p, scal_b, None, None, items.view(-1)[96:], st_lb, out_stride=192)
    ctx.pairing_check_batch_rlc_dev(items, d_g2, st_b, verdict_b, seed)


def once(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); call(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1)


once(call_a); once(call_b)
ta, tb = [], []
for _ in range(5):
    ta.append(once(call_a)); tb.append(once(call_b))
ma, mb = statistics.median(ta), statistics.median(tb)
print(f"n = 2^{log2n}, shape (k, m, p) = ({K}, {M}, {NP})", flush=True)
print(f"(a) kzg_multi_check_batch_rlc_dev                 : median {ma:9.3f} ms  (min {min(ta):.3f}, max {max(ta):.3f})  {n / ma * 1e3:.3e} items/s")
print(f"(b) decode x2, lincomb (7, 4) and (2, 0), pairing rlc: median {mb:9.3f} ms  (min {min(tb):.3f}, max {max(tb):.3f})  {n / mb * 1e3:.3e} items/s")
print(f"(b) / (a) = {mb / ma:.2f}", flush=True)
sa, sb = st_a.cpu().numpy(), st_b.cpu().numpy()
dec_ok = not dst_c.cpu().numpy().any() and not dst_p.cpu().numpy().any()
assert not sa.any() and not sb.any() and dec_ok and not st_la.cpu().numpy().any() and not st_lb.cpu().numpy().any(), "invalid items"
assert (sa == sb).all() and int(verdict_a.cpu()[0]) == 0 and int(verdict_b.cpu()[0]) == 0, "(a) and (b) disagree"
print("statuses and verdicts of (a) and (b) agree: all 0, verdict 0")
ctx.profile(True)
total = once(call_a)
ms, groups = ctx.profile_read()
ctx.profile(False)
print(f"stages of (a), one call of {total:.3f} ms: decode {ms[0]:.3f} | digest, prep, fold {ms[1]:.3f} | buckets {ms[2]:.3f} | "
      f"final, combine {ms[3]:.3f} | pairing (the rest) {total - sum(ms):.3f} ms  ({groups} launch group)")
ctx.close()
