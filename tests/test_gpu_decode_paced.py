"""GPU: the one-pass checked decode stage (decompression by inverse root, evenly paced divsteps rounds under the subgroup
test's symbols and under the finish stage's inversion) of the IETF verifier, on Bandersnatch (joint tables) and on JubJub
(no GLV: one radix-16 table per point), through the compressed, keyed and from-alpha forms; statuses against the C oracle.

n = 1, 63, 64, 65, 129: the decode launches run one proof per lane and the finish launch two, so these sizes end in an odd
tail, fill one wave less a lane, fill it, and cross the wave boundary once and twice.  Item i is mutated by i % 12, so every
wave mixes
  0..2 genuine proofs,
  3, 4, 5 a Gamma, pk, H that is no point of the curve,
  6, 7, 8 pk, H, Gamma plus the point of order 2 (on the curve, outside the prime-order subgroup),
  9 a Gamma whose y went in as y + q (or, where that needs bit 255, y = q: not canonical),
  10, 11 the neutral element as pk and as Gamma.
The neutral element puts the symbols' extremes side by side with the random points' 24..36 rounds: 1 - y = 0 finishes
before the first round, and the Montgomery image of 1 + y = 2 rides the slow cycle of two steps per trip (43 rounds).
From alpha H comes out of hash-to-curve, so rows 5 and 7 are genuine there; keyed, the mutated pk is a key of the set that
keyset_create refused."""
import os

import numpy as np
import pytest

import verify_uv_cases as vc
from oracle import c_oracle as co, vrf_oracle as vo

pytestmark = pytest.mark.gpu
NCPU = min(8, os.cpu_count() or 1)
AD = b"paced"
BASE, NKEYS = 132, 8                     # 11 mutation cycles: every row set below starts a cycle somewhere else
SIZES = [1, 63, 64, 65, 129]
SUITES = {"bandersnatch": ("BandersnatchSha512Ell2", 1), "jubjub": ("JubJubSha512Tai", 2)}


def _u8(b):
    return np.frombuffer(b, np.uint8)


@pytest.fixture(scope="module", params=sorted(SUITES))
def batch(request):
    import ark_ec_vrfs_amd as pkg
    name = request.param
    cls, oracle_id = SUITES[name]
    g = vc.group(name)
    S = g.S
    co.set_suite(oracle_id)
    ctx = pkg.Context(0, suite=getattr(pkg, cls), test_blinding_base=True) if name != "bandersnatch" else pkg.Context(0)
    try:
        sk = np.stack([_u8(co.secret_from_seed(vo.synth_seed(700 + i))) for i in range(NKEYS)])
        msg = np.stack([_u8(vo.synth_msg(700 + i)) for i in range(BASE)])
        key = (np.arange(BASE, dtype=np.uint32) * 3) % NKEYS
        ref = co.ietf_prove_batch(sk[key], msgs=msg, ad=AD, threads=NCPU)
        b = {k: ref[k].copy() for k in ("pk", "input", "output", "c", "s")}
        keys = np.stack([b["pk"][np.flatnonzero(key == k)[0]] for k in range(NKEYS)])
        neutral = _u8(vo.point_encode(S, (0, 1)))
        no_point = _u8(g.undecodable())
        # further keys of the set: no point, off the subgroup (key 0 plus the point of order 2), the neutral element
        off_key = _u8(g.off_subgroup(vo.point_decode(S, keys[0].tobytes())))
        extra = np.stack([no_point, off_key, neutral])
        mut = np.arange(BASE) % 12
        for i in range(BASE):
            m = mut[i]
            if m in (3, 4, 5):
                b[("output", "pk", "input")[m - 3]][i] = no_point
                if m == 4:
                    key[i] = NKEYS
            elif m in (6, 7, 8):
                col = ("pk", "input", "output")[m - 6]
                b[col][i] = _u8(g.off_subgroup(vo.point_decode(S, b[col][i].tobytes())))
                if m == 6:
                    key[i] = NKEYS + 1
            elif m == 9:
                raw = int.from_bytes(b["output"][i].tobytes(), "little")
                y, flag = raw & ((1 << 255) - 1), raw >> 255
                y = y + S.q if y + S.q < 1 << 255 else S.q
                b["output"][i] = _u8((y | flag << 255).to_bytes(32, "little"))
            elif m == 10:
                b["pk"][i] = neutral
                key[i] = NKEYS + 2
            elif m == 11:
                b["output"][i] = neutral
        want = co.ietf_verify_batch(b["pk"], b["input"], b["output"], b["c"], b["s"], AD, threads=NCPU)
        want_alpha = co.ietf_verify_batch(b["pk"], ref["input"], b["output"], b["c"], b["s"], AD, threads=NCPU)
        assert (want[mut <= 2] == 0).all() and (want[(mut >= 3) & (mut <= 9)] == 2).all() and (want[mut >= 10] != 0).all()
        assert (want_alpha[(mut == 5) | (mut == 7)] == 0).all()
        ks, kst = ctx.keyset_create(np.concatenate([keys, extra]))
        assert list(kst[:NKEYS + 2]) == [0] * NKEYS + [2, 2]
        want_keyed = want.copy()
        if kst[NKEYS + 2] != 0:                         # a key set that refuses the neutral element answers InvalidData
            want_keyed[mut == 10] = 2
        yield dict(ctx=ctx, b=b, msg=msg, key=key, want=want, want_alpha=want_alpha, want_keyed=want_keyed, ks=ks, name=name)
        ks.close()
    finally:
        ctx.close()
        co.set_suite(1)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("form", ["plain", "keyed", "alpha"])
def test_statuses_of_mixed_waves(batch, form, n):
    ctx, b = batch["ctx"], batch["b"]
    r = (8 + 7 * n + np.arange(n)) % BASE         # n = 1 is row 15: a Gamma that is no point
    pk, inp, out, c, s = (b[k][r] for k in ("pk", "input", "output", "c", "s"))
    if form == "plain":
        got, want = ctx.ietf_verify_batch(pk, inp, out, c, s, ad=AD), batch["want"][r]
    elif form == "keyed":
        got, want = ctx.ietf_verify_batch_keyed(batch["ks"], batch["key"][r], inp, out, c, s, ad=AD), batch["want_keyed"][r]
    else:
        got, want = ctx.ietf_verify_batch_alpha(pk, batch["msg"][r], out, c, s, ad=AD), batch["want_alpha"][r]
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s %s n=%d: %d differ, first rows %s got %s want %s" % (
        batch["name"], form, n, bad.size, r[bad[:8]], got[bad[:8]], want[bad[:8]])
