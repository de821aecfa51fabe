"""GPU: the joint-table IETF verifier of the GLV suite through its four entry forms -- compressed points, from alpha, keyed and
x || y -- on a mixed batch: genuine proofs, flipped c, flipped s, an undecodable Gamma, a pk outside the prime-order subgroup
and s = r, statuses against the C oracle.  Sizes end inside a lane's K-group and inside a wave (1, 2, 63, 65, 513); 2^17 + 3
takes the two-launch ladder path, everything at or below 2^17 the fused launch."""
import os

import numpy as np
import pytest

import verify_uv_cases as vc
from oracle import c_oracle as co, vrf_oracle as vo

pytestmark = pytest.mark.gpu
NCPU = min(8, os.cpu_count() or 1)
S = vo.BANDERSNATCH
AD = b"joint"
BASE, OFF, NKEYS = 520, 3, 8
SIZES = [1, 2, 63, 65, 513, (1 << 17) + 3]


def _xy(p):
    return np.frombuffer(p[0].to_bytes(32, "little") + p[1].to_bytes(32, "little"), np.uint8)


@pytest.fixture(scope="module")
def batch(ctx, synth):
    """BASE proofs over NKEYS keys, item i mutated by i % 8: 0..2 genuine, 3 flipped c, 4 flipped s, 5 undecodable Gamma
    (x || y form: a point off the curve), 6 pk + the point of order 2 (keyed form: the index of such a key), 7 s = r."""
    g = vc.group("bandersnatch")
    sk, msg = synth(BASE, start=900)
    key = (np.arange(BASE, dtype=np.uint32) * 3) % NKEYS
    ref = co.ietf_prove_batch(sk[key], msgs=msg, ad=AD, threads=NCPU)
    b = {k: ref[k].copy() for k in ("pk", "input", "output", "c", "s")}
    keys = np.stack([b["pk"][np.flatnonzero(key == k)[0]] for k in range(NKEYS)])
    bad_key = np.frombuffer(g.off_subgroup(vo.point_decode(S, keys[0].tobytes())), np.uint8)
    st, xy = ctx.point_validate_batch(np.concatenate([b["pk"], b["input"], b["output"]]), want_xy=True)
    assert (st == 0).all()
    xyv = {k: xy[j * BASE:(j + 1) * BASE].copy() for j, k in enumerate(("pk", "input", "output"))}
    mut = np.arange(BASE) % 8
    for i in range(BASE):
        if mut[i] == 3:
            b["c"][i, 0] ^= 1
        elif mut[i] == 4:
            b["s"][i, 5] ^= 0x10
        elif mut[i] == 5:
            b["output"][i] = np.frombuffer(g.undecodable(), np.uint8)
            x, y = vo.point_decode(S, ref["output"][i].tobytes())
            assert not vo.te_is_on_curve(S, (x, (y + 1) % S.q))
            xyv["output"][i] = _xy((x, (y + 1) % S.q))
        elif mut[i] == 6:
            x, y = vo.point_decode(S, b["pk"][i].tobytes())
            b["pk"][i] = np.frombuffer(g.off_subgroup((x, y)), np.uint8)
            xyv["pk"][i] = _xy(((-x) % S.q, (-y) % S.q))
            key[i] = NKEYS
        elif mut[i] == 7:
            b["s"][i] = np.frombuffer(S.r.to_bytes(32, "little"), np.uint8)
    want = co.ietf_verify_batch(b["pk"], b["input"], b["output"], b["c"], b["s"], AD, threads=NCPU)
    assert (want[mut <= 2] == 0).all() and (want[(mut == 3) | (mut == 4)] == 1).all() and (want[mut >= 5] == 2).all()
    ks, kst = ctx.keyset_create(np.concatenate([keys, bad_key[None]]))
    assert list(kst) == [0] * NKEYS + [2]
    yield dict(b=b, xy=xyv, msg=msg, key=key, want=want, ks=ks)
    ks.close()


def _rows(n):
    return OFF + np.arange(n) % 513


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("form", ["plain", "alpha", "keyed", "xy"])
def test_joint_verifier_statuses(ctx, batch, form, n):
    r = _rows(n)
    b, want = batch["b"], batch["want"][r]
    pk, inp, out, c, s = (b[k][r] for k in ("pk", "input", "output", "c", "s"))
    if form == "plain":
        got = ctx.ietf_verify_batch(pk, inp, out, c, s, ad=AD)
    elif form == "alpha":
        got = ctx.ietf_verify_batch_alpha(pk, batch["msg"][r], out, c, s, ad=AD)
    elif form == "keyed":
        got = ctx.ietf_verify_batch_keyed(batch["ks"], batch["key"][r], inp, out, c, s, ad=AD)
    else:
        x = batch["xy"]
        got = ctx.ietf_verify_batch_affine(x["pk"][r], x["input"][r], x["output"][r], c, s, ad=AD)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s n=%d: %d differ, first rows %s got %s want %s" % (form, n, bad.size, r[bad[:8]], got[bad[:8]], want[bad[:8]])
