"""GPU (-m gpu): every verification and proving path that runs the twisted Edwards addition laws (te.cuh: te_add_cached,
te_add_affine on the fused sum of two products), against the C oracle and against the statuses the forgeries call for.

Bandersnatch IETF verification from the wire format at n = 1, 65, 2^17 and 2^17 + 1 -- the last two straddle
STRAUS_FUSE_MAX_ITEMS (kernels.h), so both launch shapes of the Straus ladders run -- with about one proof in 16 forged the
way bench.py's forgery_kinds does it.  Then, at n = 65: IETF prove (proof bytes), IETF verify and Pedersen verify per proof
and batched on Bandersnatch, JubJub, Ed25519 and Baby-JubJub; bandersnatch_sw; keyed verification, affine inputs and
verification from alpha on Bandersnatch."""
import hashlib
import os

import numpy as np
import pytest

from oracle import c_oracle as co

pytestmark = pytest.mark.gpu
NCPU = min(16, os.cpu_count() or 1)
FUSE_MAX = 1 << 17                   # kernels.h: STRAUS_FUSE_MAX_ITEMS
FORGE_EVERY = 16
FORGED_STATUS = np.array([1, 1, 2], np.uint8)      # a bit of c flipped, a bit of s flipped, Gamma = 0xff..ff (InvalidData)
N_ORACLE = 4096


def forgery_kinds(first, m):
    """bench.py's rule: a fixed function of the item index; -1 genuine, 0 / 1 / 2 the kind of forgery"""
    h = (np.arange(first, first + m, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(40)
    return np.where(h % FORGE_EVERY == 0, (h // FORGE_EVERY) % 3, -1).astype(np.int8)


def forge(pr, kinds):
    c, s, g = pr["c"].copy(), pr["s"].copy(), pr["output"].copy()
    c[kinds == 0, 8] ^= 1
    s[kinds == 1, 8] ^= 1
    g[kinds == 2] = 255
    return c, s, g


def expected_status(kinds):
    return np.where(kinds < 0, 0, FORGED_STATUS[np.maximum(kinds, 0)]).astype(np.uint8)


def synth(n, start=0):
    seeds = np.arange(start, start + n, dtype=np.uint64).view(np.uint8).reshape(n, 8)
    raw = b"".join(hashlib.sha512(b"vrfhip-msg" + int(start + k).to_bytes(8, "little")).digest()[:32] for k in range(n))
    return seeds, np.frombuffer(raw, np.uint8).reshape(n, 32).copy()


@pytest.fixture(scope="module")
def big(ctx):
    """2^17 + 1 Bandersnatch proofs made on the device once, forged by forgery_kinds, and the C oracle's statuses of the first
    4096; every size below is a prefix of it"""
    n = FUSE_MAX + 1
    seeds, msg = synth(n)
    sk, _ = ctx.secret_from_seed_batch(seeds)
    pr = ctx.ietf_prove_batch(sk, msgs=msg, ad=b"")
    assert not pr["status"].any()
    kinds = forgery_kinds(0, n)
    c, s, g = forge(pr, kinds)
    m = N_ORACLE
    oracle = co.ietf_verify_batch(pr["pk"][:m], pr["input"][:m], g[:m], c[:m], s[:m], b"", threads=NCPU)
    return dict(pk=pr["pk"], input=pr["input"], output=g, c=c, s=s, want=expected_status(kinds), oracle=oracle,
                sk=sk, msg=msg, genuine=pr)


@pytest.mark.parametrize("n", [1, 65, FUSE_MAX, FUSE_MAX + 1])
def test_bandersnatch_verify_from_the_wire_format(ctx, big, n):
    got = ctx.ietf_verify_batch(big["pk"][:n], big["input"][:n], big["output"][:n], big["c"][:n], big["s"][:n], ad=b"")
    m = min(n, N_ORACLE)
    assert (big["oracle"][:m] == big["want"][:m]).all() and set(np.unique(big["want"])) == {0, 1, 2}
    assert (got[:m] == big["oracle"][:m]).all()
    assert (got == big["want"][:n]).all()


N = 65


def test_bandersnatch_prove_bytes_equal_the_oracle(ctx, big):
    ref = co.ietf_prove_batch(big["sk"][:N], msgs=big["msg"][:N], ad=b"", threads=NCPU)
    for k in ("output", "c", "s", "pk", "input"):
        assert (big["genuine"][k][:N] == ref[k]).all(), k
    got = ctx.ietf_prove_batch(big["sk"][:N], msgs=big["msg"][:N], ad=b"other")
    ref = co.ietf_prove_batch(big["sk"][:N], msgs=big["msg"][:N], ad=b"other", threads=NCPU)
    for k in ("output", "c", "s", "pk", "input"):
        assert (got[k] == ref[k]).all(), k


def test_bandersnatch_from_alpha_keyed_and_affine_inputs(ctx, big):
    a = {k: big[k][:N] for k in ("pk", "input", "output", "c", "s")}
    want = big["oracle"][:N]
    assert want.any() and not want.all()
    assert (ctx.ietf_verify_batch_alpha(a["pk"], big["msg"][:N], a["output"], a["c"], a["s"], ad=b"") == want).all()
    ks, st = ctx.keyset_create(a["pk"][:8])
    try:
        assert not st.any()
        # every proof against its own key among eight resident ones: the proofs of items 0..7, repeated
        idx = (np.arange(N) % 8).astype(np.uint32)
        rep = {k: a[k][idx] for k in ("input", "output", "c", "s")}
        assert (ctx.ietf_verify_batch_keyed(ks, idx, rep["input"], rep["output"], rep["c"], rep["s"], ad=b"") == want[idx]).all()
        wrong = (idx + 1) % 8
        assert ctx.ietf_verify_batch_keyed(ks, wrong, rep["input"], rep["output"], rep["c"], rep["s"], ad=b"").all()
    finally:
        ks.close()
    # typed points: x || y of every decodable encoding; the undecodable Gammas have no typed form, so those items keep the
    # genuine Gamma with the forged c of a neighbour kind
    xy = np.zeros((3, N, 64), np.uint8)
    g = np.where((want == 2)[:, None], big["genuine"]["output"][:N], a["output"])
    c = a["c"].copy()
    c[want == 2, 8] ^= 1
    for j, arr in enumerate((a["pk"], a["input"], g)):
        for i in range(N):
            x, y = co.point_decode(arr[i].tobytes())
            xy[j, i] = np.frombuffer(x.to_bytes(32, "little") + y.to_bytes(32, "little"), np.uint8)
    want_xy = co.ietf_verify_batch(a["pk"], a["input"], g, c, a["s"], b"", threads=NCPU)
    assert (want_xy != 0).sum() == (want != 0).sum()
    assert (ctx.ietf_verify_batch_affine(xy[0], xy[1], xy[2], c, a["s"], ad=b"") == want_xy).all()


SUITES = {"bandersnatch": ("BandersnatchSha512Ell2", 1), "jubjub": ("JubJubSha512Tai", 2), "ed25519": ("Ed25519Sha512Tai", 3), "babyjubjub": ("BabyJubJubSha512Tai", 4)}


@pytest.fixture(params=sorted(SUITES))
def other(request):
    import ark_ec_vrfs_amd as pkg
    cls, sid = SUITES[request.param]
    c = pkg.Context(0, suite=getattr(pkg, cls), test_blinding_base=sid != 1)      # Bandersnatch has its upstream blinding base
    co.set_suite(sid)
    yield c
    co.set_suite(1)
    c.close()


def test_every_curve_prove_verify_and_pedersen(other):
    cx = other
    seeds, msg = synth(N, start=700)
    sk, _ = cx.secret_from_seed_batch(seeds)
    ref = co.ietf_prove_batch(sk, msgs=msg, ad=b"a", threads=NCPU)
    got = cx.ietf_prove_batch(sk, msgs=msg, ad=b"a")
    for k in ("output", "c", "s", "pk", "input"):
        assert (got[k] == ref[k]).all(), k
    kinds = forgery_kinds(0, N)
    c, s, g = forge(ref, kinds)                       # byte 8 of c lies inside every suite's CHALLENGE_LEN
    want = co.ietf_verify_batch(ref["pk"], ref["input"], g, c, s, b"a", threads=NCPU)
    assert ((want != 0) == (kinds >= 0)).all() and want.any()
    assert (cx.ietf_verify_batch(ref["pk"], ref["input"], g, c, s, ad=b"a") == want).all()
    # Pedersen: per proof and batched (one MSM, then the per-proof kernels locate the failures)
    pp = co.pedersen_prove_batch(sk, msgs=msg, ad=b"p", threads=NCPU)
    gp = cx.pedersen_prove_batch(sk, msgs=msg, ad=b"p")
    for k in ("output", "pk_com", "r", "ok", "s", "sb", "input"):
        assert (gp[k] == pp[k]).all(), k
    ps, psb = pp["s"].copy(), pp["sb"].copy()
    ps[kinds == 0, 3] ^= 1
    psb[kinds == 1, 3] ^= 1
    args = (pp["input"], pp["output"], pp["pk_com"], pp["r"], pp["ok"], ps, psb)
    wantp = co.pedersen_verify_batch(*args, ad=b"p", threads=NCPU)
    assert (wantp[kinds < 0] == 0).all() and (wantp[(kinds == 0) | (kinds == 1)] != 0).all()
    assert (cx.pedersen_verify_batch(*args, ad=b"p") == wantp).all()
    st, batch_ok = cx.pedersen_verify_batch_rlc(*args, ad=b"p", seed=bytes(range(32)))
    assert (st == wantp).all() and batch_ok == (not wantp.any())
    clean = (pp["input"], pp["output"], pp["pk_com"], pp["r"], pp["ok"], pp["s"], pp["sb"])
    st, batch_ok = cx.pedersen_verify_batch_rlc(*clean, ad=b"p", seed=bytes(range(32)))
    assert not st.any() and batch_ok


def test_bandersnatch_sw_prove_and_verify():
    import ark_ec_vrfs_amd as pkg
    cx = pkg.Context(0, pkg.BandersnatchSwSha512Tai)
    try:
        _, msg = synth(N, start=900)
        sks = [co.bsw_secret_public(bytes([i]) * 8)[0] for i in range(N)]
        sk = np.stack([np.frombuffer(b, np.uint8) for b in sks])
        ref = co.bsw_ietf_prove_batch(sk, msgs=msg, ad=b"w", threads=NCPU)
        got = cx.ietf_prove_batch(sk, msgs=msg, ad=b"w")
        for k in ("output", "c", "s", "pk", "input"):
            assert (got[k] == ref[k]).all(), k
        kinds = forgery_kinds(0, N)
        c, s = ref["c"].copy(), ref["s"].copy()
        c[kinds == 0, 8] ^= 1
        s[kinds == 1, 8] ^= 1
        want = co.bsw_ietf_verify_batch(ref["pk"], ref["input"], ref["output"], c, s, b"w", threads=NCPU)
        assert want.any() and not want.all()
        assert (cx.ietf_verify_batch(ref["pk"], ref["input"], ref["output"], c, s, ad=b"w") == want).all()
    finally:
        cx.close()
