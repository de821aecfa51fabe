"""GPU (-m gpu): per-proof Pedersen verification on crafted (c, s, sb).  vrfhip_test_pedersen_verify_c runs the decode, ladder
and finish launches of vrfhip_pedersen_verify_batch and puts a supplied challenge over the hashed one in between, so
tests/pedersen_c_cases.py can build ACCEPTING items at the scalars where recodings and comb walks change shape -- and for
each a near miss that must be rejected.  The production kernels answer 0 exactly when s*H - c*Gamma and
s*G + sb*B - c*pk_com come out right; no status test on genuine proofs can say that about scalars no prover emits, and the
U / V readout of tests/test_gpu_verify_uv.py pins the IETF verifier's ladders, which are no longer the ones Pedersen runs.

The host simulation (tests/test_hostsim_pedersen_c.py) runs the same rows; it has neither the chained field products nor the
16-bit combs of the generator and of the blinding base.  These tests see both.

All six suites: the whole set at its own size (the fused launch of the Edwards suites), tiled to either side of
STRAUS_FUSE_MAX_ITEMS, x || y inputs (canonical and Montgomery-256), and descriptors with a non-default challenge length."""
import numpy as np
import pytest

import pedersen_c_cases as pc

pytestmark = pytest.mark.gpu
FUSE_MAX = 1 << 17                   # kernels.h: STRAUS_FUSE_MAX_ITEMS


def _suite_class(suite):
    import ark_ec_vrfs_amd as m
    return {"bandersnatch": m.BandersnatchSha512Ell2, "jubjub": m.JubJubSha512Tai, "ed25519": m.Ed25519Sha512Tai,
            "baby_jubjub": m.BabyJubJubSha512Tai, "secp256r1": m.Secp256r1Sha256Tai,
            "bandersnatch_sw": m.BandersnatchSwSha512Tai}[suite]


@pytest.fixture(scope="module")
def contexts():
    """one context per (suite, challenge length), made on first use and closed with the module; Bandersnatch has its pinned
    blinding base, the others the test base the oracles share"""
    from ark_ec_vrfs_amd import Context, SuiteDesc
    made = {}

    def get(suite, L=None):
        L = pc.DEFAULT_L[suite] if L is None else L
        if (suite, L) not in made:
            cls = _suite_class(suite)
            d = SuiteDesc.default(cls) if suite == "bandersnatch" else SuiteDesc.with_test_blinding_base(cls)
            d.challenge_len = L
            made[suite, L] = Context(0, desc=d)
            assert made[suite, L].desc().challenge_len == L
        return made[suite, L]
    yield get
    for c in made.values():
        c.close()


def _compare(cs, st, rows=None):
    """the statuses against the generator's (rows: which row of the set each item is)"""
    rows = np.arange(cs.n) if rows is None else rows
    bad = np.flatnonzero(st != cs.status[rows])
    print("%s L=%d: %d items, %d differ" % (cs.suite, cs.L, rows.size, bad.size))
    assert bad.size == 0, "%s L=%d: %d items differ, first (row, tag, got, want): %s" % (
        cs.suite, cs.L, bad.size, [(int(rows[i]), cs.tags[rows[i]], int(st[i]), int(cs.status[rows[i]])) for i in bad[:8]])


@pytest.mark.parametrize("suite", pc.SUITES)
def test_whole_set(contexts, suite):
    """the set at its own number (several hundred): one launch group, the fused Straus launch on the Edwards suites.  The genuine
    proofs among the rows must also pass the production call, whose challenge is the hash the supplied one was recomputed as."""
    cs = pc.cases(suite)
    ctx = contexts(suite)
    _compare(cs, ctx.test_pedersen_verify_c(*cs.points(), cs.c, cs.s, cs.sb))
    tie = np.array([i for i, k in enumerate(cs.kinds) if k == "tie"])
    assert tie.size == pc.N_TIE
    assert not ctx.pedersen_verify_batch(*cs.points(tie), cs.s[tie], cs.sb[tie], ad=b"").any()


@pytest.mark.parametrize("n", (FUSE_MAX, FUSE_MAX + 1))
@pytest.mark.parametrize("suite", [s for s in pc.SUITES if s != "secp256r1"])
def test_either_side_of_the_fuse_threshold(contexts, suite, n):
    """The set tiled to STRAUS_FUSE_MAX_ITEMS and to one more: launch_ped_t runs both halves in one launch
    (k_ped_verify_straus_both) up to it and as two launches above it; every tile must give the same rows.  bandersnatch_sw runs at
    the same sizes (launch_bsw_pedersen_verify does not switch).  secp256r1 is left out: p256::launch_pedersen_verify has no size
    switch -- the same launches at every n."""
    cs = pc.cases(suite)
    rows = np.arange(n) % cs.n
    _compare(cs, contexts(suite).test_pedersen_verify_c(*cs.points(rows), cs.c[rows], cs.s[rows], cs.sb[rows]), rows)


@pytest.mark.parametrize("suite", ("bandersnatch", "secp256r1"))
def test_affine_inputs(contexts, suite):
    """x || y inputs built from the oracle's coordinates: the same statuses.  Rows without five affine points (an undecodable
    string, a point off the subgroup, a neutral point of a short-Weierstrass codec) are left out."""
    cs = pc.cases(suite)
    r = cs.xy_rows
    assert r.size >= cs.n - 8
    _compare(cs, contexts(suite).test_pedersen_verify_c(*cs.points(xy=True), cs.c[r], cs.s[r], cs.sb[r], affine=True), r)


def test_affine_inputs_montgomery():
    """the same under VRFHIP_FLAG_COORDS_MONT256: every coordinate as v * 2^256 mod q, converted here with Python integers"""
    from ark_ec_vrfs_amd import Context
    cs = pc.cases("bandersnatch")
    q = pc.group("bandersnatch").S.q
    r = cs.xy_rows

    def mont(a):
        out = bytearray()
        for row in a:
            b = row.tobytes()
            for k in (0, 32):
                out += (int.from_bytes(b[k:k + 32], "little") * (1 << 256) % q).to_bytes(32, "little")
        return np.frombuffer(bytes(out), np.uint8).reshape(-1, 64)

    ctx = Context(0, _suite_class("bandersnatch"))
    try:
        ctx.set_flags(ctx.COORDS_MONT256)
        _compare(cs, ctx.test_pedersen_verify_c(*(mont(a) for a in cs.points(xy=True)), cs.c[r], cs.s[r], cs.sb[r], affine=True), r)
    finally:
        ctx.close()


@pytest.mark.parametrize("suite,L", [(s, L) for s, ls in pc.EXTRA_L.items() for L in ls])
def test_other_challenge_lengths(contexts, suite, L):
    """a descriptor's challenge length moves the window the c ladders start from (challenge_top_window), the bound on a supplied
    c, and the truncation of the real challenge the genuine rows carry"""
    cs = pc.cases(suite, L)
    ctx = contexts(suite, L)
    _compare(cs, ctx.test_pedersen_verify_c(*cs.points(), cs.c, cs.s, cs.sb))
    tie = np.array([i for i, k in enumerate(cs.kinds) if k == "tie"])
    assert not ctx.pedersen_verify_batch(*cs.points(tie), cs.s[tie], cs.sb[tie], ad=b"").any()
