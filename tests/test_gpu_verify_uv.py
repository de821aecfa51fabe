"""GPU (-m gpu): the two points IETF verification hashes, U = s*G - c*pk and V = s*H - c*Gamma, read out of the verification
kernels themselves (vrfhip_test_verify_uv: the decode and ladder launches of vrfhip_ietf_verify_batch, then a readout in
place of the finish stage) and compared byte for byte with the oracles' integer arithmetic on tests/verify_uv_cases.py.

The verifier's verdict cannot show a subtly wrong ladder on crafted scalars -- every crafted (c, s) is a forgery and is
rejected either way -- and the host simulation builds neither the chained field products (fe.cuh mac<true> differs from
mac<false> under __HIP_DEVICE_COMPILE__ only) nor the 16-bit fixed-base comb.  These tests see both.

All six suites: the whole set at its own size (the fused launch of the Edwards suites), tiled to either side of
STRAUS_FUSE_MAX_ITEMS, the keyed launches, x || y inputs, and descriptors with a non-default challenge length."""
import numpy as np
import pytest

import verify_uv_cases as vc

pytestmark = pytest.mark.gpu
FUSE_MAX = 1 << 17                   # kernels.h: STRAUS_FUSE_MAX_ITEMS


def _suite_class(suite):
    import ark_ec_vrfs_amd as m
    return {"bandersnatch": m.BandersnatchSha512Ell2, "jubjub": m.JubJubSha512Tai, "ed25519": m.Ed25519Sha512Tai,
            "baby_jubjub": m.BabyJubJubSha512Tai, "secp256r1": m.Secp256r1Sha256Tai,
            "bandersnatch_sw": m.BandersnatchSwSha512Tai}[suite]


@pytest.fixture(scope="module")
def contexts():
    """one context per (suite, challenge length), made on first use and closed with the module"""
    from ark_ec_vrfs_amd import Context, SuiteDesc
    made = {}

    def get(suite, L=None):
        L = vc.DEFAULT_L[suite] if L is None else L
        if (suite, L) not in made:
            cls = _suite_class(suite)
            if L == vc.DEFAULT_L[suite]:
                made[suite, L] = Context(0, cls)
            else:
                d = SuiteDesc.default(cls)
                d.challenge_len = L
                made[suite, L] = Context(0, desc=d)
            assert made[suite, L].desc().challenge_len == L
        return made[suite, L]
    yield get
    for c in made.values():
        c.close()


def _compare(cs, got, rows=None):
    """byte equality of u, v and status with the generator's rows (rows: which row of the set each item is)"""
    u, v, st = got
    rows = np.arange(cs.n) if rows is None else rows
    bad = np.flatnonzero((st != cs.status[rows]) | (u != cs.u[rows]).any(axis=1) | (v != cs.v[rows]).any(axis=1))
    assert bad.size == 0, "%s L=%d: %d items differ, first: %s" % (
        cs.suite, cs.L, bad.size, [(int(i), cs.tags[rows[i]], int(st[i])) for i in bad[:8]])


@pytest.mark.parametrize("suite", vc.SUITES)
def test_whole_set(contexts, suite):
    """the distinct cases at their own number (a few hundred): one launch group, the fused Straus launch on the Edwards suites"""
    cs = vc.cases(suite)
    _compare(cs, contexts(suite).test_verify_uv(cs.pk, cs.input, cs.output, cs.c, cs.s))


@pytest.mark.parametrize("n", (FUSE_MAX, FUSE_MAX + 1))
@pytest.mark.parametrize("suite", [s for s in vc.SUITES if s != "secp256r1"])
def test_either_side_of_the_fuse_threshold(contexts, suite, n):
    """The set tiled to STRAUS_FUSE_MAX_ITEMS and to one more: launch_verify_t runs both halves in one launch up to it and
    as two launches (and the capped decode instantiation) above it; every tile must give the same rows.  bandersnatch_sw
    runs at the same sizes (launch_bsw_ietf_verify does not switch today).  secp256r1 is left out: p256::launch_verify has
    no size threshold -- the same four launches at every n."""
    cs = vc.cases(suite)
    rows = np.arange(n) % cs.n
    got = contexts(suite).test_verify_uv(cs.pk[rows], cs.input[rows], cs.output[rows], cs.c[rows], cs.s[rows])
    _compare(cs, got, rows)


@pytest.mark.parametrize("suite", vc.SUITES)
def test_keyed(contexts, suite):
    """the keyed launches (U from the key's resident comb): every challenge case under three keys of an 8-key set, and an
    index that names no key -- status 2, as k_verify_decode_keyed and verify_finish_multi report it"""
    kc = vc.keyed_cases(suite)
    ctx = contexts(suite)
    ks, kst = ctx.keyset_create(kc.keys)
    try:
        assert not kst.any()
        cs = kc.cases
        _compare(cs, ctx.test_verify_uv(None, cs.input, cs.output, cs.c, cs.s, keyset=ks, key_index=kc.key_index))
    finally:
        ks.close()


@pytest.mark.parametrize("suite", ("bandersnatch", "secp256r1"))
def test_affine_inputs(contexts, suite):
    """x || y inputs built from the oracle's coordinates: the same U and V"""
    cs = vc.cases(suite)
    r = cs.xy_rows
    assert r.size >= cs.n - 8
    _compare(cs, contexts(suite).test_verify_uv(cs.pk_xy, cs.input_xy, cs.output_xy, cs.c[r], cs.s[r], affine=True), r)


@pytest.mark.parametrize("suite,L", [(s, L) for s, ls in vc.EXTRA_L.items() for L in ls])
def test_other_challenge_lengths(contexts, suite, L):
    """a descriptor's challenge length moves the window the c ladders start from (challenge_top_window)"""
    cs = vc.cases(suite, L)
    _compare(cs, contexts(suite, L).test_verify_uv(cs.pk, cs.input, cs.output, cs.c, cs.s))
