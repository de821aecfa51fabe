"""GPU (-m gpu): the provers on crafted secrets and given inputs.  tests/prove_cases.py puts sk where the provers' recodings change
shape -- the four 16-digit streams of prove_var_mul, the GLV halves of var_base_mul, sw_scalar_fold and the patched top digit of
sw_quad_mul, the 16-bit comb rows of gcomb_mul / gcomb_mul2 with their rippling carry (the host simulation has 8-bit rows), the
33rd row of sw_comb_mul -- and H on G, -G, 2G, the blinding base, pk, the neutral element, strings that are no point and points
outside the subgroup.  Every output is compared byte for byte with the C oracle's proof (plain double-and-add), pk and Gamma also
with the values the Python oracles' integer arithmetic gives, and the proofs go back through the C oracle's verifier.

All six suites; CT_TABLES; x || y outputs; K proofs per lane forced through VRFHIP_DEBUG_PROVE_K with the set in its own order
and rolled by one, so that refused items, the zero secret and neutral inputs stand at every place within a lane's group of the
shared inversions; the secrets behind the hash-to-curve front ends.  tests/test_hostsim_prove_cases.py runs the same cases on the
CPU.  A refused item has status 2 and zero bytes in every output; its `input` is not compared (the oracle writes none)."""
import numpy as np
import pytest

import prove_cases as pc

pytestmark = pytest.mark.gpu
DEBUG_PROVE_K = 4                    # include/vrfhip.h: VRFHIP_DEBUG_PROVE_K
EDWARDS = ("bandersnatch", "jubjub", "ed25519", "baby_jubjub")       # the suites whose launches read k_lane
AFFINE = ("bandersnatch", "secp256r1", "bandersnatch_sw")


def _suite_class(suite):
    import ark_ec_vrfs_amd as m
    return {"bandersnatch": m.BandersnatchSha512Ell2, "jubjub": m.JubJubSha512Tai, "ed25519": m.Ed25519Sha512Tai,
            "baby_jubjub": m.BabyJubJubSha512Tai, "secp256r1": m.Secp256r1Sha256Tai,
            "bandersnatch_sw": m.BandersnatchSwSha512Tai}[suite]


@pytest.fixture(scope="module")
def contexts():
    """one context per suite, made on first use and closed with the module; Bandersnatch has its upstream blinding base, the
    others the explicitly requested test base the oracles share"""
    from ark_ec_vrfs_amd import Context, SuiteDesc
    made = {}

    def get(suite):
        if suite not in made:
            cls = _suite_class(suite)
            d = SuiteDesc.default(cls) if suite == "bandersnatch" else SuiteDesc.with_test_blinding_base(cls)
            made[suite] = Context(0, desc=d)
            assert made[suite].get_flags() == 0
        return made[suite]
    yield get
    for c in made.values():
        c.close()


def _prove(ctx, cs, pedersen, ad, rows=None, msgs=None):
    rows = np.arange(cs.n) if rows is None else rows
    f = ctx.pedersen_prove_batch if pedersen else ctx.ietf_prove_batch
    if msgs is not None:
        return f(cs.sk[rows], msgs=np.ascontiguousarray(msgs[rows]), ad=ad)
    return f(cs.sk[rows], inputs=cs.inputs[rows], ad=ad)


def _check(cs, got, want, pedersen, rows, what, int_values=True):
    """the C oracle's bytes; pk and Gamma by integer arithmetic; zero bytes for the refused"""
    keys = pc.PED_KEYS if pedersen else pc.IETF_KEYS
    pc.compare(cs, got, want, keys, rows, what)
    if int_values:
        assert (got["output"] == cs.gamma_int[rows]).all(), what
        if not pedersen:
            assert (got["pk"] == cs.pk_int[rows]).all(), what
    bad = got["status"] != 0
    assert (got["status"][bad] == 2).all() and all(not got[k][bad].any() for k in keys[:-1]), what


@pytest.mark.parametrize("suite", pc.SUITES)
def test_ietf_prove_from_given_inputs(contexts, suite):
    """pk, output, c, s, input and status under the three ad; the proofs verify under the C oracle"""
    cs = pc.cases(suite)
    print(cs.describe())
    ctx = contexts(suite)
    for a, ad in enumerate(pc.ADS):
        got = _prove(ctx, cs, False, ad)
        _check(cs, got, cs.ietf[a], False, np.arange(cs.n), "ietf ad %d" % len(ad))
        assert (pc.verify_with_oracle(suite, False, got, ad, cs.accepted) == cs.round_trip).all()


@pytest.mark.parametrize("suite", pc.SUITES)
def test_pedersen_prove_from_given_inputs(contexts, suite):
    """pk_com, r, ok, s, sb and the blinding factor under the three ad; pk_com = sk*G + b*B by the Python oracle's additions from
    the returned b; the proofs verify under the C oracle"""
    cs = pc.cases(suite)
    print(cs.describe())
    ctx = contexts(suite)
    for a, ad in enumerate(pc.ADS):
        got = _prove(ctx, cs, True, ad)
        _check(cs, got, cs.ped[a], True, np.arange(cs.n), "pedersen ad %d" % len(ad))
        st = pc.verify_with_oracle(suite, True, got, ad, cs.accepted)
        assert (st[cs.round_trip == 0] == 0).all() and (a != 1 or (st == cs.round_trip_ped).all())
        if a == 1:
            assert (got["blinding"] == cs.ped[1]["blinding"]).all() and (got["pk_com"] == cs.pk_com_int).all()


@pytest.mark.parametrize("suite", pc.SUITES)
def test_ct_tables_give_the_same_bytes(contexts, suite):
    """Context.CT_TABLES on the whole set: win_lookup_t<true> and sw_lookup_ct differ from the plain lookups at digit 0, at +-8 and
    under the negated fold of secp256r1 -- the digits the crafted secrets hold"""
    cs = pc.cases(suite)
    print(cs.describe())
    ctx = contexts(suite)
    plain = [_prove(ctx, cs, p, pc.ADS[1]) for p in (False, True)]
    ctx.set_flags(ctx.CT_TABLES)
    try:
        ct = [_prove(ctx, cs, p, pc.ADS[1]) for p in (False, True)]
    finally:
        ctx.set_flags(0)
    for p in (False, True):
        _check(cs, ct[p], (cs.ped if p else cs.ietf)[1], p, np.arange(cs.n), "ct %s" % ("pedersen" if p else "ietf"))
        for k in plain[p]:
            assert (plain[p][k] == ct[p][k]).all(), (suite, p, k)


def _xy_expected(suite, enc, mont):
    """(n, 64) x || y of compressed encodings by the Python oracles' decoders: 32-byte little-endian integers, times 2^256 mod q
    under COORDS_MONT256; zero bytes where the encoding is zero bytes (a refused item) or the neutral element has no x || y"""
    from oracle import bsw_oracle as bo, sw_oracle as so, vrf_oracle as vo
    g = pc.group(suite)
    q = {"secp256r1": so.P, "bandersnatch_sw": bo.Q}.get(suite) or g.S.q
    out = np.zeros((len(enc), 64), np.uint8)
    for i, row in enumerate(enc):
        b = row.tobytes()
        if not any(b):
            continue
        if suite == "secp256r1":
            p = so.point_decode(b)
        elif suite == "bandersnatch_sw":
            ok, p = bo.point_decode(b)
            assert ok
        else:
            p = vo.point_decode(g.S, b)
        if p is None:
            continue
        x, y = ((v << 256) % q for v in p) if mont else p
        out[i] = np.frombuffer(x.to_bytes(32, "little") + y.to_bytes(32, "little"), np.uint8)
    return out


@pytest.mark.parametrize("mont", (False, True), ids=("canonical", "mont256"))
@pytest.mark.parametrize("suite", AFFINE)
def test_affine_outputs(contexts, suite, mont):
    """VRFHIP_FLAG_PROVE_POINTS_AFFINE, with and without COORDS_MONT256: the points come out as the x || y of the compressed
    outputs, zero bytes for the refused items and for a neutral point of the short-Weierstrass codecs; scalars unchanged"""
    cs = pc.cases(suite)
    print(cs.describe())
    ctx = contexts(suite)
    ctx.set_flags(ctx.PROVE_POINTS_AFFINE | (ctx.COORDS_MONT256 if mont else 0))
    try:
        gi, gp = _prove(ctx, cs, False, pc.ADS[1]), _prove(ctx, cs, True, pc.ADS[1])
    finally:
        ctx.set_flags(0)
    wi, wp = cs.ietf[1], cs.ped[1]
    n_neutral = 0
    for got, want, pts in ((gi, wi, ("output", "pk")), (gp, wp, ("output", "pk_com", "r", "ok"))):
        for k in pts:
            exp = _xy_expected(suite, want[k], mont)
            n_neutral += int((~exp.any(axis=1) & (want["status"] == 0)).sum())
            bad = np.flatnonzero((got[k] != exp).any(axis=1))
            assert bad.size == 0, (suite, k, [cs.tags[i] for i in bad[:8]])
        for k in ("c", "s", "sb", "blinding", "status"):
            if k in got:
                assert (got[k] == want[k]).all(), (suite, k)
        acc = want["status"] == 0
        assert (got["input"][acc] == want["input"][acc]).all()
    print("%s: %d cases, %d neutral points without x || y" % (suite, cs.n, n_neutral))
    assert (n_neutral > 0) == (suite != "bandersnatch")          # (0, 1) has coordinates; infinity has none


@pytest.mark.parametrize("K", (1, 2, 4, 8))
@pytest.mark.parametrize("suite", EDWARDS)
def test_several_proofs_per_lane(contexts, suite, K):
    """VRFHIP_DEBUG_PROVE_K: the shared inversion of prove_encode_multi over 4K Z coordinates (and, on Bandersnatch from
    messages, the two of prove_prepare_multi).  The set in its own order and rolled by one item; both schemes; every item's
    bytes are those of the K = 1 run and of the expectations.  lanes_k gives a lane several proofs only from 2^18 items up."""
    cs = pc.cases(suite)
    print(cs.describe())
    ctx = contexts(suite)
    own = np.arange(cs.n)
    sec = cs.secret_rows
    runs = [(own, None), (np.roll(own, 1), None)]
    if suite == "bandersnatch":
        runs += [(sec, cs.msgs), (np.roll(sec, 1), cs.msgs)]
    base = {}
    try:
        for k_lane in (1, K):
            ctx.debug_set(DEBUG_PROVE_K, k_lane)
            for j, (rows, msgs) in enumerate(runs):
                for p in (False, True):
                    got = _prove(ctx, cs, p, pc.ADS[1], rows, msgs)
                    want = ((cs.ped_msg if p else cs.ietf_msg) if msgs is not None else (cs.ped if p else cs.ietf)[1])
                    _check(cs, got, want, p, rows, "K=%d run %d %s" % (k_lane, j, "pedersen" if p else "ietf"), int_values=msgs is None)
                    if k_lane == 1:
                        base[j, p] = got
                    else:
                        for k in got:
                            assert (got[k] == base[j, p][k]).all(), (suite, K, j, p, k)
    finally:
        ctx.debug_set(DEBUG_PROVE_K, 0)


@pytest.mark.parametrize("suite", ("secp256r1", "bandersnatch_sw"))
def test_zero_secret_and_neutral_input_leave_the_finite_points_whole(contexts, suite):
    """sk = 0 (pk and Gamma neutral) and H neutral on the short-Weierstrass suites: on bandersnatch_sw two, or all four, map
    denominators of k_bsw_prove_finish degenerate inside one fe_batch_inv<true> and bsw_frac puts one in their place; the finite
    points of the same item -- k*G, k*H, and with them c, s, R and Ok -- must come out as the oracle has them"""
    cs = pc.cases(suite)
    print(cs.describe())
    ctx = contexts(suite)
    rows = np.array([i for i in range(cs.n) if cs.sk_int[i] == 0 or cs.kinds[i] == "neutral"])
    assert len(rows) >= 12 and (cs.status[rows] == 0).sum() >= (7 if suite == "secp256r1" else 20)
    gi, gp = _prove(ctx, cs, False, pc.ADS[1], rows), _prove(ctx, cs, True, pc.ADS[1], rows)
    _check(cs, gi, cs.ietf[1], False, rows, "degenerate ietf")
    _check(cs, gp, cs.ped[1], True, rows, "degenerate pedersen")
    acc = cs.status[rows] == 0
    assert gi["c"][acc].any(axis=1).all() and gi["s"][acc].any(axis=1).all() and gp["r"][acc].any(axis=1).all()
    neutral = pc.group(suite).enc_out(None)          # 33 zero bytes on secp256r1, x = 0 with the infinity flag on bandersnatch_sw
    for j, i in enumerate(rows):
        if acc[j] and cs.sk_int[i] == 0:
            assert gi["pk"][j].tobytes() == neutral and gi["output"][j].tobytes() == neutral and gp["output"][j].tobytes() == neutral
        if acc[j] and cs.kinds[i] == "neutral":
            assert gi["output"][j].tobytes() == neutral and gp["ok"][j].tobytes() == neutral


@pytest.mark.parametrize("suite", pc.SUITES)
def test_prove_from_messages(contexts, suite):
    """the secrets-only part with one fixed message per item: crafted secrets behind Elligator 2 and try-and-increment"""
    cs = pc.cases(suite)
    ctx = contexts(suite)
    rows = cs.secret_rows
    print(cs.describe())
    for p in (False, True):
        got = _prove(ctx, cs, p, pc.ADS[1], rows, cs.msgs)
        want = cs.ped_msg if p else cs.ietf_msg
        _check(cs, got, want, p, rows, "msgs %s" % ("pedersen" if p else "ietf"), int_values=False)
        if not p:
            assert (got["pk"] == cs.pk_int[rows]).all()
        st = pc.verify_with_oracle(suite, p, got, pc.ADS[1], np.flatnonzero(want["status"] == 0))
        ok = np.array([cs.sk_int[i] != 0 or suite != "secp256r1" for i in np.flatnonzero(want["status"] == 0)])
        assert (st[ok] == 0).all()
