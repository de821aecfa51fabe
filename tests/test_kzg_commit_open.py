"""GPU: vrfhip_g1_srs_*, vrfhip_kzg_commit_batch*, vrfhip_kzg_open_batch* -- KZG commitments and non-hiding openings over a
resident base set -- against the native C oracle (oracle.c_oracle.g1_mul / g1_add) and Python integers.

With the bases [tau^j] G of a toy tau the commitment of p is [p(tau) mod r] G and the proof of p(z) = v is
[(p(tau) - v) (tau - z)^-1 mod r] G: one scalar multiplication of the oracle per expected point.  The same commitments and
openings then go through Context.kzg_check_batch / kzg_check_batch_rlc under the toy key (G, H, [tau] H)."""
import ctypes
import random

import numpy as np
import pytest

from oracle import bls_oracle as bls
from oracle import c_oracle as co

pytestmark = pytest.mark.gpu

P, R = bls.P, bls.R
INF = bytes(96)
INF48 = bytes([0xC0]) + bytes(47)
TAU = 0x1D0C7A5E2B9F4C6D8E1A3B5C7D9E0F123456789ABCDEF0123456789ABCDEF01 % R
N_SRS = 2304
B, M = 256, 16                                     # lanes per workgroup and coefficients per lane of the quotient kernel
OPEN_LENGTHS = [1, 2, 3, B - 1, B, B + 1, 2 * B + 1, 2049]
COMMIT_SHAPES = [(1, 1), (1, 2), (3, 65), (2, 300), (3, 2049), (5, 2049)]
le = lambda x: int(x).to_bytes(32, "little")


def w48(x):
    return int(x).to_bytes(48, "little")


G96 = w48(bls.G1[0]) + w48(bls.G1[1])
H192 = b"".join(w48(x) for x in (bls.G2[0].a, bls.G2[0].b, bls.G2[1].a, bls.G2[1].b))


def neg96(b):
    return b if b == INF else b[:48] + w48((P - int.from_bytes(b[48:], "little")) % P)


def compress(b96):
    """96-byte affine point -> the 48-byte zcash / ark-bls12-381 form"""
    if b96 == INF:
        return INF48
    x, y = int.from_bytes(b96[:48], "little"), int.from_bytes(b96[48:], "little")
    out = bytearray(x.to_bytes(48, "big"))
    out[0] |= 0x80 | (0x20 if y > P - y else 0)
    return bytes(out)


def mulG(k):
    k %= R
    return INF if k == 0 else co.g1_mul(k, G96)


def chunks10(pattern, chunks=26):
    return sum(pattern << (10 * w) for w in range(chunks)) % (1 << 255) % R


EDGE_SCALARS = [0, 1, R - 1] + [chunks10(p) for p in (0x1ff, 0x200, 0x3ff)] + [chunks10(p, 25) for p in (0x1ff, 0x200, 0x3ff)]
_rnd = random.Random(2026)
NONSQUARE_X = next(x for x in iter(lambda: _rnd.randrange(P), None) if pow((x ** 3 + 4) % P, (P - 1) // 2, P) == P - 1)
ENC_NONSQUARE = bytes([0x80 | (NONSQUARE_X >> 376)]) + (NONSQUARE_X & ((1 << 376) - 1)).to_bytes(47, "big")
ENC_TORSION = bytes([0x80]) + bytes(47)                      # x = 0, y = 2: on the curve, of order 3
ENC_INFSTRAY = bytes([0xC0]) + bytes(46) + b"\x01"           # the infinity flag with a stray bit


def ev(p, x):
    acc = 0
    for c in reversed(p):
        acc = (acc * x + c) % R
    return acc


def cols(polys):
    return np.frombuffer(b"".join(le(x) for p in polys for x in p), np.uint8).reshape(len(polys), len(polys[0]), 32)


def pts32(zs):
    return np.frombuffer(b"".join(le(z) for z in zs), np.uint8).reshape(len(zs), 32)


def as48(points96):
    return np.frombuffer(b"".join(compress(p) for p in points96), np.uint8).reshape(len(points96), 48)


@pytest.fixture(scope="module")
def ctx():
    from ark_ec_vrfs_amd import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def bases():
    """[tau^j] G, j < N_SRS, as 96-byte points"""
    out, t = [], 1
    for _ in range(N_SRS):
        out.append(co.g1_mul(t, G96))
        t = t * TAU % R
    return out


@pytest.fixture(scope="module")
def srs(ctx, bases):
    s = ctx.g1_srs_create(as48(bases))
    yield s
    s.close()


def groups(ctx, n, sets):
    g = ctx._lib.vrfhip_test_g1_msm_groups(ctx.handle, n, sets, 26)
    assert g > 0
    return g


# ------------------------------------------------------------------------------------------------ create
def test_create_size_bytes_and_refusals(ctx, bases, srs):
    from ark_ec_vrfs_amd import InvalidData, VrfHipError
    assert srs.size() == N_SRS and srs.bytes() == 128 * N_SRS
    good = [compress(b) for b in bases[:5]]
    for pos, enc in ((0, ENC_NONSQUARE), (2, ENC_TORSION), (4, ENC_INFSTRAY)):
        pts = list(good)
        pts[pos] = enc
        with pytest.raises(InvalidData) as e:
            ctx.g1_srs_create(np.frombuffer(b"".join(pts), np.uint8).reshape(-1, 48))
        assert e.value.status.tolist() == [2 if i == pos else 0 for i in range(5)]
    with pytest.raises(VrfHipError):
        ctx.g1_srs_create(np.zeros((0, 48), np.uint8))
    h = ctypes.c_void_p(1)                         # the C contract: no handle, the invalid-argument error
    bad = np.frombuffer(good[0] + ENC_TORSION, np.uint8)
    st = np.zeros(2, np.uint8)
    assert ctx._lib.vrfhip_g1_srs_create(ctx.handle, 2, bad.ctypes.data, st.ctypes.data, ctypes.byref(h)) == -1
    assert not h.value and st.tolist() == [0, 2]


def test_a_set_holding_infinity(ctx, bases):
    small = ctx.g1_srs_create(np.frombuffer(compress(bases[1]) + INF48 + compress(bases[2]), np.uint8).reshape(3, 48))
    assert small.size() == 3
    rnd = random.Random(3)
    p = [rnd.randrange(1, R) for _ in range(3)]
    out, xy, st = ctx.kzg_commit_batch(small, cols([p]))
    want = co.g1_add(co.g1_mul(p[0], bases[1]), co.g1_mul(p[2], bases[2]))
    assert st.tolist() == [0] and xy[0].tobytes() == want and out[0].tobytes() == compress(want)
    # an opening over it: q_1 meets the base at infinity
    z = rnd.randrange(R)
    q1, q0 = p[2], (p[1] + z * p[2]) % R
    v, pr, pxy, st = ctx.kzg_open_batch(small, cols([p]), pts32([z]))
    assert st.tolist() == [0] and int.from_bytes(v[0].tobytes(), "little") == ev(p, z) and q1
    assert pxy[0].tobytes() == co.g1_mul(q0, bases[1])
    small.close()


# ------------------------------------------------------------------------------------------------ commit
@pytest.fixture(scope="module")
def committed(ctx, srs):
    """every shape once: (k, len) -> (polys, out48, out_xy, status)"""
    res = {}
    for k, n in COMMIT_SHAPES:
        rnd = random.Random(k * 10000 + n)
        polys = [[rnd.randrange(R) for _ in range(n)] for _ in range(k)]
        res[(k, n)] = (polys,) + ctx.kzg_commit_batch(srs, cols(polys))
    return res


@pytest.mark.parametrize("shape", COMMIT_SHAPES)
def test_commit_equals_p_of_tau(committed, shape):
    polys, out, xy, st = committed[shape]
    assert not st.any()
    for c, p in enumerate(polys):
        want = mulG(ev(p, TAU))
        assert xy[c].tobytes() == want and out[c].tobytes() == compress(want), c


def test_shapes_cover_one_and_several_point_groups(ctx):
    g = {(k, n): groups(ctx, n, k) for k, n in COMMIT_SHAPES}
    assert any(v > 1 for v in g.values()) and any(v == 1 for v in g.values()), g


@pytest.mark.parametrize("first,n", [(0, 40), (1, 40), (255, N_SRS - 255)])
def test_commit_over_a_slice(ctx, srs, first, n):
    rnd = random.Random(first)
    polys = [[rnd.randrange(R) for _ in range(n)] for _ in range(2)]
    out, xy, st = ctx.kzg_commit_batch(srs, cols(polys), first=first)
    assert not st.any()
    for c, p in enumerate(polys):
        want = mulG(ev(p, TAU) * pow(TAU, first, R))
        assert xy[c].tobytes() == want and out[c].tobytes() == compress(want)


def test_commit_refusals_and_the_empty_column(ctx, srs):
    from ark_ec_vrfs_amd import VrfHipError
    one = cols([[1] * 10])
    for first in (N_SRS - 9, N_SRS, N_SRS + 1, 2 ** 63):
        with pytest.raises(VrfHipError):
            ctx.kzg_commit_batch(srs, one, first=first)
    with pytest.raises(VrfHipError):
        ctx.kzg_commit_batch(srs, np.zeros((0, 4, 32), np.uint8))
    out, xy, st = ctx.kzg_commit_batch(srs, one, first=N_SRS - 10)
    assert st.tolist() == [0]
    for first in (0, N_SRS):
        out, xy, st = ctx.kzg_commit_batch(srs, np.zeros((3, 0, 32), np.uint8), first=first)
        assert st.tolist() == [0, 0, 0] and all(o.tobytes() == INF48 for o in out) and not xy.any()


def test_commit_invalid_column_and_edge_scalars(ctx, srs):
    rnd = random.Random(11)
    n = 70
    polys = [[rnd.randrange(R) for _ in range(n)] for _ in range(4)]
    polys[1][33] = R
    polys[2] = [EDGE_SCALARS[j % len(EDGE_SCALARS)] for j in range(n)]
    polys[3][n - 1] = (1 << 256) - 1
    out, xy, st = ctx.kzg_commit_batch(srs, cols(polys))
    assert st.tolist() == [0, 2, 0, 2]
    for c in (1, 3):
        assert not out[c].any() and not xy[c].any()
    for c in (0, 2):
        want = mulG(ev(polys[c], TAU))
        assert xy[c].tobytes() == want and out[c].tobytes() == compress(want)


def test_unstructured_bases_meet_doubling_and_cancellation(ctx):
    rnd = random.Random(12)
    Pt, Q = co.g1_mul(rnd.randrange(1, R), G96), co.g1_mul(rnd.randrange(1, R), G96)
    pts = [Pt, Pt, neg96(Pt), INF, Q, Q, neg96(Q), Pt, INF, Q]
    small = ctx.g1_srs_create(as48(pts))
    s, t = rnd.randrange(1, R), rnd.randrange(1, R)
    columns = [[s] * len(pts), [s, s, s, t, t, t, t, s, s, t], [rnd.randrange(R) for _ in pts]]
    out, xy, st = ctx.kzg_commit_batch(small, cols(columns))
    assert not st.any()
    for c, col in enumerate(columns):
        want = INF
        for k, pt in zip(col, pts):
            if k and pt != INF:
                want = co.g1_add(want, co.g1_mul(k, pt))
        assert xy[c].tobytes() == want and out[c].tobytes() == compress(want), c
        assert ctx.g1_msm(np.frombuffer(b"".join(pts), np.uint8).reshape(-1, 96), cols([col])[0]) == want, c
    small.close()


# ------------------------------------------------------------------------------------------------ open
def proof_of(p, z):
    v = ev(p, z)
    return v, mulG((ev(p, TAU) - v) * pow((TAU - z) % R, -1, R))


@pytest.fixture(scope="module")
def opened(ctx, srs):
    """every length once: len -> (polys, zs, value, proof48, proof_xy, status); z in {0, 1, r - 1, a root, random}"""
    res = {}
    for n in OPEN_LENGTHS:
        rnd = random.Random(500 + n)
        p = [rnd.randrange(R) for _ in range(n)]
        root = rnd.randrange(R)
        pr = list(p)
        pr[0] = (p[0] - ev(p, root)) % R
        polys = [p, p, p, pr, [rnd.randrange(R) for _ in range(n)]]
        zs = [0, 1, R - 1, root, rnd.randrange(R)]
        res[n] = (polys, zs) + ctx.kzg_open_batch(srs, cols(polys), pts32(zs))
    return res


@pytest.mark.parametrize("n", OPEN_LENGTHS)
def test_open_value_and_proof(opened, n):
    polys, zs, v, pr, pxy, st = opened[n]
    assert not st.any()
    for c, (p, z) in enumerate(zip(polys, zs)):
        want_v, want_pi = proof_of(p, z)
        assert int.from_bytes(v[c].tobytes(), "little") == want_v, c
        assert pxy[c].tobytes() == want_pi and pr[c].tobytes() == compress(want_pi), c
    assert not v[3].any()                                            # opened at its root
    if n == 1:
        assert all(x.tobytes() == INF48 for x in pr)


def test_open_over_several_workgroups(ctx):
    """the chain over workgroups needs len > B * M = 4096, more bases than the shared set: [s^j] G with a small s, so that
    the bases come from additions"""
    n = 2 * B * M + 37
    pts, acc = [], G96
    for _ in range(n - 1):
        pts.append(acc)
        acc = co.g1_add(acc, G96)                                      # bases [j + 1] G: srs[j] = [j + 1] G
    big = ctx.g1_srs_create(as48(pts + [G96]))
    rnd = random.Random(77)
    polys = [[rnd.randrange(R) for _ in range(n)] for _ in range(2)]
    zs = [rnd.randrange(R), R - 1]
    v, pr, pxy, st = ctx.kzg_open_batch(big, cols(polys), pts32(zs))
    assert not st.any()
    for c, (p, z) in enumerate(zip(polys, zs)):
        q, carry = [0] * (n - 1), 0
        for j in range(n - 1, 0, -1):
            carry = (p[j] + z * carry) % R
            q[j - 1] = carry
        assert int.from_bytes(v[c].tobytes(), "little") == (p[0] + z * carry) % R
        assert pxy[c].tobytes() == mulG(sum((j + 1) * x for j, x in enumerate(q)))
    big.close()


@pytest.mark.parametrize("n", [3, B + 1, 2049])
def test_open_defects_and_edges(ctx, srs, n):
    rnd = random.Random(900 + n)
    p = [rnd.randrange(R) for _ in range(n)]
    bad = lambda j, x: p[:j] + [x] + p[j + 1:]
    top_zero = p[:max(1, n // 2)] + [0] * (n - max(1, n // 2))
    edge = [EDGE_SCALARS[j % len(EDGE_SCALARS)] for j in range(n)]
    polys = [p, bad(0, R), bad(n // 2, (1 << 256) - 1), bad(n - 1, R + 5), top_zero, [0] * n, edge, p]
    zs = [R] + [rnd.randrange(R) for _ in range(6)] + [(1 << 256) - 1]
    v, pr, pxy, st = ctx.kzg_open_batch(srs, cols(polys), pts32(zs))
    assert st.tolist() == [2, 2, 2, 2, 0, 0, 0, 2]
    for c in range(8):
        if st[c]:
            assert not v[c].any() and not pr[c].any() and not pxy[c].any(), c
        else:
            want_v, want_pi = proof_of(polys[c], zs[c])
            assert int.from_bytes(v[c].tobytes(), "little") == want_v and pxy[c].tobytes() == want_pi, c
            assert pr[c].tobytes() == compress(want_pi), c
    assert pr[5].tobytes() == INF48 and not v[5].any()                # the zero polynomial


def test_open_refusals(ctx, srs):
    from ark_ec_vrfs_amd import VrfHipError
    with pytest.raises(VrfHipError):
        ctx.kzg_open_batch(srs, np.zeros((1, 0, 32), np.uint8), pts32([1]))
    with pytest.raises(VrfHipError):
        ctx.kzg_open_batch(srs, np.zeros((1, N_SRS + 1, 32), np.uint8), pts32([1]))


# ------------------------------------------------------------------------------------------------ prover -> verifier
def test_commitments_and_openings_pass_the_checks(ctx, srs, committed, opened):
    vk = np.frombuffer(G96 + H192 + co.g2_mul(TAU, H192), np.uint8)
    n = 2049
    polys, zs, v, pr, _, _ = opened[n]
    c48, _, st = ctx.kzg_commit_batch(srs, cols(polys))
    assert not st.any()
    assert not ctx.kzg_check_batch(c48, pts32(zs), v, pr, vk).any()
    st, ok = ctx.kzg_check_batch_rlc(c48, pts32(zs), v, pr, vk, seed=bytes(range(32)))
    assert ok and not st.any()
    v1 = pts32([(int.from_bytes(x.tobytes(), "little") + 1) % R for x in v])
    assert ctx.kzg_check_batch(c48, pts32(zs), v1, pr, vk).tolist() == [1] * 5
    st, ok = ctx.kzg_check_batch_rlc(c48, pts32(zs), v1, pr, vk, seed=bytes(range(32)))
    assert not ok and st.tolist() == [1] * 5
    other = np.roll(pr, 1, axis=0)                                   # another polynomial's proof (items 0..2 share p: 3, 4 differ)
    st = ctx.kzg_check_batch(c48, pts32(zs), v, other, vk)
    assert st[0] == 1 and st[3] == 1 and st[4] == 1


def test_dev_forms_chain_on_one_stream(ctx, srs, opened):
    import torch
    vk = torch.from_numpy(np.frombuffer(G96 + H192 + co.g2_mul(TAU, H192), np.uint8).copy()).cuda()
    polys, zs, v, pr, pxy, _ = opened[2 * B + 1]
    k = len(polys)
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()
    u8 = lambda *s: torch.full(s, 0xEE, dtype=torch.uint8, device="cuda")
    d_co, d_z = dev(cols(polys)), dev(pts32(zs))
    c48, cxy, cst, val, p48, p96, pst, chk = u8(k, 48), u8(k, 96), u8(k), u8(k, 32), u8(k, 48), u8(k, 96), u8(k), u8(k)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ctx.kzg_commit_batch_dev(srs, d_co, c48, cst, out_xy=cxy)
        ctx.kzg_open_batch_dev(srs, d_co, d_z, val, p48, pst, proof_xy=p96)
        ctx.kzg_check_batch_dev(c48, d_z, val, p48, vk, chk)
    stream.synchronize()
    h48, hxy, hst = ctx.kzg_commit_batch(srs, cols(polys))
    assert (c48.cpu().numpy() == h48).all() and (cxy.cpu().numpy() == hxy).all() and not cst.cpu().numpy().any()
    assert (val.cpu().numpy() == v).all() and (p48.cpu().numpy() == pr).all() and (p96.cpu().numpy() == pxy).all()
    assert not pst.cpu().numpy().any() and not chk.cpu().numpy().any()
