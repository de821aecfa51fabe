"""GPU: vrfhip_kzg_check_batch* -- KZG openings from wire bytes, per item and as one batch -- against the native C oracle
(oracle.c_oracle: g1_mul / g1_add / g2_mul / pairing_check_batch / batch_digest), hashlib and Python integers.

Instances without polynomials: with a toy secret tau, g = [gamma] G1, h = G2, beta_h = [tau] h, an honest item is
C = [c] g, pi = [p] g, v = c - p (tau - z) mod r for random c, p, z: then (c - v + z p) - p tau = 0, which is the exponent of
e(C - v g + z pi, h) e(-pi, beta_h)."""
import hashlib
import random

import numpy as np
import pytest

from oracle import bls_oracle as bls
from oracle import c_oracle as co

P, R = bls.P, bls.R
INF, BAD96 = bytes(96), b"\xff" * 96
TAU, GAMMA = 0x1D0C7A5E2B9F4C6D8E1A3B5C7D9E0F123456789ABCDEF0123456789ABCDEF01 % R, 0xC0FFEE1234567
HONEST = ("honest", "zero", "const")
FALSE = ("v+1", "z+1", "otherC", "negpi", "swap")
INVALID = ("nonsquare", "torsion", "infstray", "z=r", "v>=r")
SEED = bytes(range(32))
SEED_A = np.frombuffer(SEED, np.uint8).copy()


def w48(x):
    return int(x).to_bytes(48, "little")


def xy96(pt):
    return INF if pt is None else w48(pt[0]) + w48(pt[1])


def neg96(b):
    return b if b == INF else b[:48] + w48((P - int.from_bytes(b[48:], "little")) % P)


def compress(b96):
    """96-byte affine point -> the 48-byte zcash / ark-bls12-381 form"""
    if b96 == INF:
        return bytes([0xC0]) + bytes(47)
    x, y = int.from_bytes(b96[:48], "little"), int.from_bytes(b96[48:], "little")
    out = bytearray(x.to_bytes(48, "big"))
    out[0] |= 0x80 | (0x20 if y > P - y else 0)
    return bytes(out)


G96 = co.g1_mul(GAMMA, xy96(bls.G1))
H192 = b"".join(w48(x) for x in (bls.G2[0].a, bls.G2[0].b, bls.G2[1].a, bls.G2[1].b))
VK = G96 + H192 + co.g2_mul(TAU, H192)
_rnd = random.Random(2025)
NONSQUARE_X = next(x for x in iter(lambda: _rnd.randrange(P), None) if pow((x ** 3 + 4) % P, (P - 1) // 2, P) == P - 1)
ENC_NONSQUARE = bytes([0x80 | (NONSQUARE_X >> 376)]) + (NONSQUARE_X & ((1 << 376) - 1)).to_bytes(47, "big")
ENC_TORSION = bytes([0x80]) + bytes(47)                      # x = 0, y = 2: on the curve, of order 3 (the codec tests' fixture)
ENC_INFSTRAY = bytes([0xC0]) + bytes(46) + b"\x01"           # the infinity flag with a stray bit


class Item:
    """c48 / pi48: the wire encodings; C / PI: the decoded points (None: the encoding is invalid); z, v: integers"""

    def __init__(self, c48, z, v, pi48, C, PI):
        self.c48, self.z, self.v, self.pi48, self.C, self.PI = c48, z, v, pi48, C, PI

    @property
    def valid(self):
        return self.C is not None and self.PI is not None and self.z < R and self.v < R


def make_item(kind, rnd, vk_g=G96):
    c, p, z = rnd.randrange(1, R), rnd.randrange(1, R), rnd.randrange(R)
    if kind == "zero":
        c = p = 0
    if kind == "const":
        p = 0
    v = (c - p * (TAU - z)) % R
    C, PI = co.g1_mul(c, vk_g), co.g1_mul(p, vk_g)
    if kind == "v+1": v = (v + 1) % R
    if kind == "z+1": z = (z + 1) % R
    if kind == "otherC": C = co.g1_mul((c + 5) % R, vk_g)
    if kind == "negpi": PI = neg96(PI)
    if kind == "swap": C, PI = PI, C
    it = Item(compress(C), z, v, compress(PI), C, PI)
    if kind == "nonsquare": it.c48, it.C = ENC_NONSQUARE, None
    if kind == "torsion": it.pi48, it.PI = ENC_TORSION, None
    if kind == "infstray": it.c48, it.C = ENC_INFSTRAY, None
    if kind == "z=r": it.z = R
    if kind == "v>=r": it.v = R + rnd.randrange(1 << 200)
    return it


def make_batch(kinds, seed):
    rnd = random.Random(seed)
    return [make_item(k, rnd) for k in kinds]


def mixed_kinds(n):
    """every kind in turn, invalid items at the first, a middle and the last position"""
    allk = HONEST + FALSE + INVALID
    kinds = [allk[(i + n) % len(allk)] for i in range(n)]
    if n >= 4:
        kinds[0], kinds[n // 2], kinds[n - 1] = INVALID[n % 5], INVALID[(n + 1) % 5], INVALID[(n + 2) % 5]
    return kinds


def honest_kinds(n):
    return [HONEST[i % 3] if i % 7 else "honest" for i in range(n)]


def arrays(items):
    u8 = lambda bs, w: np.frombuffer(b"".join(bs), np.uint8).reshape(-1, w).copy()
    le = lambda x: int(x).to_bytes(32, "little")
    return (u8([it.c48 for it in items], 48), u8([le(it.z) for it in items], 32), u8([le(it.v) for it in items], 32),
            u8([it.pi48 for it in items], 48))


def oracle_statuses(items, vk=VK):
    """co.pairing_check_batch on the oracle's own (A_i, -pi_i); an invalid item has no A_i: all-0xFF, which the oracle rejects"""
    g1 = []
    for it in items:
        if not it.valid:
            g1.append(BAD96 + BAD96)
            continue
        A = co.g1_add(co.g1_add(it.C, co.g1_mul((R - it.v) % R, vk[:96])), co.g1_mul(it.z, it.PI))
        g1.append(A + neg96(it.PI))
    return co.pairing_check_batch(np.frombuffer(b"".join(g1), np.uint8).reshape(-1, 192), np.frombuffer(vk[96:], np.uint8),
                                  shared=True)


def oracle_sums(items, seed, vk=VK):
    c, z, v, pi = arrays(items)
    root = co.batch_digest([c, z, v, pi], vk)
    sa, sb, rv = INF, INF, 0
    for i, it in enumerate(items):
        if not it.valid:
            continue
        r = int.from_bytes(hashlib.sha512(b"vrfhip-kzg-rlc-v1" + seed + root + i.to_bytes(8, "little")).digest()[:16], "little")
        sa = co.g1_add(sa, co.g1_add(co.g1_mul(r, it.C), co.g1_mul(r * it.z % R, it.PI)))
        sb = co.g1_add(sb, co.g1_mul(r, it.PI))
        rv += r * it.v
    return co.g1_add(sa, co.g1_mul((-rv) % R, vk[:96])) + neg96(sb)


def rlc_dev(ctx, items, vk=VK, seed=SEED, want_sums=True):
    """-> (status (n,), verdict, sums 192 bytes)"""
    import torch
    c, z, v, pi = (torch.from_numpy(a).cuda() for a in arrays(items))
    d_vk = torch.from_numpy(np.frombuffer(vk, np.uint8).copy()).cuda()
    st = torch.full((len(items),), 0x5A, dtype=torch.uint8, device="cuda")
    verdict = torch.full((1,), 0x5A, dtype=torch.uint8, device="cuda")
    sums = torch.full((192,), 0x5A, dtype=torch.uint8, device="cuda") if want_sums else None
    ctx.kzg_check_batch_rlc_dev(c, z, v, pi, d_vk, st, verdict, seed, sums=sums)
    torch.cuda.synchronize()
    return st.cpu().numpy(), int(verdict.cpu()[0]), (sums.cpu().numpy().tobytes() if want_sums else None)


def item_dev(ctx, items, vk=VK):
    import torch
    c, z, v, pi = (torch.from_numpy(a).cuda() for a in arrays(items))
    d_vk = torch.from_numpy(np.frombuffer(vk, np.uint8).copy()).cuda()
    st = torch.full((len(items),), 0x5A, dtype=torch.uint8, device="cuda")
    ctx.kzg_check_batch_dev(c, z, v, pi, d_vk, st)
    torch.cuda.synchronize()
    return st.cpu().numpy()


def test_oracle_instances_are_what_they_claim():
    """CPU: the instance builder against the oracle -- honest kinds hold, false kinds fail, invalid kinds are invalid"""
    items = make_batch(HONEST + FALSE + INVALID, 1)
    assert list(oracle_statuses(items)) == [0] * 3 + [1] * 5 + [2] * 5
    assert items[1].C == INF and items[1].PI == INF and items[1].v == 0 and items[2].PI == INF


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 4, 5, 33])
def test_gpu_per_item_form_equals_the_oracle(ctx, n):
    batches = [make_batch(mixed_kinds(n), n)] if n > 1 else [make_batch([k], 10 + j) for j, k in enumerate(("honest", "v+1", "nonsquare", "zero"))]
    for items in batches:
        want = oracle_statuses(items)
        got = ctx.kzg_check_batch(*arrays(items), VK)
        assert list(got) == list(want)
        assert list(item_dev(ctx, items)) == list(want)
    if n == 33:
        assert set(want) == {0, 1, 2}


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 33, 128, 129, 300])
def test_gpu_batched_dev_form(ctx, n):
    honest = make_batch(honest_kinds(n), 100 + n)
    st, verdict, sums = rlc_dev(ctx, honest)
    assert verdict == 0 and not st.any()
    base_sums = sums
    if n <= 129:
        assert sums == oracle_sums(honest, SEED)
    # invalid items are left out: they get 2 and the verdict stays 0
    kinds = honest_kinds(n)
    for j, pos in enumerate(sorted({0, n // 3, n // 2, 2 * n // 3, n - 1}) if n >= 4 else [0]):
        kinds[pos] = INVALID[(j + n) % 5]
    with_invalid = make_batch(kinds, 200 + n)
    st, verdict, sums = rlc_dev(ctx, with_invalid)
    assert verdict == 0 and list(st) == [0 if it.valid else 2 for it in with_invalid] and (st == 2).sum() >= 1
    if n <= 129:
        assert sums == oracle_sums(with_invalid, SEED)
    # one changed byte of any array, of vk or of the seed changes the sums.  The four array cases change a point or a scalar
    # that enters the sums itself, so they show only that the byte is read; that it is read into the WEIGHTS is pinned by the
    # equality with oracle_sums above and by the cases after them, whose changed byte reaches the sums through the digest alone
    for which in range(4):
        mod = make_batch(honest_kinds(n), 100 + n)
        it = mod[n // 2]
        if which == 0: it.c48 = it.c48[:47] + bytes([it.c48[47] ^ 1])
        if which == 1: it.z ^= 1 << 100
        if which == 2: it.v ^= 1 << 100
        if which == 3: it.pi48 = it.pi48[:47] + bytes([it.pi48[47] ^ 1])
        assert rlc_dev(ctx, mod)[2] != base_sums, which
    if n >= 3:
        mod = make_batch(honest_kinds(n), 100 + n)
        assert mod[2].PI == INF                                # a constant polynomial: z multiplies infinity,
        mod[2].z ^= 1                                          # so it reaches the sums through the digest only
        assert rlc_dev(ctx, mod)[2] != base_sums
    vk2 = VK[:479] + bytes([VK[479] ^ 1])                      # a byte of beta_h: the sums do not use it but through the digest
    assert rlc_dev(ctx, honest, vk=vk2)[2] != base_sums
    assert rlc_dev(ctx, honest, seed=SEED[:31] + b"\x00")[2] != base_sums
    # each false kind, and two opposite errors that cancel under equal weights
    for j, kind in enumerate(FALSE):
        kinds = honest_kinds(n)
        kinds[(j * 7 + 3) % n] = kind
        st, verdict, _ = rlc_dev(ctx, make_batch(kinds, 300 + n), want_sums=False)
        assert verdict == 1 and not st.any(), kind
    if n >= 2:
        two = make_batch(["honest"] * n, 400 + n)
        a, b, delta = 0, n - 1, 12345
        two[a].v, two[b].v = (two[a].v + delta) % R, (two[b].v - delta) % R
        assert rlc_dev(ctx, two, want_sums=False)[1] == 1
    # an invalid key
    off_g = G96[:48] + w48((int.from_bytes(G96[48:], "little") + 1) % P)
    flip = lambda k, at: k[:at] + bytes([k[at] ^ 1]) + k[at + 1:]
    for bad_vk in (off_g + VK[96:], flip(VK, 96 + 5), flip(VK, 288 + 5), BAD96 + VK[96:]):
        assert rlc_dev(ctx, honest, vk=bad_vk, want_sums=False)[1] == 2


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 33, 128, 129, 300])
def test_gpu_batched_host_form_equals_the_per_item_form(ctx, n):
    cases = [(honest_kinds(n), True)]
    kinds = honest_kinds(n)
    kinds[n // 2] = INVALID[n % 5]
    cases.append((list(kinds), True))
    kinds[(n // 2 + 1) % n] = FALSE[n % 5]
    cases.append((list(kinds), False))
    if n >= 4:
        cases.append((mixed_kinds(n), False))
    for j, (kinds, ok) in enumerate(cases):
        items = make_batch(kinds, 500 + 10 * n + j)
        want = ctx.kzg_check_batch(*arrays(items), VK)
        got, batch_ok = ctx.kzg_check_batch_rlc(*arrays(items), VK, seed=SEED)
        assert list(got) == list(want) and batch_ok == ok, j
        if n <= 33:
            assert list(want) == list(oracle_statuses(items))
    if n >= 2:
        two = make_batch(["honest"] * n, 400 + n)
        two[0].v, two[n - 1].v = (two[0].v + 12345) % R, (two[n - 1].v - 12345) % R
        got, batch_ok = ctx.kzg_check_batch_rlc(*arrays(two), VK, seed=SEED)
        assert not batch_ok and list(got) == [1] + [0] * (n - 2) + [1]


@pytest.mark.gpu
def test_gpu_invalid_key_makes_every_item_invalid_data(ctx):
    """per-item form, host and _dev, and the host batched form (verdict 2 -> per-item fallback): g off the curve, a coordinate
    of g >= p, h off its curve, beta_h off its curve -- every status 2, the invalid item's included, and batch_ok false"""
    items = make_batch(["honest", "const", "v+1", "nonsquare", "zero"], 88)
    off_g = G96[:48] + w48((int.from_bytes(G96[48:], "little") + 1) % P)
    flip = lambda k, at: k[:at] + bytes([k[at] ^ 1]) + k[at + 1:]
    for bad_vk in (off_g + VK[96:], BAD96 + VK[96:], flip(VK, 96 + 5), flip(VK, 288 + 5)):
        if bad_vk[:96] == G96:                                 # the oracle judges (h, beta_h) itself; it has no A_i for a bad g
            assert list(oracle_statuses(items, bad_vk)) == [2] * 5
        assert list(ctx.kzg_check_batch(*arrays(items), bad_vk)) == [2] * 5
        assert list(item_dev(ctx, items, bad_vk)) == [2] * 5
        got, batch_ok = ctx.kzg_check_batch_rlc(*arrays(items), bad_vk, seed=SEED)
        assert list(got) == [2] * 5 and not batch_ok
    assert list(ctx.kzg_check_batch(*arrays(items), VK)) == [0, 0, 1, 2, 0]               # the good key still answers


@pytest.fixture(scope="module")
def large():
    """1025 honest items with c and p in arithmetic progressions: C_i and pi_i come from g1_add chains"""
    n, rnd = 1025, random.Random(1025)
    c0, dc, p0, dp = (rnd.randrange(1, R) for _ in range(4))
    C, PI = co.g1_mul(c0, G96), co.g1_mul(p0, G96)
    DC, DP = co.g1_mul(dc, G96), co.g1_mul(dp, G96)
    items = []
    for i in range(n):
        c, p, z = (c0 + i * dc) % R, (p0 + i * dp) % R, rnd.randrange(R)
        items.append(Item(compress(C), z, (c - p * (TAU - z)) % R, compress(PI), C, PI))
        C, PI = co.g1_add(C, DC), co.g1_add(PI, DP)
    return items


@pytest.mark.gpu
def test_gpu_one_larger_batch(ctx, large):
    """1025 items: nine prep blocks, and the fold's strided pass and tree"""
    n = len(large)
    st, verdict, _ = rlc_dev(ctx, large, want_sums=False)
    assert verdict == 0 and not st.any()
    got, batch_ok = ctx.kzg_check_batch_rlc(*arrays(large), VK, seed=SEED)
    assert batch_ok and not got.any()
    it = large[n - 1]
    false_last = large[:n - 1] + [Item(it.c48, it.z, (it.v + 1) % R, it.pi48, it.C, it.PI)]
    st, verdict, _ = rlc_dev(ctx, false_last, want_sums=False)
    assert verdict == 1 and not st.any()
    got, batch_ok = ctx.kzg_check_batch_rlc(*arrays(false_last), VK, seed=SEED)
    assert not batch_ok and list(got) == [0] * (n - 1) + [1]


@pytest.mark.gpu
def test_gpu_argument_rules(ctx):
    import ctypes
    import torch
    from ark_ec_vrfs_amd import Context, Secp256r1Sha256Tai, _lib
    lib, h = _lib.load(), ctx._h
    e = lambda w: np.empty((0, w), np.uint8)
    # n = 0 touches nothing
    assert ctx.kzg_check_batch(e(48), e(32), e(32), e(48), VK).shape == (0,)
    st, ok = ctx.kzg_check_batch_rlc(e(48), e(32), e(32), e(48), VK, seed=SEED)
    assert st.shape == (0,) and ok
    assert lib.vrfhip_kzg_check_batch(h, 0, None, None, None, None, None, None) == 0
    assert lib.vrfhip_kzg_check_batch_dev(h, 0, None, None, None, None, None, None, None) == 0
    verdict = torch.full((1,), 0x5A, dtype=torch.uint8, device="cuda")
    assert lib.vrfhip_kzg_check_batch_rlc_dev(h, 0, None, None, None, None, None, SEED_A.ctypes.data, None, verdict.data_ptr(), None, None) == 0
    torch.cuda.synchronize()
    assert int(verdict.cpu()[0]) == 0
    # NULLs
    items = make_batch(["honest", "v+1"], 7)
    c, z, v, pi = arrays(items)
    vk = np.frombuffer(VK, np.uint8).copy()
    st = np.zeros(2, np.uint8)
    okf = ctypes.c_int32(1)
    args = [a.ctypes.data for a in (c, z, v, pi, vk, st)]
    for j in range(6):
        a = list(args)
        a[j] = None
        assert lib.vrfhip_kzg_check_batch(h, 2, *a) == -1, j
        assert lib.vrfhip_kzg_check_batch_rlc(h, 2, *a[:5], SEED_A.ctypes.data, a[5], ctypes.byref(okf)) == -1, j
    assert lib.vrfhip_kzg_check_batch_rlc(h, 2, *args[:5], None, args[5], ctypes.byref(okf)) == -1
    assert lib.vrfhip_kzg_check_batch_rlc(h, 2, *args[:5], SEED_A.ctypes.data, args[5], None) == 0 and list(st) == [0, 1]
    assert lib.vrfhip_kzg_check_batch(None, 2, *args) == -1
    d = [torch.from_numpy(a).cuda() for a in (c, z, v, pi, vk, st)]
    dp = [t.data_ptr() for t in d]
    assert lib.vrfhip_kzg_check_batch_rlc_dev(h, 2, *dp[:5], SEED_A.ctypes.data, dp[5], None, None, None) == -1
    assert lib.vrfhip_kzg_check_batch_rlc_dev(h, 2, *dp[:5], None, dp[5], verdict.data_ptr(), None, None) == -1
    assert lib.vrfhip_kzg_check_batch_dev(h, 2, dp[0], None, dp[2], dp[3], dp[4], dp[5], None) == -1
    assert lib.vrfhip_kzg_check_batch_dev(h, (1 << 28) + 1, *dp, None) == -1
    # a secp256r1 context is refused
    other = Context(0, Secp256r1Sha256Tai)
    try:
        assert lib.vrfhip_kzg_check_batch(other._h, 2, *args) == -5
        assert lib.vrfhip_kzg_check_batch_rlc(other._h, 2, *args[:5], SEED_A.ctypes.data, args[5], ctypes.byref(okf)) == -5
        assert lib.vrfhip_kzg_check_batch_dev(other._h, 2, *dp, None) == -5
        assert lib.vrfhip_kzg_check_batch_rlc_dev(other._h, 2, *dp[:5], SEED_A.ctypes.data, dp[5], verdict.data_ptr(), None, None) == -5
    finally:
        other.close()


@pytest.mark.gpu
def test_gpu_two_keys_on_one_context(ctx):
    """the prepared lines of (h, beta_h) are cached in the context: a second key must replace them, and the first come back"""
    tau2 = (TAU * 7 + 11) % R
    vk2 = G96 + H192 + co.g2_mul(tau2, H192)
    items = make_batch(["honest", "const", "v+1", "honest"], 77)
    for _ in range(2):
        assert list(ctx.kzg_check_batch(*arrays(items), VK)) == [0, 0, 1, 0]
        # under the other secret only the constant polynomial (pi = infinity) still opens
        want2 = list(oracle_statuses(items, vk2))
        assert want2 == [1, 0, 1, 1]
        assert list(ctx.kzg_check_batch(*arrays(items), vk2)) == want2
        got, ok = ctx.kzg_check_batch_rlc(*arrays(items[:2]), VK, seed=SEED)
        assert ok and list(got) == [0, 0]
        got, ok = ctx.kzg_check_batch_rlc(*arrays(items[:2]), vk2, seed=SEED)
        assert not ok and list(got) == [1, 0]
