"""GPU: vrfhip_kzg_multi_check_batch* -- multi-commitment, multi-point KZG openings, per item and as one batch -- against the
native C oracle (oracle.c_oracle: g1_mul / g1_add / g2_mul / pairing_check_batch / batch_digest), hashlib and Python integers.

Instances without polynomials: with toy secrets tau and gamma, g = [gamma] G1, h = G2, beta_h = [tau] h, all points are
multiples of g -- C_ij = [c_ij] g, S_j = [sigma_j] g, pi_ij = [q_ij] g -- with random s, u, z and t_ij (j >= 1), and t_i0 is
chosen so that the exponent of e(A_i, h) e(B_i, beta_h) over e(g, h),
    sum s c + sum_{j>=1} t sigma + t_i0 + sum u z q - tau sum u q,
is zero."""
import hashlib
import random

import numpy as np
import pytest

from oracle import bls_oracle as bls
from oracle import c_oracle as co

import test_kzg_check as single                      # the single-point file: its key, encodings and mixed batch

P, R = bls.P, bls.R
INF, BAD96 = single.INF, single.BAD96
TAU, G96, VK = single.TAU, single.G96, single.VK
w48, neg96, compress = single.w48, single.neg96, single.compress
SEED = bytes(range(32))
TAG = b"vrfhip-kzg-multi-rlc-v1"
SHAPES = [(1, 0, 1), (5, 3, 2), (0, 0, 1), (11, 2, 2)]
RING = (5, 3, 2)
le = lambda x: int(x).to_bytes(32, "little")

_rnd = random.Random(532)
SIGMA = [_rnd.randrange(1, R) for _ in range(3)]
SHARED = [co.g1_mul(s, G96) for s in SIGMA]           # S_1 .. S_3
# multiples of g to draw commitments and proofs from: entry 0 is infinity
POOL = [(0, INF)] + [(e, co.g1_mul(e, G96)) for e in (_rnd.randrange(1, R) for _ in range(23))]

HONEST = ("honest", "allinf", "piinf", "zero_s")
FALSE = ("s+1", "t+1", "z+1", "u+1", "otherC", "negpi", "swappi")
BAD_ENC = {"nonsquare": single.ENC_NONSQUARE, "torsion": single.ENC_TORSION, "infstray": single.ENC_INFSTRAY}
INVALID = tuple(BAD_ENC) + ("s=r", "t=r", "z=r", "u=r")


def shared_bytes(shape):
    return b"".join(SHARED[:shape[1]])


class Item:
    """c48 / pi48: lists of wire encodings; C / PI: the decoded points (None: the encoding is invalid); s, t, z, u: integers"""

    def __init__(self, C, s, t, PI, z, u):
        self.C, self.s, self.t, self.PI, self.z, self.u = list(C), list(s), list(t), list(PI), list(z), list(u)
        self.c48, self.pi48 = [compress(x) for x in C], [compress(x) for x in PI]

    @property
    def valid(self):
        return None not in self.C and None not in self.PI and all(x < R for x in self.s + self.t + self.z + self.u)


def make_item(kind, shape, rnd, where=0):
    """where: 0 / -1 = an invalid encoding goes to the first / the last term of the item (its terms: commitments, then proofs)"""
    k, m, p = shape
    nz = lambda: rnd.randrange(1, len(POOL))
    ci, qi = [nz() for _ in range(k)], rnd.sample(range(1, len(POOL)), p)          # distinct non-trivial proofs
    if kind == "allinf": ci, qi = [0] * k, [0] * p
    if kind == "piinf": qi = [0] * p
    s, u, z = ([rnd.randrange(1, R) for _ in range(c)] for c in (k, p, p))
    if kind == "zero_s" and k: s[0] = 0
    t = [0] + [rnd.randrange(R) for _ in range(m)]
    c, q = [POOL[i][0] for i in ci], [POOL[i][0] for i in qi]
    t[0] = -(sum(a * b for a, b in zip(s, c)) + sum(a * b for a, b in zip(t[1:], SIGMA)) +
             sum(a * b * d for a, b, d in zip(u, z, q)) - TAU * sum(a * b for a, b in zip(u, q))) % R
    C, PI = [POOL[i][1] for i in ci], [POOL[i][1] for i in qi]
    if kind in ("s+1", "otherC", "s=r") and not k: kind = "t" + kind[1:] if kind != "otherC" else "t+1"
    if kind == "swappi" and p < 2: kind = "negpi"
    if kind == "s+1": s[-1] = (s[-1] + 1) % R
    if kind == "t+1": t[m] = (t[m] + 1) % R
    if kind == "z+1": z[0] = (z[0] + 1) % R
    if kind == "u+1": u[-1] = (u[-1] + 1) % R
    if kind == "otherC": C[k // 2] = co.g1_mul((c[k // 2] + 5) % R, G96)
    if kind == "negpi": PI[0] = neg96(PI[0])
    if kind == "swappi": PI[0], PI[1] = PI[1], PI[0]
    it = Item(C, s, t, PI, z, u)
    if kind in BAD_ENC:
        first_is_c = k > 0 and where == 0
        enc, dec, at = (it.c48, it.C, 0) if first_is_c else (it.pi48, it.PI, 0 if where == 0 else p - 1)
        enc[at], dec[at] = BAD_ENC[kind], None
    if kind == "s=r": it.s[0] = R
    if kind == "t=r": it.t[m // 2] = R
    if kind == "z=r": it.z[p - 1] = R
    if kind == "u=r": it.u[0] = R
    return it


def make_batch(kinds, shape, seed):
    rnd = random.Random(seed)
    return [make_item(kd, shape, rnd, where=-(i % 2)) for i, kd in enumerate(kinds)]


def honest_kinds(n):
    return [HONEST[i % 4] if i % 7 else "honest" for i in range(n)]


def mixed_kinds(n):
    """every kind in turn, invalid items at the first, a middle and the last position"""
    allk = HONEST + FALSE + INVALID
    kinds = [allk[(i + n) % len(allk)] for i in range(n)]
    if n >= 4:
        kinds[0], kinds[n // 2], kinds[n - 1] = INVALID[n % 7], INVALID[(n + 1) % 7], INVALID[(n + 2) % 7]
    return kinds


def arrays(items, shape):
    """the seven arrays in the order of the entry points: None for one whose count is 0"""
    k, m, p = shape
    n = len(items)
    u8 = lambda rows, cnt, w: None if cnt == 0 else np.frombuffer(b"".join(rows), np.uint8).reshape(n, cnt, w).copy()
    return [u8([x for it in items for x in it.c48], k, 48), u8([le(x) for it in items for x in it.s], k, 32),
            None if m == 0 else np.frombuffer(shared_bytes(shape), np.uint8).reshape(m, 96).copy(),
            u8([le(x) for it in items for x in it.t], m + 1, 32), u8([x for it in items for x in it.pi48], p, 48),
            u8([le(x) for it in items for x in it.z], p, 32), u8([le(x) for it in items for x in it.u], p, 32)]


def lincomb(terms):
    acc = INF
    for scalar, pt in terms:
        if scalar % R and pt != INF:
            acc = co.g1_add(acc, co.g1_mul(scalar % R, pt))
    return acc


def oracle_statuses(items, shape, vk=VK, shared=None):
    """co.pairing_check_batch on the oracle's own (A_i, B_i); an invalid item has none: all-0xFF, which the oracle rejects"""
    bases = [vk[:96]] + (SHARED[:shape[1]] if shared is None else shared)
    g1 = []
    for it in items:
        if not it.valid:
            g1.append(BAD96 + BAD96)
            continue
        A = lincomb(list(zip(it.s, it.C)) + list(zip(it.t, bases)) + [(u * z, pi) for u, z, pi in zip(it.u, it.z, it.PI)])
        g1.append(A + neg96(lincomb(list(zip(it.u, it.PI)))))
    return co.pairing_check_batch(np.frombuffer(b"".join(g1), np.uint8).reshape(-1, 192), np.frombuffer(vk[96:], np.uint8),
                                  shared=True)


def oracle_sums(items, shape, seed, vk=VK):
    """S_A || S_B restated: the digest over the arrays as they arrive, the weights, the sums"""
    k, m, p = shape
    a = arrays(items, shape)
    root = co.batch_digest([x.reshape(len(items), -1) for j, x in enumerate(a) if j != 2 and x is not None],
                           vk + shared_bytes(shape))
    pre = TAG + b"".join(x.to_bytes(4, "little") for x in shape) + seed + root
    ta, tb, cols = [], [], [0] * (m + 1)
    for i, it in enumerate(items):
        if not it.valid:
            continue
        r = int.from_bytes(hashlib.sha512(pre + i.to_bytes(8, "little")).digest()[:16], "little")
        ta += [(r * s, C) for s, C in zip(it.s, it.C)] + [(r * u * z, pi) for u, z, pi in zip(it.u, it.z, it.PI)]
        tb += [(r * u, pi) for u, pi in zip(it.u, it.PI)]
        cols = [c + r * t for c, t in zip(cols, it.t)]
    return lincomb(ta + list(zip(cols, [vk[:96]] + SHARED[:m]))) + neg96(lincomb(tb))


def dev_tensors(items, shape, vk, shared=None):
    import torch
    a = arrays(items, shape)
    if shared is not None:
        a[2] = np.frombuffer(b"".join(shared), np.uint8).reshape(-1, 96).copy()
    t = [None if x is None else torch.from_numpy(x).cuda() for x in a]
    return t + [torch.from_numpy(np.frombuffer(vk, np.uint8).copy()).cuda()]


def rlc_dev(ctx, items, shape, vk=VK, seed=SEED, want_sums=True, shared=None):
    """-> (status (n,), verdict, sums 192 bytes)"""
    import torch
    st = torch.full((len(items),), 0x5A, dtype=torch.uint8, device="cuda")
    verdict = torch.full((1,), 0x5A, dtype=torch.uint8, device="cuda")
    sums = torch.full((192,), 0x5A, dtype=torch.uint8, device="cuda") if want_sums else None
    ctx.kzg_multi_check_batch_rlc_dev(*dev_tensors(items, shape, vk, shared), st, verdict, seed, sums=sums)
    torch.cuda.synchronize()
    return st.cpu().numpy(), int(verdict.cpu()[0]), (sums.cpu().numpy().tobytes() if want_sums else None)


def item_dev(ctx, items, shape, vk=VK, shared=None):
    import torch
    st = torch.full((len(items),), 0x5A, dtype=torch.uint8, device="cuda")
    ctx.kzg_multi_check_batch_dev(*dev_tensors(items, shape, vk, shared), st)
    torch.cuda.synchronize()
    return st.cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES)
def test_oracle_instances_are_what_they_claim(shape):
    """CPU: the instance builder against the oracle -- honest kinds hold, false kinds fail, invalid kinds are invalid, with the
    invalid encodings at the first (where = 0) and the last (where = -1) term"""
    kinds = HONEST + FALSE + INVALID + INVALID
    rnd = random.Random(1)
    items = [make_item(kd, shape, rnd, where=0 if j < len(kinds) - len(INVALID) else -1) for j, kd in enumerate(kinds)]
    assert list(oracle_statuses(items, shape)) == [0] * 4 + [1] * 7 + [2] * 14
    assert all(x == INF for x in items[1].C + items[1].PI + items[2].PI)
    k, p = shape[0], shape[2]
    first, last = items[11], items[18]                                     # "nonsquare" at the first and at the last term
    assert (first.C[0] if k else first.PI[0]) is None and last.PI[p - 1] is None
    if k:
        assert items[3].s[0] == 0 and items[3].C[0] != INF                 # a zero scalar on a non-trivial commitment


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("n", [1, 4, 5, 33])
def test_gpu_per_item_form_equals_the_oracle(ctx, n, shape):
    batches = [make_batch(mixed_kinds(n), shape, n)] if n > 1 else \
        [make_batch([kd], shape, 10 + j) for j, kd in enumerate(("honest", "t+1", "nonsquare", "allinf"))]
    for items in batches:
        want = oracle_statuses(items, shape)
        assert list(ctx.kzg_multi_check_batch(*arrays(items, shape), VK)) == list(want)
        assert list(item_dev(ctx, items, shape)) == list(want)
    if n == 33:
        assert set(want) == {0, 1, 2}


def flip_byte(a, at):
    a.reshape(-1)[at] ^= 1


@pytest.mark.gpu
@pytest.mark.parametrize("n,shape", [(n, RING) for n in (1, 2, 33, 128, 129, 300)] +
                         [(n, sh) for sh in SHAPES if sh != RING for n in (2, 129)])
def test_gpu_batched_dev_form(ctx, n, shape):
    k, m, p = shape
    honest = make_batch(honest_kinds(n), shape, 100 + n)
    st, verdict, base_sums = rlc_dev(ctx, honest, shape)
    assert verdict == 0 and not st.any()
    if n <= 129:
        assert base_sums == oracle_sums(honest, shape, SEED)
    # invalid items are left out: they get 2 and the verdict stays 0
    kinds = honest_kinds(n)
    for j, pos in enumerate(sorted({0, n // 3, n // 2, 2 * n // 3, n - 1}) if n >= 4 else [0]):
        kinds[pos] = INVALID[(j + n) % 7]
    with_invalid = make_batch(kinds, shape, 200 + n)
    st, verdict, sums = rlc_dev(ctx, with_invalid, shape)
    assert verdict == 0 and list(st) == [0 if it.valid else 2 for it in with_invalid] and (st == 2).sum() >= 1
    if n <= 129:
        assert sums == oracle_sums(with_invalid, shape, SEED)
    # each false kind, and two opposite errors that cancel under equal weights
    for j, kind in enumerate(FALSE):
        kinds = honest_kinds(n)
        kinds[(j * 7 + 3) % n] = kind
        st, verdict, _ = rlc_dev(ctx, make_batch(kinds, shape, 300 + n), shape, want_sums=False)
        assert verdict == 1 and not st.any(), kind
    if n >= 2:
        two = make_batch(["honest"] * n, shape, 400 + n)
        two[0].t[0], two[n - 1].t[0] = (two[0].t[0] + 12345) % R, (two[n - 1].t[0] - 12345) % R
        assert rlc_dev(ctx, two, shape, want_sums=False)[1] == 1
    # an invalid key or shared base
    off = lambda b: b[:48] + w48((int.from_bytes(b[48:], "little") + 1) % P)
    flip = lambda key, at: key[:at] + bytes([key[at] ^ 1]) + key[at + 1:]
    for bad_vk in (off(G96) + VK[96:], flip(VK, 96 + 5), flip(VK, 288 + 5), BAD96 + VK[96:]):
        st, verdict, sums = rlc_dev(ctx, honest, shape, vk=bad_vk)
        assert verdict == 2
        if bad_vk[:96] != G96:
            assert sums == BAD96 + BAD96
    for at in range(m):
        for bad in (off(SHARED[at]), BAD96):
            st, verdict, sums = rlc_dev(ctx, honest, shape, shared=SHARED[:at] + [bad] + SHARED[at + 1:m])
            assert verdict == 2 and sums == BAD96 + BAD96


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 129])
def test_gpu_every_byte_reaches_the_sums(ctx, n):
    """one changed byte in any of the six arrays, in shared_bases, in beta_h or in the seed changes the sums.  A changed point
    or scalar enters the sums itself, which shows only that the byte is read; that it is read into the WEIGHTS is pinned by the
    equality with oracle_sums in the test above and by the cases here whose byte reaches the sums through the digest alone:
    z and u of a proof at infinity, and beta_h"""
    import torch
    shape = RING
    items = make_batch(["honest", "piinf"] * (n // 2) + ["honest"] * (n % 2), shape, 600 + n)
    base = rlc_dev(ctx, items, shape)[2]

    def run(mod=None, vk=VK, seed=SEED, shared=None):
        t = dev_tensors(items, shape, vk, shared)
        if mod:
            j, at = mod
            t[j].view(-1)[at] ^= 1
        st = torch.zeros(n, dtype=torch.uint8, device="cuda")
        verdict, sums = torch.zeros(1, dtype=torch.uint8, device="cuda"), torch.zeros(192, dtype=torch.uint8, device="cuda")
        ctx.kzg_multi_check_batch_rlc_dev(*t, st, verdict, seed, sums=sums)
        torch.cuda.synchronize()
        return sums.cpu().numpy().tobytes()

    last = n - 1 if (n - 1) % 2 == 0 else n - 2       # an honest item with non-trivial points
    k, m, p = shape
    assert run((0, (last * k + 2) * 48 + 47)) != base                 # commitments48: the low byte of x (InvalidData or another point)
    assert run((1, (last * k + 1) * 32 + 12)) != base                 # scalars32
    assert run((3, (last * (m + 1) + 2) * 32 + 12)) != base           # shared_scalars32
    assert run((4, (last * p + 1) * 48 + 47)) != base                 # proofs48
    assert run((5, (last * p) * 32 + 12)) != base                     # points32
    assert run((6, (last * p + 1) * 32 + 12)) != base                 # coefs32
    assert run((5, (1 * p + 1) * 32 + 3)) != base                     # z of a proof at infinity: through the digest only
    assert run((6, (1 * p) * 32 + 3)) != base                         # u of a proof at infinity: likewise
    assert run((2, 96 + 1)) != base                                   # shared_bases (S_2 off its curve: all-0xFF sums)
    assert run(vk=VK[:479] + bytes([VK[479] ^ 1])) != base            # beta_h: through the digest only
    assert run(seed=SEED[:31] + b"\x00") != base
    assert run() == base


@pytest.mark.gpu
def test_gpu_empty_batch(ctx):
    import torch
    for shape in SHAPES:
        st, verdict, sums = rlc_dev(ctx, [], shape)
        assert st.shape == (0,) and verdict == 0 and sums == INF + INF
        assert item_dev(ctx, [], shape).shape == (0,)
        a = arrays([], shape)
        assert ctx.kzg_multi_check_batch(*a, VK).shape == (0,)
        st, ok = ctx.kzg_multi_check_batch_rlc(*a, VK, seed=SEED)
        assert st.shape == (0,) and ok


@pytest.mark.gpu
@pytest.mark.parametrize("n,shape", [(n, RING) for n in (1, 2, 33, 129, 300)] + [(33, sh) for sh in SHAPES if sh != RING])
def test_gpu_batched_host_form_equals_the_per_item_form(ctx, n, shape):
    cases = [(honest_kinds(n), True)]
    kinds = honest_kinds(n)
    kinds[n // 2] = INVALID[n % 7]
    cases.append((list(kinds), True))
    kinds[(n // 2 + 1) % n] = FALSE[n % 7]
    cases.append((list(kinds), False))
    if n >= 4:
        cases.append((mixed_kinds(n), False))
    for j, (kinds, ok) in enumerate(cases):
        items = make_batch(kinds, shape, 500 + 10 * n + j)
        a = arrays(items, shape)
        want = ctx.kzg_multi_check_batch(*a, VK)
        got, batch_ok = ctx.kzg_multi_check_batch_rlc(*a, VK, seed=SEED)
        assert list(got) == list(want) and batch_ok == ok, j
        if n <= 33:
            assert list(want) == list(oracle_statuses(items, shape))
    if n >= 2:
        two = make_batch(["honest"] * n, shape, 400 + n)
        two[0].t[0], two[n - 1].t[0] = (two[0].t[0] + 12345) % R, (two[n - 1].t[0] - 12345) % R
        got, batch_ok = ctx.kzg_multi_check_batch_rlc(*arrays(two, shape), VK, seed=SEED)
        assert not batch_ok and list(got) == [1] + [0] * (n - 2) + [1]


@pytest.mark.gpu
def test_gpu_invalid_key_or_shared_base_makes_every_item_invalid_data(ctx):
    shape = RING
    items = make_batch(["honest", "piinf", "t+1", "nonsquare", "allinf"], shape, 88)
    off = lambda b: b[:48] + w48((int.from_bytes(b[48:], "little") + 1) % P)
    flip = lambda key, at: key[:at] + bytes([key[at] ^ 1]) + key[at + 1:]
    a = arrays(items, shape)
    for bad_vk in (off(G96) + VK[96:], BAD96 + VK[96:], flip(VK, 96 + 5), flip(VK, 288 + 5)):
        assert list(ctx.kzg_multi_check_batch(*a, bad_vk)) == [2] * 5
        assert list(item_dev(ctx, items, shape, bad_vk)) == [2] * 5
        got, batch_ok = ctx.kzg_multi_check_batch_rlc(*a, bad_vk, seed=SEED)
        assert list(got) == [2] * 5 and not batch_ok
    for at in range(3):
        bad = SHARED[:at] + [off(SHARED[at])] + SHARED[at + 1:]
        b = list(a)
        b[2] = np.frombuffer(b"".join(bad), np.uint8).reshape(3, 96).copy()
        assert list(ctx.kzg_multi_check_batch(*b, VK)) == [2] * 5
        assert list(item_dev(ctx, items, shape, shared=bad)) == [2] * 5
        got, batch_ok = ctx.kzg_multi_check_batch_rlc(*b, VK, seed=SEED)
        assert list(got) == [2] * 5 and not batch_ok
    assert list(ctx.kzg_multi_check_batch(*a, VK)) == [0, 0, 1, 2, 0]                     # the good key still answers


@pytest.mark.gpu
def test_gpu_reduces_to_the_single_point_check(ctx):
    """(1, 0, 1) with s = u = 1 and t_i0 = r - v: all four calls return the statuses of vrfhip_kzg_check_batch on the mixed batch
    of the single-point tests (an item with v >= r becomes t = r - v out of range or, wrapped, stays invalid as 2^256 - 1)"""
    import torch
    n = 33
    items = single.make_batch(single.mixed_kinds(n), n)
    want = ctx.kzg_check_batch(*single.arrays(items), VK)
    assert set(want) == {0, 1, 2}
    c, z, v, pi = single.arrays(items)
    one = np.zeros((n, 1, 32), np.uint8)
    one[:, 0, 0] = 1
    t = np.frombuffer(b"".join(le((R - it.v) % R if it.v < R else (1 << 256) - 1) for it in items), np.uint8).reshape(n, 1, 32).copy()
    a = [c.reshape(n, 1, 48), one, None, t, pi.reshape(n, 1, 48), z.reshape(n, 1, 32), one.copy()]
    assert list(ctx.kzg_multi_check_batch(*a, VK)) == list(want)
    got, batch_ok = ctx.kzg_multi_check_batch_rlc(*a, VK, seed=SEED)
    assert list(got) == list(want) and not batch_ok
    d = [None if x is None else torch.from_numpy(x).cuda() for x in a] + [torch.from_numpy(np.frombuffer(VK, np.uint8).copy()).cuda()]
    st = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")
    ctx.kzg_multi_check_batch_dev(*d, st)
    torch.cuda.synchronize()
    assert list(st.cpu().numpy()) == list(want)
    verdict = torch.full((1,), 0x5A, dtype=torch.uint8, device="cuda")
    ctx.kzg_multi_check_batch_rlc_dev(*d, st, verdict, SEED)
    torch.cuda.synchronize()
    assert list(st.cpu().numpy()) == [2 if w == 2 else 0 for w in want] and int(verdict.cpu()[0]) == 1
    # without the false items the one equation holds
    keep = [i for i in range(n) if want[i] != 1]
    sub = [None if x is None else x[keep] for x in a]
    got, batch_ok = ctx.kzg_multi_check_batch_rlc(*sub, VK, seed=SEED)
    assert list(got) == [want[i] for i in keep] and batch_ok


@pytest.mark.gpu
def test_gpu_argument_rules(ctx):
    import ctypes
    import torch
    from ark_ec_vrfs_amd import Context, Secp256r1Sha256Tai, _lib
    lib, h = _lib.load(), ctx._h
    seed = np.frombuffer(SEED, np.uint8).copy()
    shape = RING
    items = make_batch(["honest", "t+1"], shape, 7)
    a = arrays(items, shape)
    vk = np.frombuffer(VK, np.uint8).copy()
    st = np.zeros(2, np.uint8)
    okf = ctypes.c_int32(1)
    args = [x.ctypes.data for x in a + [vk]]
    d = [torch.from_numpy(x).cuda() for x in a + [vk, st]]
    dp = [t.data_ptr() for t in d]
    verdict = torch.full((1,), 0x5A, dtype=torch.uint8, device="cuda")
    host = lambda ctxh, n, sh, ar, stp: lib.vrfhip_kzg_multi_check_batch(ctxh, n, *sh, *ar, stp)
    host_rlc = lambda ctxh, n, sh, ar, sd, stp: lib.vrfhip_kzg_multi_check_batch_rlc(ctxh, n, *sh, *ar, sd, stp, ctypes.byref(okf))
    dev = lambda ctxh, n, sh, ar: lib.vrfhip_kzg_multi_check_batch_dev(ctxh, n, *sh, *ar, None)
    dev_rlc = lambda ctxh, n, sh, ar, sd, vd: lib.vrfhip_kzg_multi_check_batch_rlc_dev(ctxh, n, *sh, *ar[:8], sd, ar[8], vd, None, None)
    assert host(h, 2, shape, args, st.ctypes.data) == 0 and list(st) == [0, 1]
    # n = 0 touches nothing, NULLs are fine; the shape is still checked
    none8 = [None] * 8
    assert host(h, 0, shape, none8, None) == 0 and dev(h, 0, shape, none8 + [None]) == 0
    assert host_rlc(h, 0, shape, none8, seed.ctypes.data, None) == 0 and okf.value == 1
    assert dev_rlc(h, 0, shape, none8 + [None], seed.ctypes.data, verdict.data_ptr()) == 0
    torch.cuda.synchronize()
    assert int(verdict.cpu()[0]) == 0
    # a shape outside the bounds
    for bad in ((5, 3, 0), (5, 3, 8), (12, 2, 2), (0, 15, 1), (2 ** 32 - 1, 1, 1), (1, 2 ** 32 - 1, 1), (1, 1, 2 ** 32 - 1)):
        assert host(h, 2, bad, args, st.ctypes.data) == -1 and host(h, 0, bad, none8, None) == -1, bad
        assert host_rlc(h, 2, bad, args, seed.ctypes.data, st.ctypes.data) == -1, bad
        assert dev(h, 2, bad, dp) == -1 and dev_rlc(h, 2, bad, dp, seed.ctypes.data, verdict.data_ptr()) == -1, bad
    # NULL with a non-zero count
    for j in range(8):
        b, db = list(args), list(dp)
        b[j] = db[j] = None
        assert host(h, 2, shape, b, st.ctypes.data) == -1 and host_rlc(h, 2, shape, b, seed.ctypes.data, st.ctypes.data) == -1, j
        assert dev(h, 2, shape, db) == -1 and dev_rlc(h, 2, shape, db, seed.ctypes.data, verdict.data_ptr()) == -1, j
    assert host(h, 2, shape, args, None) == -1 and host(None, 2, shape, args, st.ctypes.data) == -1
    assert host_rlc(h, 2, shape, args, None, st.ctypes.data) == -1
    assert dev_rlc(h, 2, shape, dp, seed.ctypes.data, None) == -1 and dev_rlc(h, 2, shape, dp, None, verdict.data_ptr()) == -1
    assert dev(h, (1 << 28) + 1, shape, dp) == -1 and dev(h, 1 << 26, shape, dp) == -1      # n (k + p) + m + 1 > 2^28
    # an array whose count is 0 may be NULL
    it0 = make_batch(["honest", "negpi"], (0, 0, 1), 8)
    a0 = arrays(it0, (0, 0, 1))
    assert a0[0] is None and a0[1] is None and a0[2] is None
    assert list(ctx.kzg_multi_check_batch(*a0, VK)) == [0, 1]
    # a secp256r1 context is refused
    other = Context(0, Secp256r1Sha256Tai)
    try:
        assert host(other._h, 2, shape, args, st.ctypes.data) == -5
        assert host_rlc(other._h, 2, shape, args, seed.ctypes.data, st.ctypes.data) == -5
        assert dev(other._h, 2, shape, dp) == -5
        assert dev_rlc(other._h, 2, shape, dp, seed.ctypes.data, verdict.data_ptr()) == -5
    finally:
        other.close()
    # the Python layer infers and checks the shape
    with pytest.raises(ValueError):
        ctx.kzg_multi_check_batch(a[0], a[1][:, :4], a[2], a[3], a[4], a[5], a[6], VK)
    with pytest.raises(ValueError):
        ctx.kzg_multi_check_batch(a[0], a[1], a[2], a[3][:, :3], a[4], a[5], a[6], VK)
