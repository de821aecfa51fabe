"""CPU: the per-lane functions of the multi-point KZG opening check (kzg_multi.cuh: kzgm_weight, kzgm_item_valid,
kzgm_col_term, kzgm_prep_term, kzgm_fold_finish, kzgm_combine, kzgm_item_rows) compiled for the host
(tests/hostsim_kzg_multi) against hashlib and Python integers: the weights with the shape words, the products r_i s_ij,
r_i u_ij z_ij and r_i u_ij mod r recombined from their digit rows, the block partials and the m + 1 folded column scalars,
the statuses, the rows of the per-item form.  The lane reductions of the kernels are restated in the host program with the
kernels' shape.  Points come from the native C oracle (oracle.c_oracle.g1_mul / g1_add on the 96-byte form)."""
import ctypes
import hashlib
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import bls_oracle as bls
from oracle import c_oracle as co

P, R = bls.P, bls.R
HERE = os.path.dirname(os.path.abspath(__file__))
SIM = os.path.join(HERE, "hostsim_kzg_multi")
INF, BAD96 = bytes(96), b"\xff" * 96
SIZES = [1, 2, 127, 128, 129, 300]
SHAPES = [(1, 0, 1), (0, 0, 1), (5, 3, 2), (3, 1, 3), (11, 2, 2)]
TAG = b"vrfhip-kzg-multi-rlc-v1"
le = lambda x: int(x).to_bytes(32, "little")


def xy96(pt):
    return INF if pt is None else pt[0].to_bytes(48, "little") + pt[1].to_bytes(48, "little")


def neg96(b):
    return b if b == INF else b[:48] + ((P - int.from_bytes(b[48:], "little")) % P).to_bytes(48, "little")


def weight(shape, seed, root, i):
    pre = TAG + b"".join(x.to_bytes(4, "little") for x in shape)
    return int.from_bytes(hashlib.sha512(pre + seed + root + i.to_bytes(8, "little")).digest()[:16], "little")


def recombine(col):
    return sum(int(d) << (10 * w) for w, d in enumerate(col))


class Item:
    """c, pi: lists of decoded points (BAD96: what the decode stage leaves for an invalid one); s, t, z, u: lists of integers"""

    def __init__(self, c, s, t, pi, z, u):
        self.c, self.s, self.t, self.pi, self.z, self.u = c, s, t, pi, z, u

    @property
    def valid(self):
        return BAD96 not in self.c and BAD96 not in self.pi and all(x < R for x in self.s + self.t + self.z + self.u)


class Sim:
    def __init__(self, lib):
        self.lib = lib
        V, C, U = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint32
        lib.hm_block.restype = lib.hm_windows.restype = lib.hm_shape_ok.restype = ctypes.c_int
        lib.hm_weight.restype = lib.hm_combine.restype = lib.hm_item_rows.restype = None
        lib.hm_prep_fold.restype = ctypes.c_size_t
        lib.hm_shape_ok.argtypes = [U] * 3
        lib.hm_weight.argtypes = [U] * 3 + [C, C, ctypes.c_uint64, V]
        lib.hm_prep_fold.argtypes = [ctypes.c_size_t] + [U] * 3 + [C] * 11 + [V] * 5
        lib.hm_combine.argtypes = [C, C, ctypes.c_int, V]
        lib.hm_item_rows.argtypes = [ctypes.c_size_t] + [U] * 3 + [C] * 8 + [V] * 6
        self.windows, self.block = lib.hm_windows(), lib.hm_block()

    def weight(self, shape, seed, root, i):
        out = ctypes.create_string_buffer(32)
        self.lib.hm_weight(*shape, seed, root, i, out)
        return int.from_bytes(out.raw, "little")

    @staticmethod
    def inputs(items):
        """the eight input arrays in the order of hm_prep_fold / hm_item_rows (+ b"\\0": never an empty buffer)"""
        cat = lambda rows: b"".join(rows) + b"\0"
        return [cat(x for it in items for x in it.c), bytes(2 * (x == BAD96) for it in items for x in it.c) + b"\0",
                cat(le(x) for it in items for x in it.s), cat(le(x) for it in items for x in it.t),
                cat(x for it in items for x in it.pi), bytes(2 * (x == BAD96) for it in items for x in it.pi) + b"\0",
                cat(le(x) for it in items for x in it.z), cat(le(x) for it in items for x in it.u)]

    def prep_fold(self, shape, items, bases, seed, root):
        """-> A digits (windows, n (k + p) + m + 1), B digits (windows, n p), status (n,), partials (m + 1, blocks, 9), flag"""
        k, m, p = shape
        n = len(items)
        ad = np.full((self.windows, n * (k + p) + m + 1), 9999, np.int16)
        bd = np.full((self.windows, n * p), 9999, np.int16)
        st, flag = np.full(n, 9, np.uint8), np.full(1, 9, np.uint8)
        part = np.zeros((m + 1, (n + self.block - 1) // self.block, 9), np.uint32)
        got = self.lib.hm_prep_fold(n, k, m, p, *self.inputs(items), b"".join(bases), seed, root, ad.ctypes.data, bd.ctypes.data,
                                    st.ctypes.data, part.ctypes.data, flag.ctypes.data)
        assert got == part.shape[1]
        return ad, bd, st, part, int(flag[0])

    def combine(self, a, b, vk_ok=True):
        out = ctypes.create_string_buffer(192)
        self.lib.hm_combine(a, b, int(vk_ok), out)
        return out.raw


@pytest.fixture(scope="module")
def sim():
    subprocess.run(["make", "-C", SIM, "libhostsim_kzg_multi.so"], check=True, stdout=subprocess.DEVNULL)
    return Sim(ctypes.CDLL(os.path.join(SIM, "libhostsim_kzg_multi.so")))


@pytest.fixture(scope="module")
def pool():
    rnd = random.Random(381)
    g = xy96(bls.G1)
    return [co.g1_mul(rnd.randrange(1, R), g) for _ in range(6)]


SCALAR_ARRAYS = ("s", "t", "z", "u")


def make_batch(n, shape, pool, rnd, special=True):
    """random items; with `special`, item i takes kind i mod 24: the edge scalars 0, 1, r - 1 and the invalid values r and
    2^256 - 1 in each of the four scalar arrays in turn, infinity and 0xFF points at the first, a middle and the last term"""
    k, m, p = shape
    items = []
    for i in range(n):
        it = Item([pool[(i + j) % 6] for j in range(k)], [rnd.randrange(R) for _ in range(k)],
                  [rnd.randrange(R) for _ in range(m + 1)], [pool[(i + j + 1) % 6] for j in range(p)],
                  [rnd.randrange(R) for _ in range(p)], [rnd.randrange(R) for _ in range(p)])
        kind = i % 24 if special else -1
        if 0 <= kind < 20:                        # five values x four arrays, at a position that walks through the row
            arr = getattr(it, SCALAR_ARRAYS[kind % 4])
            if arr:
                arr[(i // 24) % len(arr)] = (0, 1, R - 1, R, (1 << 256) - 1)[kind // 4]
        pts = it.c + it.pi                        # the item's terms in the order of layout A
        where = {20: 0, 21: len(pts) // 2, 22: len(pts) - 1}.get(kind)
        if where is not None:
            pts[where] = BAD96 if (i // 24) % 2 == 0 else INF
            it.c, it.pi = pts[:k], pts[k:]
        if kind == 23:
            it.c, it.pi, it.u = [INF] * k, [INF] * p, [0] * p
        items.append(it)
    return items


def check_batch(sim, shape, items, bases, seed, root, bad_base=None):
    k, m, p = shape
    n, T = len(items), k + p
    ad, bd, st, part, flag = sim.prep_fold(shape, items, bases, seed, root)
    assert flag == (0 if bad_base is None else 2)
    assert ad.min() >= -511 and ad.max() <= 512 and (bd.size == 0 or (bd.min() >= -511 and bd.max() <= 512))
    cols = [0] * (m + 1)
    for i, it in enumerate(items):
        ok, r = it.valid, weight(shape, seed, root, i)
        assert st[i] == (0 if ok else 2), i
        for j in range(k):
            assert recombine(ad[:, i * T + j]) == (r * it.s[j] % R if ok and it.c[j] != INF else 0), (i, j)
        for j in range(p):
            live = ok and it.pi[j] != INF
            assert recombine(ad[:, i * T + k + j]) == (r * it.u[j] * it.z[j] % R if live else 0), (i, j)
            assert recombine(bd[:, i * p + j]) == (r * it.u[j] % R if live else 0), (i, j)
        if not ok:
            assert not ad[:, i * T:(i + 1) * T].any() and not bd[:, i * p:(i + 1) * p].any(), i
        else:
            cols = [c + r * t for c, t in zip(cols, it.t)]
    # the partial sums: 9 limbs of 29 bits, a plain residue below 2 r, one per column and block of 128 items
    for c in range(m + 1):
        for b in range(part.shape[1]):
            val = sum(int(x) << (29 * j) for j, x in enumerate(part[c, b]))
            blk = range(b * sim.block, min(n, (b + 1) * sim.block))
            want = sum(weight(shape, seed, root, i) * items[i].t[c] for i in blk if items[i].valid)
            assert val < 2 * R and val % R == want % R, (c, b)
        assert recombine(ad[:, n * T + c]) == (0 if c == bad_base or bases[c] == INF else cols[c] % R), c
    return ad, bd, st, part


def test_weights_equal_the_definition_and_depend_on_the_shape(sim):
    rnd = random.Random(1)
    for i in (0, 1, 127, 128, 2 ** 28, 2 ** 40 + 5):
        seed, root = rnd.randbytes(32), rnd.randbytes(32)
        got = [sim.weight(sh, seed, root, i) for sh in SHAPES + [(1, 1, 0), (0, 1, 1), (2, 5, 3), (5, 2, 3)]]
        assert got[:5] == [weight(sh, seed, root, i) for sh in SHAPES] and all(w < 1 << 128 for w in got)
        assert len(set(got)) == len(got)          # the shape alone changes the weight, whichever of its words differs


def test_shape_bounds(sim):
    ok = lambda *sh: bool(sim.lib.hm_shape_ok(*sh))
    assert all(ok(*sh) for sh in SHAPES) and ok(0, 14, 1) and ok(14, 0, 1) and ok(0, 0, 15)
    assert not ok(1, 0, 0) and not ok(5, 3, 8) and not ok(0, 15, 1) and not ok(15, 0, 1) and not ok(2 ** 32 - 1, 1, 1)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("n", SIZES)
def test_digits_products_fold_and_statuses(sim, pool, n, shape):
    rnd = random.Random(n * 100 + sum(shape))
    seed, root = rnd.randbytes(32), rnd.randbytes(32)
    bases = [pool[(j + 2) % 6] for j in range(shape[1] + 1)]
    st = check_batch(sim, shape, make_batch(n, shape, pool, rnd), bases, seed, root)[2]
    if n >= 128:
        assert 0 < (st == 2).sum() < n
    check_batch(sim, shape, make_batch(n, shape, pool, rnd, special=False), bases, seed, root)


@pytest.mark.parametrize("shape", SHAPES)
def test_every_item_invalid(sim, pool, shape):
    k, m, p = shape
    for n in (1, 129):
        rnd = random.Random(200 + n)
        items = make_batch(n, shape, pool, rnd, special=False)
        for i, it in enumerate(items):
            which = i % 5
            if which == 0 and k: it.s[-1] = R
            elif which == 1: it.t[0] = (1 << 256) - 1
            elif which == 2: it.z[-1] = R
            elif which == 3: it.u[0] = R + 1
            else: it.pi[p // 2] = BAD96
        bases = [pool[j % 6] for j in range(m + 1)]
        ad, bd, st, part, flag = sim.prep_fold(shape, items, bases, rnd.randbytes(32), rnd.randbytes(32))
        assert flag == 0 and (st == 2).all() and not ad.any() and not bd.any() and not part.any()


@pytest.mark.parametrize("shape", [(5, 3, 2), (0, 0, 1)])
def test_the_shared_bases(sim, pool, shape):
    rnd = random.Random(7)
    seed, root = rnd.randbytes(32), rnd.randbytes(32)
    m = shape[1]
    items = make_batch(5, shape, pool, rnd, special=False)
    good = [pool[j % 6] for j in range(m + 1)]
    gx, gy = bls.G1
    for at in range(m + 1):                                                              # g (at = 0) and every shared base
        check_batch(sim, shape, items, good[:at] + [INF] + good[at + 1:], seed, root)   # at infinity: valid, no digits
        for bad in (xy96((gx, (gy + 1) % P)), P.to_bytes(48, "little") + gy.to_bytes(48, "little"), BAD96):
            check_batch(sim, shape, items, good[:at] + [bad] + good[at + 1:], seed, root, bad_base=at)


def test_combine_equals_the_oracle(sim, pool):
    a, b = pool[0], pool[1]
    assert sim.combine(a, b) == a + neg96(b) and sim.combine(a, a) == a + neg96(a)
    assert sim.combine(INF, b) == INF + neg96(b) and sim.combine(a, INF) == a + INF and sim.combine(INF, INF) == INF + INF
    assert sim.combine(a, b, vk_ok=False) == BAD96 + BAD96
    assert co.g1_add(sim.combine(a, b)[96:], b) == INF                                   # S_B is the oracle's -b


@pytest.mark.parametrize("shape", SHAPES)
def test_item_rows(sim, pool, shape):
    k, m, p = shape
    rnd = random.Random(9)
    items = make_batch(48, shape, pool, rnd)
    n, T = len(items), k + p
    widths = (96 * T, 32 * T, 32 * (m + 1), 96 * p, 32 * p, 1)
    bufs = [ctypes.create_string_buffer(w * n) for w in widths]
    sim.lib.hm_item_rows(n, k, m, p, *sim.inputs(items), *bufs)
    rows = [[b.raw[w * i:w * (i + 1)] for b, w in zip(bufs, widths)] for i in range(n)]
    assert 0 < sum(it.valid for it in items) < n
    for it, (bases_a, scalars_a, shared_a, bases_b, scalars_b, ok) in zip(items, rows):
        if it.valid:
            assert ok == b"\1" and bases_a == b"".join(it.c + it.pi) and bases_b == b"".join(it.pi)
            assert scalars_a == b"".join(le(x) for x in it.s + [u * z % R for u, z in zip(it.u, it.z)])
            assert shared_a == b"".join(le(x) for x in it.t) and scalars_b == b"".join(le((R - u) % R) for u in it.u)
        else:
            assert ok == b"\0" and bases_a + scalars_a + shared_a + bases_b + scalars_b == b"\xff" * sum(widths[:5])
