"""CPU: the per-lane functions of the KZG opening check (kzg.cuh: kzg_weight, kzg_prep_item, kzg_acc, kzg_fold_finish,
kzg_combine, kzg_item_rows) compiled for the host (tests/hostsim_kzg) against hashlib and Python integers: the weights, the
products r_i z_i mod r, the folded scalar -sum r_i v_i mod r, the digit rows recombined to their scalars, the statuses.  The
lane reductions of the kernels are restated in the host program with the kernels' shape (blocks of 128, 256 strided sums, a
tree).  Points come from the native C oracle (oracle.c_oracle.g1_mul / g1_add on the 96-byte form)."""
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
SIM = os.path.join(HERE, "hostsim_kzg")
INF, BAD96 = bytes(96), b"\xff" * 96
SIZES = [1, 2, 127, 128, 129, 300]


def xy96(pt):
    return INF if pt is None else pt[0].to_bytes(48, "little") + pt[1].to_bytes(48, "little")


def neg96(b):
    return b if b == INF else b[:48] + ((P - int.from_bytes(b[48:], "little")) % P).to_bytes(48, "little")


def weight(seed, root, i):
    return int.from_bytes(hashlib.sha512(b"vrfhip-kzg-rlc-v1" + seed + root + i.to_bytes(8, "little")).digest()[:16], "little")


def recombine(col):
    return sum(int(d) << (10 * w) for w, d in enumerate(col))


class Sim:
    def __init__(self, lib):
        self.lib = lib
        for f in ("hk_block", "hk_windows_short", "hk_windows_full"):
            getattr(lib, f).restype = ctypes.c_int
        lib.hk_weight.restype = lib.hk_combine.restype = lib.hk_item_rows.restype = None
        lib.hk_prep_fold.restype = ctypes.c_size_t
        V = ctypes.c_void_p
        lib.hk_weight.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint64, V]
        lib.hk_prep_fold.argtypes = [ctypes.c_size_t] + [ctypes.c_char_p] * 7 + [V] * 5
        lib.hk_combine.argtypes = [ctypes.c_char_p] * 3 + [ctypes.c_int, V]
        lib.hk_item_rows.argtypes = [ctypes.c_size_t] + [ctypes.c_char_p] * 5 + [V] * 5
        self.ws, self.wf, self.block = lib.hk_windows_short(), lib.hk_windows_full(), lib.hk_block()

    def weight(self, seed, root, i):
        out = ctypes.create_string_buffer(32)
        self.lib.hk_weight(seed, root, i, out)
        return int.from_bytes(out.raw, "little")

    def prep_fold(self, items, g, seed, root):
        """items: (c96, z, v, pi96) -> short digits (2, ws, n), full digits (wf, n + 1), status (n,), partials, flag"""
        n = len(items)
        sd, fd = np.full((2, self.ws, n), 9999, np.int16), np.full((self.wf, n + 1), 9999, np.int16)
        st, flag = np.full(n, 9, np.uint8), np.full(1, 9, np.uint8)
        part = np.zeros(((n + self.block - 1) // self.block, 9), np.uint32)
        le = lambda x: x.to_bytes(32, "little")
        got = self.lib.hk_prep_fold(n, b"".join(it[0] for it in items), b"".join(it[3] for it in items),
                                    b"".join(le(it[1]) for it in items), b"".join(le(it[2]) for it in items), g, seed, root,
                                    sd.ctypes.data, fd.ctypes.data, st.ctypes.data, part.ctypes.data, flag.ctypes.data)
        assert got == part.shape[0]
        return sd, fd, st, part, int(flag[0])

    def combine(self, a, f, b, vk_ok=True):
        out = ctypes.create_string_buffer(192)
        self.lib.hk_combine(a, f, b, int(vk_ok), out)
        return out.raw


@pytest.fixture(scope="module")
def sim():
    subprocess.run(["make", "-C", SIM, "libhostsim_kzg.so"], check=True, stdout=subprocess.DEVNULL)
    return Sim(ctypes.CDLL(os.path.join(SIM, "libhostsim_kzg.so")))


@pytest.fixture(scope="module")
def pool():
    rnd = random.Random(381)
    g = xy96(bls.G1)
    return [co.g1_mul(rnd.randrange(1, R), g) for _ in range(6)]


def make_batch(n, pool, rnd, special=True):
    """(c, z, v, pi) with the edge scalars, both infinities and every kind of invalid item spread over the batch"""
    items = []
    for i in range(n):
        c, pi = pool[i % 6], pool[(i + 1) % 6]
        z, v = rnd.randrange(R), rnd.randrange(R)
        if special:
            k = i % 16
            z = {1: 0, 2: 1, 3: R - 1}.get(k, z)
            v = {1: R - 1, 2: 0, 3: 1, 4: R - 1}.get(k, v)
            if k == 5: c = INF
            if k == 6: pi = INF
            if k == 7: c, pi, v = INF, INF, 0
            if k == 8: z = R                      # invalid scalars
            if k == 9: v = (1 << 256) - 1
            if k == 10: c = BAD96                 # what the decode stage leaves for an invalid point
            if k == 11: pi = BAD96
        items.append((c, z, v, pi))
    return items


def valid(it):
    return it[0] != BAD96 and it[3] != BAD96 and it[1] < R and it[2] < R


def check_batch(sim, items, g, seed, root, g_ok=True):
    n = len(items)
    sd, fd, st, part, flag = sim.prep_fold(items, g, seed, root)
    assert flag == (0 if g_ok else 2)
    assert sd.min() >= -511 and sd.max() <= 512 and fd.min() >= -511 and fd.max() <= 512
    total = 0
    for i, it in enumerate(items):
        ok, r = valid(it), weight(seed, root, i)
        assert st[i] == (0 if ok else 2), i
        assert recombine(sd[0, :, i]) == (r if ok and it[0] != INF else 0), i
        assert recombine(sd[1, :, i]) == (r if ok and it[3] != INF else 0), i
        assert recombine(fd[:, i]) == (r * it[1] % R if ok and it[3] != INF else 0), i
        if not ok:
            assert not sd[:, :, i].any() and not fd[:, i].any(), i
        else:
            total += r * it[2]
    # the partial sums: 9 limbs of 29 bits, a plain residue below 2 r, one per block of 128 items
    for b in range(part.shape[0]):
        val = sum(int(x) << (29 * j) for j, x in enumerate(part[b]))
        blk = range(b * sim.block, min(n, (b + 1) * sim.block))
        assert val < 2 * R and val % R == sum(weight(seed, root, i) * items[i][2] for i in blk if valid(items[i])) % R, b
    want = (-total) % R if g_ok and g != INF else 0
    assert recombine(fd[:, n]) == want
    return fd


def test_weights_equal_the_definition(sim):
    rnd = random.Random(1)
    for i in (0, 1, 127, 128, 2 ** 28, 2 ** 40 + 5):
        seed, root = rnd.randbytes(32), rnd.randbytes(32)
        w = sim.weight(seed, root, i)
        assert w == weight(seed, root, i) and w < 1 << 128


@pytest.mark.parametrize("n", SIZES)
def test_digits_products_fold_and_statuses(sim, pool, n):
    rnd = random.Random(n)
    seed, root = rnd.randbytes(32), rnd.randbytes(32)
    g = co.g1_mul(rnd.randrange(1, R), xy96(bls.G1))
    check_batch(sim, make_batch(n, pool, rnd), g, seed, root)
    check_batch(sim, make_batch(n, pool, rnd, special=False), g, seed, root)


@pytest.mark.parametrize("n", SIZES)
def test_all_values_zero_leaves_g_out(sim, pool, n):
    rnd = random.Random(100 + n)
    items = [(c, z, 0, pi) for c, z, _, pi in make_batch(n, pool, rnd, special=False)]
    fd = check_batch(sim, items, pool[0], rnd.randbytes(32), rnd.randbytes(32))
    assert not fd[:, n].any()


@pytest.mark.parametrize("n", SIZES)
def test_every_item_invalid(sim, pool, n):
    rnd = random.Random(200 + n)
    kinds = [(BAD96, 1, 1, pool[0]), (pool[0], 1, 1, BAD96), (pool[0], R, 1, pool[1]), (pool[0], 1, (1 << 256) - 1, pool[1]),
             (INF, R + 1, 0, INF)]
    items = [kinds[i % 5] for i in range(n)]
    sd, fd, st, part, flag = sim.prep_fold(items, pool[2], rnd.randbytes(32), rnd.randbytes(32))
    assert flag == 0 and (st == 2).all() and not sd.any() and not fd.any() and not part.any()


def test_the_key_s_g(sim, pool):
    rnd = random.Random(7)
    seed, root = rnd.randbytes(32), rnd.randbytes(32)
    items = make_batch(5, pool, rnd, special=False)
    gx, gy = bls.G1
    check_batch(sim, items, INF, seed, root)                                             # g at infinity: valid, no digits
    for bad in (xy96((gx, (gy + 1) % P)), P.to_bytes(48, "little") + gy.to_bytes(48, "little"), BAD96):
        check_batch(sim, items, bad, seed, root, g_ok=False)


def test_combine_equals_the_oracle(sim, pool):
    a, f, b = pool[0], pool[1], pool[2]
    assert sim.combine(a, f, b) == co.g1_add(a, f) + neg96(b)
    assert sim.combine(a, a, b) == co.g1_add(a, a) + neg96(b)                            # the law doubles
    assert sim.combine(INF, f, INF) == f + INF and sim.combine(a, INF, b) == a + neg96(b)
    assert sim.combine(a, neg96(a), b) == INF + neg96(b) and sim.combine(INF, INF, INF) == INF + INF
    assert sim.combine(a, f, b, vk_ok=False) == BAD96 + BAD96


def test_item_rows(sim, pool):
    rnd = random.Random(9)
    items = make_batch(48, pool, rnd)
    n = len(items)
    dec_ok = bytes(0 if (it[0] == BAD96 or it[3] == BAD96) else 1 for it in items)
    le = lambda x: x.to_bytes(32, "little")
    bufs = [ctypes.create_string_buffer(w * n) for w in (192, 64, 32, 96, 1)]
    sim.lib.hk_item_rows(n, b"".join(it[0] for it in items), b"".join(it[3] for it in items), dec_ok,
                         b"".join(le(it[1]) for it in items), b"".join(le(it[2]) for it in items), *bufs)
    bases, scalars, shared, neg_pi, ok = (b.raw for b in bufs)
    for i, (c, z, v, pi) in enumerate(items):
        if valid(items[i]):
            assert ok[i] == 1 and bases[192 * i:192 * i + 192] == c + pi
            assert scalars[64 * i:64 * i + 64] == le(1) + le(z) and shared[32 * i:32 * i + 32] == le((R - v) % R)
            assert neg_pi[96 * i:96 * i + 96] == neg96(pi)
        else:
            assert ok[i] == 0
            assert bases[192 * i:192 * i + 192] + scalars[64 * i:64 * i + 64] + shared[32 * i:32 * i + 32] + \
                neg_pi[96 * i:96 * i + 96] == b"\xff" * 384
