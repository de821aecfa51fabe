"""CPU: the per-lane functions of the BLS12-381 G1 linear combinations (g1_lincomb.cuh: lc_recode / lc_digit, lc_term,
lc_finish) compiled for the host (tests/hostsim_g1lincomb) against the native C oracle (oracle.c_oracle.g1_mul / g1_add on
the 96-byte form): the signed 3-bit recoding on its own, one term, and sums of 1..16 terms with the cases that go through the
corners of the complete addition law.  The kernel's lane reduction is here a sequential g1_add."""
import ctypes
import os
import random
import subprocess

import pytest

from oracle import bls_oracle as bls
from oracle import c_oracle as co

P, R = bls.P, bls.R
HERE = os.path.dirname(os.path.abspath(__file__))
SIM = os.path.join(HERE, "hostsim_g1lincomb")
INF, BAD96 = bytes(96), b"\xff" * 96
ALT4 = sum(4 << (3 * w) for w in range(84))            # 0b100100...: every window 4, the recoding carries all the way up
ALT3 = sum(3 << (3 * w) for w in range(84))            # 0b011011...: every window 3, no carry anywhere
EDGE = [0, 1, 3, 4, 5, R - 1, (1 << 254) - 1, ALT4, ALT3]          # 2^255 - 1 masked to < r: its low 254 bits


def xy96(pt):
    return INF if pt is None else pt[0].to_bytes(48, "little") + pt[1].to_bytes(48, "little")


def neg96(b):
    return b if b == INF else b[:48] + ((P - int.from_bytes(b[48:], "little")) % P).to_bytes(48, "little")


class Sim:
    def __init__(self, lib):
        self.lib = lib
        lib.hl_windows.restype = ctypes.c_int
        lib.hl_recode.restype = lib.hl_lincomb.restype = None
        lib.hl_recode.argtypes = [ctypes.c_size_t, ctypes.c_char_p, ctypes.c_char_p]
        lib.hl_lincomb.argtypes = [ctypes.c_size_t, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p,
                                   ctypes.c_char_p]
        self.windows = lib.hl_windows()

    def recode(self, scalars):
        n, W = len(scalars), self.windows
        out = ctypes.create_string_buffer(n * W)
        self.lib.hl_recode(n, b"".join(s.to_bytes(32, "little") for s in scalars), out)
        return [[b - 256 if b > 127 else b for b in out.raw[i * W:(i + 1) * W]] for i in range(n)]

    def lincomb(self, items):
        """items: equally long lists of (scalar, base96) -> [(status, 96 bytes)]"""
        n, t = len(items), len(items[0])
        assert all(len(it) == t for it in items)
        out, st = ctypes.create_string_buffer(96 * n), ctypes.create_string_buffer(n)
        self.lib.hl_lincomb(n, t, b"".join(b for it in items for _, b in it),
                            b"".join(s.to_bytes(32, "little") for it in items for s, _ in it), out, st)
        return [(st.raw[i], out.raw[96 * i:96 * i + 96]) for i in range(n)]


@pytest.fixture(scope="module")
def sim():
    subprocess.run(["make", "-C", SIM, "libhostsim_g1lincomb.so"], check=True, stdout=subprocess.DEVNULL)
    return Sim(ctypes.CDLL(os.path.join(SIM, "libhostsim_g1lincomb.so")))


@pytest.fixture(scope="module")
def pool():
    """16 bases: multiples of the generator, both signs"""
    rnd = random.Random(381)
    g = xy96(bls.G1)
    pts = [co.g1_mul(rnd.randrange(1, R), g) for _ in range(8)]
    return pts + [neg96(p) for p in pts]


def expected(item):
    acc = INF
    for s, b in item:
        acc = co.g1_add(acc, co.g1_mul(s, b))
    return (0, acc)


def test_oracle_agrees_with_the_python_oracle():
    """the native oracle the expected values come from, against the pure-Python one, on a handful of points"""
    rnd = random.Random(5)
    for s in (1, 2, R - 1, rnd.randrange(R)):
        assert co.g1_mul(s, xy96(bls.G1)) == xy96(bls.g1_mul(s, bls.G1))
    a, b = bls.g1_mul(7, bls.G1), bls.g1_mul(11, bls.G1)
    assert co.g1_add(xy96(a), xy96(b)) == xy96(bls.g1_mul(18, bls.G1))
    assert co.g1_add(xy96(a), neg96(xy96(a))) == INF and co.g1_mul(0, xy96(a)) == INF


def test_recoding_digits_sum_to_the_scalar(sim):
    rnd = random.Random(3)
    scalars = EDGE + [rnd.randrange(R) for _ in range(10 ** 4)] + [rnd.randrange(R) >> rnd.randrange(250) for _ in range(500)]
    digs = sim.recode(scalars)
    assert sim.windows == 86
    for s, d in zip(scalars, digs):
        assert all(abs(x) <= 4 for x in d), hex(s)
        assert sum(x << (3 * w) for w, x in enumerate(d)) == s, hex(s)
    top = {s: d[85] for s, d in zip(scalars, digs)}
    # the top window takes the carry of the 85 windows below it: r - 1, 2^254 - 1 and the all-4 pattern reach it
    assert top[R - 1] == 1 and top[(1 << 254) - 1] == 1 and top[0] == 0 and top[5] == 0 and top[ALT3] == 0
    assert digs[scalars.index(ALT4)][:85] == [-4] + [-3] * 83 + [1] and digs[scalars.index(ALT3)][:84] == [3] * 84
    assert {x for d in digs for x in d} == set(range(-4, 4))


def test_one_term_equals_the_oracle(sim, pool):
    rnd = random.Random(4)
    items = [[(s, b)] for s in EDGE for b in pool[:2]]
    items += [[(rnd.randrange(R), rnd.choice(pool))] for _ in range(200)]
    assert sim.lincomb(items) == [expected(it) for it in items]


@pytest.mark.parametrize("t", range(1, 17))
def test_sums_of_t_terms(sim, pool, t):
    rnd = random.Random(t)
    rs = lambda: rnd.randrange(R)
    s = rs()
    items = [[(rs(), pool[(j + i) % 16]) for j in range(t)] for i in range(2)]
    items.append([(rs(), pool[3]) for _ in range(t)])                                  # one base in every term
    items.append([(s, pool[5])] * t)                                                   # ... with one scalar: the law doubles
    items.append([(rs(), INF if j % 2 == 0 else pool[j]) for j in range(t)])           # bases at infinity, scalars non-zero
    items.append([(0, pool[j]) for j in range(t)])                                     # all scalars zero
    items.append([(rs() if j else 0, pool[j]) for j in range(t)])                      # a zero scalar among others
    if t >= 2:
        fill = [(0, pool[j]) for j in range(t - 2)]
        items.append([(s, pool[1]), (R - s, pool[1])] + fill)                          # s P + (r - s) P = infinity
        items.append(fill + [(s, pool[2]), (s, neg96(pool[2]))])                       # P and -P with one scalar
        items.append([(s, pool[1]), (R - s, pool[1])] + [(rs(), pool[j]) for j in range(t - 2)])
    got = sim.lincomb(items)
    want = [expected(it) for it in items]
    assert got == want
    assert got[5] == (0, INF)
    if t >= 2:
        assert got[7] == (0, INF) and got[8] == (0, INF)


def test_invalid_terms(sim, pool):
    gx, gy = bls.G1
    off_curve = xy96((gx, (gy + 1) % P))
    x_is_p = P.to_bytes(48, "little") + gy.to_bytes(48, "little")
    y_big = gx.to_bytes(48, "little") + b"\xff" * 48
    good = (7, pool[0])
    items = [[good, (1, off_curve), good], [good, good, (1, x_is_p)], [(1, y_big), good, good], [good, (R, pool[1]), good],
             [good, good, ((1 << 256) - 1, pool[1])], [(0, off_curve), good, good], [(R, INF), good, good], [good, good, good]]
    got = sim.lincomb(items)
    assert got[:7] == [(2, BAD96)] * 7 and got[7] == expected(items[7])
