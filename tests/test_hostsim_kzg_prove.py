"""CPU: the per-lane functions of the KZG commitment and opening (kzg_prove.cuh: kzg_commit_item, kzg_q_lane_sum, kzg_pow,
kzg_compose, kzg_apply, kzg_q_lane_emit) compiled for the host (tests/hostsim_kzg_prove) against Python integers: the quotient
recombined from its digit rows, the value, the statuses.  The host program restates the kernels' shape -- one chunk per lane,
B lanes per workgroup, the suffix scan in doubling strides, the chain over workgroups -- and exports B."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import bls_oracle as bls

R = bls.R
HERE = os.path.dirname(os.path.abspath(__file__))
SIM = os.path.join(HERE, "hostsim_kzg_prove")
le = lambda x: int(x).to_bytes(32, "little")


def recombine(col):
    return sum(int(d) << (10 * w) for w, d in enumerate(col))


def chunks10(pattern):
    """a 255-bit scalar whose 10-bit chunks all hold `pattern`, reduced below r"""
    return sum(pattern << (10 * w) for w in range(26)) % (1 << 255) % R


# ... and the same patterns in the low 25 chunks only (below 2^250 < r as they are: every chunk survives)
EDGE_SCALARS = [0, 1, R - 1, chunks10(0x1ff), chunks10(0x200), chunks10(0x3ff)] + \
               [sum(pat << (10 * w) for w in range(25)) for pat in (0x1ff, 0x200, 0x3ff)]
NE = len(EDGE_SCALARS)


class Sim:
    def __init__(self, lib):
        self.lib = lib
        V, Z = ctypes.c_void_p, ctypes.c_size_t
        for f in ("hp_block", "hp_chunk_max", "hp_windows"):
            getattr(lib, f).restype = ctypes.c_int
        lib.hp_cut.restype = lib.hp_commit_prep.restype = None
        lib.hp_cut.argtypes = [Z, V, V]
        lib.hp_commit_prep.argtypes = [Z, Z, ctypes.c_char_p, ctypes.c_char_p, V, V]
        lib.hp_open.restype = ctypes.c_uint32
        lib.hp_open.argtypes = [Z, Z, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, V, V, V]
        self.B, self.M, self.W = lib.hp_block(), lib.hp_chunk_max(), lib.hp_windows()

    def cut(self, n):
        c, g = ctypes.c_uint32(), ctypes.c_uint32()
        self.lib.hp_cut(n, ctypes.byref(c), ctypes.byref(g))
        return c.value, g.value

    def commit_prep(self, cols, base_inf=None):
        k, n = len(cols), len(cols[0])
        inf = bytes(n) if base_inf is None else bytes(base_inf)
        dig, fl = np.full((k, self.W, n), 9999, np.int16), np.full(k, 9, np.uint8)
        self.lib.hp_commit_prep(k, n, b"".join(le(x) for col in cols for x in col), inf, dig.ctypes.data, fl.ctypes.data)
        return dig, fl

    def open(self, polys, zs, base_inf=None):
        """-> digits (k, W, len - 1), values [k], flags (k,), workgroups per polynomial"""
        k, n = len(polys), len(polys[0])
        inf = bytes(max(n - 1, 1)) if base_inf is None else bytes(base_inf)
        dig, fl = np.full((k, self.W, n - 1), 9999, np.int16), np.full(k, 9, np.uint8)
        val = np.full((k, 32), 0xEE, np.uint8)
        wgs = self.lib.hp_open(k, n, b"".join(le(x) for p in polys for x in p), b"".join(le(z) for z in zs), inf,
                               dig.ctypes.data, val.ctypes.data, fl.ctypes.data)
        return dig, [int.from_bytes(v.tobytes(), "little") for v in val], fl, wgs


@pytest.fixture(scope="module")
def sim():
    subprocess.run(["make", "-C", SIM, "libhostsim_kzg_prove.so"], check=True, stdout=subprocess.DEVNULL)
    return Sim(ctypes.CDLL(os.path.join(SIM, "libhostsim_kzg_prove.so")))


def quotient(p, z):
    """the sequential recurrence: (q_0 .. q_{len-2}, v)"""
    q, carry = [0] * (len(p) - 1), 0
    for j in range(len(p) - 1, 0, -1):
        carry = (p[j] + z * carry) % R
        q[j - 1] = carry
    return q, (p[0] + z * carry) % R


def check_open(sim, polys, zs, base_inf=None):
    dig, val, fl, wgs = sim.open(polys, zs, base_inf)
    n = len(polys[0])
    assert wgs == sim.cut(n)[1]
    if n > 1:
        assert dig.min() >= -511 and dig.max() <= 512
    for c, (p, z) in enumerate(zip(polys, zs)):
        ok = z < R and all(x < R for x in p)
        assert fl[c] == (0 if ok else 2), c
        if not ok:
            continue                                # the finish stage zeroes the outputs of such a polynomial
        q, v = quotient(p, z)
        assert val[c] == v, c
        for j in range(n - 1):
            want = 0 if base_inf is not None and base_inf[j] else q[j]
            assert recombine(dig[c, :, j]) == want, (c, j)
    return wgs


def lengths(sim):
    B = sim.B
    return [1, 2, 3, B - 1, B, B + 1, 2 * B + 1, 2 * B * sim.M + 37]


def test_the_cut(sim):
    B, M = sim.B, sim.M
    assert sim.cut(1) == (1, 1) and sim.cut(B) == (1, 1) and sim.cut(B + 1) == (2, 1) and sim.cut(2 * B + 1) == (3, 1)
    assert sim.cut(B * M) == (M, 1) and sim.cut(B * M + 1) == (M, 2) and sim.cut(1 << 16) == (M, (1 << 16) // (B * M))
    chunk, wgs = sim.cut(2 * B * M + 37)
    assert chunk > 1 and wgs == 3                   # several coefficients per lane and more than one workgroup


@pytest.mark.parametrize("which", range(8))
def test_quotient_digits_and_value(sim, which):
    n = lengths(sim)[which]
    rnd = random.Random(1000 + n)
    p = [rnd.randrange(R) for _ in range(n)]
    root = rnd.randrange(R)
    pr = list(p)
    pr[0] = (p[0] - sum(x * pow(root, j, R) for j, x in enumerate(p))) % R      # pr(root) = 0
    polys = [p, p, p, pr, [rnd.randrange(R) for _ in range(n)]]
    zs = [0, 1, R - 1, root, rnd.randrange(R)]
    wgs = check_open(sim, polys, zs)
    assert (wgs > 1) == (n > sim.B * sim.M)
    _, val, _, _ = sim.open([pr], [root])
    assert val[0] == 0


@pytest.mark.parametrize("which", [2, 5, 7])
def test_defects_and_edges(sim, which):
    n = lengths(sim)[which]
    rnd = random.Random(2000 + n)
    p = [rnd.randrange(R) for _ in range(n)]
    bad = lambda j, x: p[:j] + [x] + p[j + 1:]
    top_zero = p[:max(1, n // 2)] + [0] * (n - max(1, n // 2))
    edge = [EDGE_SCALARS[j % NE] for j in range(n)]
    polys = [p, bad(0, R), bad(n // 2, (1 << 256) - 1), bad(n - 1, R + 5), top_zero, [0] * n, edge, p]
    zs = [R] + [rnd.randrange(R) for _ in range(6)] + [(1 << 256) - 1]
    dig, val, fl, _ = sim.open(polys, zs)
    assert list(fl) == [2, 2, 2, 2, 0, 0, 0, 2]
    check_open(sim, polys, zs)
    assert not dig[5].any() and val[5] == 0         # the zero polynomial


def test_a_base_at_infinity_gets_no_digits(sim):
    n = sim.B + 1
    rnd = random.Random(5)
    p = [rnd.randrange(1, R) for _ in range(n)]
    inf = [1 if j in (0, 7, n - 2) else 0 for j in range(n - 1)]
    check_open(sim, [p], [rnd.randrange(1, R)], inf)
    dig, fl = sim.commit_prep([p], inf + [1])
    assert not fl.any() and not dig[0, :, 0].any() and not dig[0, :, 7].any() and not dig[0, :, n - 1].any()
    assert recombine(dig[0, :, 1]) == p[1]


def test_commit_prep_digits_and_statuses(sim):
    rnd = random.Random(6)
    n = 300
    cols = [[rnd.randrange(R) for _ in range(n)] for _ in range(4)]
    cols[1] = [EDGE_SCALARS[j % NE] for j in range(n)]
    cols[2][150] = R
    cols.append([(1 << 256) - 1] + cols[0][1:])
    dig, fl = sim.commit_prep(cols)
    assert list(fl) == [0, 0, 2, 0, 2]
    assert dig.min() >= -511 and dig.max() <= 512
    for c, col in enumerate(cols):
        for j, x in enumerate(col):
            assert recombine(dig[c, :, j]) == (x if x < R else 0), (c, j)
