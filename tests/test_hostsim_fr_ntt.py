"""CPU: the per-lane functions of the radix-2 transforms over Fr (fr_ntt.cuh: ntt_load_lane, ntt_bfly_lane, ntt_store_lane,
ntt_add / ntt_sub, the domain tables) compiled for the host (tests/hostsim_fr_ntt) against Python integers
(tests/fr_ntt_ref.py).  The host program restates the kernels' shape -- the pass plan, one tile per workgroup, the tile
addressing, the twiddle indexing, the scalings -- and exports T and the plan.  Two builds run: `big` is the kernels' tile
(T = 11, rows of 8), `small` the same code with T = 6 and rows of 4, where plans of two and three passes occur from 2^7 on.

Sizes.  The issue asks for every log_n up to 2 T + 1.  A domain is refused above 2^20 (the limit of a base set), so `big`
stops there instead of at 2^23; `small` stops at 2^12, the largest size its three passes hold.  Up to 2^17 every form is
compared with the recursive reference; 2^18 .. 2^20 are compared on the plain domain with closed forms of sparse polynomials
(all n outputs) and by the round trip, because the recursion takes a quarter of a minute there and the host build of the
coset tables as long."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import fr_ntt_ref as ref

R = ref.R
HERE = os.path.dirname(os.path.abspath(__file__))
SIM = os.path.join(HERE, "hostsim_fr_ntt")
RMONT = 1 << 261                                      # the Montgomery radix of fe.cuh
EDGE, NE = ref.EDGE_SCALARS, len(ref.EDGE_SCALARS)
FULL_MAX = 17                                         # exact comparison against the recursive reference up to here


def limbs_int(row):
    return sum(int(v) << (29 * i) for i, v in enumerate(row))


class Domain:
    def __init__(self, sim, log_n, offset):
        n = 1 << log_n
        self.log_n, self.n, self.offset = log_n, n, offset
        self.w = np.zeros((n, 9), np.uint32)
        self.consts = np.zeros((3, 9), np.uint32)
        self.off = self.offi = None
        if offset is not None:
            self.off, self.offi = np.zeros((n, 9), np.uint32), np.zeros((n, 9), np.uint32)
        p = lambda a: a.ctypes.data if a is not None else None
        self.ok = sim.lib.hn_domain(log_n, None if offset is None else int(offset).to_bytes(32, "little"), p(self.w),
                                    p(self.off), p(self.offi), p(self.consts))


class Sim:
    def __init__(self, lib):
        self.lib = lib
        V, Z, U = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32
        for f in ("hn_t", "hn_logc", "hn_max_log", "hn_block", "hn_tile_words"):
            getattr(lib, f).restype = ctypes.c_int
        lib.hn_plan.restype = ctypes.c_int
        lib.hn_plan.argtypes = [ctypes.c_int, V]
        lib.hn_domain.restype = ctypes.c_int
        lib.hn_domain.argtypes = [U, ctypes.c_char_p, V, V, V, V]
        lib.hn_ntt.restype = None
        lib.hn_ntt.argtypes = [U, Z, ctypes.c_int, V, V, V, V, V, V, V]
        lib.hn_addsub.restype = None
        lib.hn_addsub.argtypes = [V, V, V, V]
        self.T, self.LOGC, self.MAX = lib.hn_t(), lib.hn_logc(), lib.hn_max_log()
        self._domains = {}

    def plan(self, log_n):
        bits = (ctypes.c_int * 3)()
        p = self.lib.hn_plan(log_n, bits)
        return list(bits)[:p]

    def domain(self, log_n, offset=None):
        key = (log_n, offset)
        if key not in self._domains:
            self._domains[key] = Domain(self, log_n, offset)
        return self._domains[key]

    def ntt(self, dom, cols, inverse=False, in_place=False):
        """-> (columns of integers, statuses)"""
        k, n = len(cols), dom.n
        src = np.frombuffer(ref.to_bytes(cols), np.uint8).copy()
        dst = src if in_place else np.full(k * n * 32, 0xEE, np.uint8)
        st = np.full(k, 9, np.uint8)
        p = lambda a: a.ctypes.data if a is not None else None
        self.lib.hn_ntt(dom.log_n, k, int(inverse), p(dom.w), p(dom.off), p(dom.offi), p(dom.consts), p(src), p(dst), p(st))
        return ref.from_bytes(dst.tobytes(), k, n), list(st)


def _load(name):
    subprocess.run(["make", "-C", SIM, name], check=True, stdout=subprocess.DEVNULL)
    return Sim(ctypes.CDLL(os.path.join(SIM, name)))


@pytest.fixture(scope="module")
def big():
    return _load("libhostsim_fr_ntt.so")


@pytest.fixture(scope="module")
def small():
    return _load("libhostsim_fr_ntt_small.so")


@pytest.fixture(scope="module", params=["small", "big"])
def sim(request):
    return request.getfixturevalue(request.param)


def test_the_reference_agrees_with_direct_evaluation():
    assert ref.self_check()
    assert ref.ROOT == 0x16a2a19edfe81f20d09b681922c813b4b63683508c2280b93829971f439f0d2b
    assert pow(ref.ROOT, 1 << 31, R) == R - 1


def test_the_plan(big, small):
    assert (big.T, big.LOGC, big.MAX) == (11, 3, 20) and (small.T, small.LOGC, small.MAX) == (6, 2, 12)
    for s in (big, small):
        B = s.T - s.LOGC
        for log_n in range(s.MAX + 1):
            bits = s.plan(log_n)
            assert sum(bits) == log_n
            if log_n <= s.T:
                assert bits == [log_n]                           # one pass, one launch
            else:
                assert len(bits) == -(-log_n // B) <= 3 and max(bits) <= B and min(bits) >= s.LOGC
    assert big.plan(11) == [11] and big.plan(12) == [6, 6] and big.plan(16) == [8, 8] and big.plan(17) == [6, 6, 5]
    assert big.plan(20) == [7, 7, 6]
    assert small.plan(7) == [4, 3] and small.plan(8) == [4, 4] and small.plan(9) == [3, 3, 3]


def boundary_positions(sim, log_n):
    """first, last, and the places where a tile, a row or a pass's block begins or ends"""
    n, pos = 1 << log_n, {0, (1 << log_n) - 1}
    marks = {1 << sim.LOGC, 1 << sim.T, n >> 1}
    acc = 0
    for b in reversed(sim.plan(log_n)):
        acc += b
        marks.add(1 << acc)
    for m in marks:
        for p in (m - 1, m, m + 1, n - m, n - m - 1):
            if 0 <= p < n:
                pos.add(p)
    return sorted(pos)


def edge_columns(sim, log_n):
    n = 1 << log_n
    cols = []
    for rot in range(3 if log_n <= 12 else 1):
        col = [EDGE[j % NE] for j in range(n)]
        for q, p in enumerate(boundary_positions(sim, log_n)):
            col[p] = (0, 1, R - 1)[(q + rot) % 3]
        cols.append(col)
    return cols


def offsets_for(log_n):
    return [None, ref.GENERATOR if log_n % 2 else random.Random(log_n).randrange(2, R)]


def run_forms(sim, log_n, cols, want_by_offset):
    """forward against the expected values, inverse of those values back to the columns, for both domains; the round trip
    in place"""
    for offset in want_by_offset:
        dom = sim.domain(log_n, offset)
        assert dom.ok
        want = want_by_offset[offset]
        got, st = sim.ntt(dom, cols)
        assert st == [0] * len(cols)
        assert got == want, (log_n, offset, "forward")
        back, st = sim.ntt(dom, want, inverse=True, in_place=True)
        assert st == [0] * len(cols)
        assert back == cols, (log_n, offset, "inverse")


def cases(which):
    small_max, big_max = 12, FULL_MAX
    return [(which, n) for n in range((small_max if which == "small" else big_max) + 1)]


@pytest.mark.parametrize("which,log_n", cases("small") + cases("big"))
def test_every_size_in_four_forms(request, which, log_n):
    sim = request.getfixturevalue(which)
    n = 1 << log_n
    rnd = random.Random(4000 + log_n)
    cols = [[rnd.randrange(R) for _ in range(n)]] + edge_columns(sim, log_n)
    if log_n <= 14:
        cols.append([rnd.randrange(R) for _ in range(n)])
    want = {}
    for offset in offsets_for(log_n):
        want[offset] = [ref.fft(c, 1 if offset is None else offset) for c in cols]
    run_forms(sim, log_n, cols, want)


@pytest.mark.parametrize("which,log_n", cases("small") + cases("big") + [("big", 18), ("big", 19), ("big", 20)])
def test_closed_forms(request, which, log_n):
    """the zero column, the constant polynomial and the constant column, X^(n-1) alone, and three far-apart terms"""
    sim = request.getfixturevalue(which)
    n = 1 << log_n
    rnd = random.Random(5000 + log_n)
    c0, c1, c2 = (rnd.randrange(1, R) for _ in range(3))
    sparse = [(0, c0)] if n == 1 else [(0, c0), (n - 1, c2)] if n < 8 else [(0, c0), (n // 2 + 1, c1), (n - 1, c2)]
    cols = [[0] * n, ref.sparse_column([(0, c0)], log_n), ref.sparse_column([(n - 1, R - 1)], log_n),
            ref.sparse_column(sparse, log_n)]
    want = {}
    for offset in offsets_for(log_n)[:2 if log_n <= FULL_MAX else 1]:
        o = 1 if offset is None else offset
        want[offset] = [[0] * n, [c0] * n, ref.sparse_evals([(n - 1, R - 1)], log_n, o), ref.sparse_evals(sparse, log_n, o)]
    run_forms(sim, log_n, cols, want)
    if log_n <= FULL_MAX:
        # the constant COLUMN as coefficients: c (x^n - 1) / (x - 1), on the plain domain c n at w^0 and zero elsewhere
        got, _ = sim.ntt(sim.domain(log_n), [[c1] * n])
        assert got == [[c1 * n % R] + [0] * (n - 1)]


def test_size_one_is_the_identity(sim):
    for offset in (None, ref.GENERATOR, R - 1):
        dom = sim.domain(0, offset)
        for x in (0, 1, R - 1, 12345):
            for inverse in (False, True):
                assert sim.ntt(dom, [[x]], inverse=inverse) == ([[x]], [0])


@pytest.mark.parametrize("which,log_n", [("small", 0), ("small", 1), ("small", 3), ("small", 6), ("small", 7), ("small", 9),
                                         ("big", 4), ("big", 11), ("big", 12), ("big", 17)])
def test_a_scalar_out_of_range_refuses_its_column_only(request, which, log_n):
    sim = request.getfixturevalue(which)
    n = 1 << log_n
    rnd = random.Random(6000 + log_n)
    p = [rnd.randrange(R) for _ in range(n)]
    bad = lambda j, x: p[:j] + [x] + p[j + 1:]
    cols = [p, bad(0, R), bad(n // 2, (1 << 256) - 1), bad(n - 1, R + 5), p]
    for offset in offsets_for(log_n):
        o = 1 if offset is None else offset
        dom = sim.domain(log_n, offset)
        for inverse, want in ((False, ref.fft(p, o)), (True, ref.ifft(p, o))):
            got, st = sim.ntt(dom, cols, inverse=inverse)
            assert st == [0, 2, 2, 2, 0]
            assert got == [want, [0] * n, [0] * n, [0] * n, want]


@pytest.mark.parametrize("which,log_n", cases("small") + cases("big"))
def test_the_domain_tables(request, which, log_n):
    sim = request.getfixturevalue(which)
    n, w = 1 << log_n, ref.omega(log_n)
    assert pow(w, n, R) == 1 and (n == 1 or pow(w, n // 2, R) == R - 1)          # order exactly n
    offset = offsets_for(log_n)[1]
    dom = sim.domain(log_n, offset)
    mont = lambda x: x * RMONT % R
    ninv = limbs_int(dom.consts[0])
    assert ninv == mont(pow(n, -1, R)) and ninv * pow(RMONT, -1, R) * n % R == 1
    assert limbs_int(dom.consts[1]) == mont(offset) and limbs_int(dom.consts[2]) == mont(pow(offset, -1, R))
    step = 1 if log_n <= 12 else 257
    idx = sorted(set(range(0, n, step)) | {n - 1, n // 2})
    oinv, nin = pow(offset, -1, R), pow(n, -1, R)
    for i in idx:
        assert limbs_int(dom.w[i]) == mont(pow(w, i, R)), i
        assert limbs_int(dom.off[i]) == mont(pow(offset, i, R)), i
        assert limbs_int(dom.offi[i]) == mont(nin * pow(oinv, i, R) % R), i
    assert dom.w.max() < 1 << 29                                                  # canonical images, exact limbs
    plain = sim.domain(log_n)
    assert plain.off is None and (plain.w == dom.w).all()


def test_offsets_that_are_refused(small):
    for offset in (0, R, R + 7, (1 << 256) - 1):
        assert not Domain(small, 3, offset).ok
    assert Domain(small, 3, 1).ok and Domain(small, 3, R - 1).ok


def test_add_and_sub_stay_below_2q_with_exact_limbs(small):
    rnd = random.Random(7)
    vals = [0, 1, R - 1, R, R + 1, 2 * R - 1, 2 * R - 2, (1 << 255), (1 << 255) - 1] + [rnd.randrange(2 * R) for _ in range(40)]
    to_limbs = lambda x: np.array([(x >> (29 * i)) & ((1 << 29) - 1) if i < 8 else x >> 232 for i in range(9)], np.uint32)
    for a in vals:
        for b in vals:
            s, d, la, lb = np.zeros(9, np.uint32), np.zeros(9, np.uint32), to_limbs(a), to_limbs(b)
            small.lib.hn_addsub(la.ctypes.data, lb.ctypes.data, s.ctypes.data, d.ctypes.data)
            assert s[:8].max() < 1 << 29 and d[:8].max() < 1 << 29
            assert limbs_int(s) == (a + b) % (2 * R) and limbs_int(d) == (a - b) % (2 * R)
