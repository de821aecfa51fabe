"""CPU: the BLS12-381 G1 codec (g1_codec.cuh: fp_sqrt, g1_decode_item, g1_validate_item, g1_encode_item) compiled for the
host (tests/hostsim_g1codec) against a decoder of a few lines of Python ints: the golden encodings, random valid points with
both sort flags, every malformed class, the order-3 point with the subgroup test on and off, and -- the check that catches a
wrong beta or an unsound shortcut -- the subgroup test against r P = O on points of every prime order dividing the cofactor."""
import ctypes
import json
import os
import random
import subprocess

import pytest

from oracle import bls_oracle as bls

P, R, X_ABS = bls.P, bls.R, bls.X_ABS
HERE = os.path.dirname(os.path.abspath(__file__))
SIM = os.path.join(HERE, "hostsim_g1codec")
ORDER = P + X_ABS                      # #E(Fp) = p + 1 - t, t = x + 1, x = -X_ABS
COFACTOR = (X_ABS + 1) ** 2 // 3
ELLS = (3, 11, 10177, 859267, 52437899)
BAD96, BAD48 = b"\xff" * 96, b"\xff" * 48


# ---------------------------------------------------------------------------------- the test's own codec
def py_decode(b, check_subgroup=True):
    """(status, 96 bytes) by the format's definition: strict infinity rule, subgroup by r P = O."""
    comp, inf, srt = b[0] >> 7 & 1, b[0] >> 6 & 1, b[0] >> 5 & 1
    x = int.from_bytes(bytes([b[0] & 0x1F]) + b[1:], "big")
    if not comp:
        return 2, BAD96
    if inf:
        return (0, bytes(96)) if not srt and x == 0 else (2, BAD96)
    if x >= P:
        return 2, BAD96
    a = (x ** 3 + 4) % P
    y = pow(a, (P + 1) // 4, P)
    if y * y % P != a:
        return 2, BAD96
    if (y > P - y) != bool(srt):
        y = (P - y) % P
    if check_subgroup and bls.g1_mul(R, (x, y)) is not None:
        return 2, BAD96
    return 0, xy96((x, y))


def py_encode(pt):
    if pt is None:
        return bytes([0xC0]) + bytes(47)
    b = bytearray(pt[0].to_bytes(48, "big"))
    b[0] |= 0x80 | (0x20 if pt[1] > P - pt[1] else 0)
    return bytes(b)


def xy96(pt):
    return bytes(96) if pt is None else pt[0].to_bytes(48, "little") + pt[1].to_bytes(48, "little")


def curve_point(rnd):
    while True:
        x = rnd.randrange(P)
        a = (x ** 3 + 4) % P
        y = pow(a, (P + 1) // 4, P)
        if y * y % P == a:
            return (x, y if rnd.getrandbits(1) else (P - y) % P)


def torsion_point(ell, rnd):
    """A point of exact order ell (prime, dividing the cofactor): the ell-part of a random curve point, multiplied by ell
    until one more step would give infinity.  ((#E / ell) Q alone is always infinity where ell^2 | #E and the ell-part of the
    group is not cyclic.)"""
    m = ORDER
    while m % ell == 0:
        m //= ell
    while True:
        T = bls.g1_mul(m, curve_point(rnd))
        if T is None:
            continue
        while bls.g1_mul(ell, T) is not None:
            T = bls.g1_mul(ell, T)
        return T


def non_square_x(rnd):
    while True:
        x = rnd.randrange(P)
        if pow((x ** 3 + 4) % P, (P - 1) // 2, P) == P - 1:
            return x


def malformed(rnd):
    """(label, 48 bytes) for every class the decoder must refuse."""
    g = py_encode(bls.G1)
    raw = lambda x, flags: bytes([flags | (x >> 376)]) + (x & ((1 << 376) - 1)).to_bytes(47, "big")
    out = [("compressed bit clear", bytes([g[0] & 0x7F]) + g[1:]),
           ("uncompressed infinity flag only", bytes([0x40]) + bytes(47)),
           ("infinity + sort", bytes([0xE0]) + bytes(47)),
           ("infinity + low x bit", bytes([0xC0]) + bytes(46) + b"\x01"),
           ("infinity + high x bit", bytes([0xD0]) + bytes(47)),
           ("x = p", raw(P, 0x80)), ("x = p, sort", raw(P, 0xA0)),
           ("x = p + 1", raw(P + 1, 0x80)),
           ("x = 2^381 - 1", raw((1 << 381) - 1, 0x80)), ("x = 2^381 - 1, sort", raw((1 << 381) - 1, 0xA0)),
           ("non-square", raw(non_square_x(rnd), 0x80)), ("non-square, sort", raw(non_square_x(rnd), 0xA0))]
    return out


# ---------------------------------------------------------------------------------- the simulation
class Sim:
    def __init__(self, lib):
        self.lib = lib
        lib.hg_fp_sqrt.restype = ctypes.c_int
        for f in (lib.hg_decode, lib.hg_validate, lib.hg_encode):
            f.restype = None
        lib.hg_decode.argtypes = [ctypes.c_size_t, ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p]
        lib.hg_validate.argtypes = [ctypes.c_size_t, ctypes.c_char_p, ctypes.c_char_p]
        lib.hg_encode.argtypes = [ctypes.c_size_t, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p]

    def sqrt(self, a):
        out = ctypes.create_string_buffer(48)
        ok = self.lib.hg_fp_sqrt(a.to_bytes(48, "little"), out)
        return ok, int.from_bytes(out.raw, "little")

    def decode(self, encs, check_subgroup=True):
        n = len(encs)
        out, st = ctypes.create_string_buffer(96 * n), ctypes.create_string_buffer(n)
        self.lib.hg_decode(n, b"".join(encs), int(check_subgroup), out, st)
        return [(st.raw[i], out.raw[96 * i:96 * i + 96]) for i in range(n)]

    def validate(self, xys):
        n = len(xys)
        st = ctypes.create_string_buffer(n)
        self.lib.hg_validate(n, b"".join(xys), st)
        return list(st.raw)

    def encode(self, xys):
        n = len(xys)
        out, st = ctypes.create_string_buffer(48 * n), ctypes.create_string_buffer(n)
        self.lib.hg_encode(n, b"".join(xys), out, st)
        return [(st.raw[i], out.raw[48 * i:48 * i + 48]) for i in range(n)]


@pytest.fixture(scope="module")
def sim():
    subprocess.run(["make", "-C", SIM, "libhostsim_g1codec.so"], check=True, stdout=subprocess.DEVNULL)
    return Sim(ctypes.CDLL(os.path.join(SIM, "libhostsim_g1codec.so")))


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(HERE, "golden", "bls12_381_g1_compressed.json")))["vectors"]


@pytest.fixture(scope="module")
def subgroup_points():
    """300 random points of the prime-order subgroup, computed once: a walk over 16 random multiples of the generator (one
    addition per point instead of one scalar multiplication)."""
    rnd = random.Random(381)
    steps = [bls.g1_mul(rnd.randrange(1, R), bls.G1) for _ in range(16)]
    pts, acc = [], bls.g1_mul(rnd.randrange(1, R), bls.G1)
    while len(pts) < 300:
        acc = bls.g1_add(acc, rnd.choice(steps))
        if acc is not None:
            pts.append(acc)
    return pts


def test_group_constants():
    assert COFACTOR * R == ORDER and X_ABS ** 4 - X_ABS ** 2 + 1 == R
    n = COFACTOR
    for ell in ELLS:
        assert n % ell == 0
        while n % ell == 0:
            n //= ell
    assert n == 1, "the primes dividing the cofactor"


def test_fp_sqrt(sim):
    rnd = random.Random(1)
    squares = [0, 1, 4] + [pow(rnd.randrange(1, P), 2, P) for _ in range(200)]
    non_squares = [P - 1]                                  # p = 3 (mod 4): -1 is a non-residue
    while len(non_squares) < 201:
        a = rnd.randrange(1, P)
        if pow(a, (P - 1) // 2, P) == P - 1:
            non_squares.append(a)
    for a in squares:
        ok, root = sim.sqrt(a)
        assert ok == 1 and root == pow(a, (P + 1) // 4, P) and root * root % P == a, hex(a)
    for a in non_squares:
        ok, root = sim.sqrt(a)
        assert ok == 0 and root == pow(a, (P + 1) // 4, P), hex(a)


def test_golden_file_is_what_the_authentication_script_writes(golden):
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "authenticate_bls_g1_vectors", os.path.join(HERE, "..", "tools", "authenticate_bls_g1_vectors.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.G == (bls.G1X, bls.G1Y) and mod.p == P and mod.r == R
    assert mod.vectors()["vectors"] == golden
    g = next(v for v in golden if v["name"] == "G")
    assert g["origin"].startswith("recalled") and g["compressed"] == mod.G_COMPRESSED


def test_decode_golden(sim, golden):
    encs = [bytes.fromhex(v["compressed"]) for v in golden]
    for v, (st, xy) in zip(golden, sim.decode(encs)):
        x, y = int(v["x"], 16), int(v["y"], 16)
        want = bytes(96) if v["name"] == "infinity" else xy96((x, y))
        assert (st, xy) == (0, want) == py_decode(bytes.fromhex(v["compressed"])), v["name"]
        if v["name"] != "infinity":
            assert (x, y) == bls.g1_mul(int(v["k"], 16), bls.G1), v["name"]


def test_decode_random_valid_points_both_sort_flags(sim, subgroup_points):
    encs, want = [], []
    for pt in subgroup_points:
        for q in (pt, bls.g1_neg(pt)):
            encs.append(py_encode(q))
            want.append((0, xy96(q)))
    assert {e[0] >> 5 for e in encs} == {4, 5}
    assert sim.decode(encs) == want
    assert sim.decode(encs, False) == want
    for e, w in list(zip(encs, want))[:40]:                 # the Python decoder itself, r P = O included
        assert py_decode(e) == w


def test_decode_refuses_every_malformed_class(sim):
    cases = malformed(random.Random(2))
    encs = [e for _, e in cases]
    for on in (True, False):
        for (label, e), got in zip(cases, sim.decode(encs, on)):
            assert got == (2, BAD96) == py_decode(e, on), (label, on)


def test_order_three_point(sim):
    """x = 0 gives y = +/-2: on the curve, of order 3."""
    assert bls.g1_mul(3, (0, 2)) is None
    for flags, y in ((0x80, 2), (0xA0, P - 2)):
        e = bytes([flags]) + bytes(47)
        assert sim.decode([e], True) == [(2, BAD96)] == [py_decode(e, True)]
        assert sim.decode([e], False) == [(0, xy96((0, y)))] == [py_decode(e, False)]
        assert sim.validate([xy96((0, y))]) == [2]


@pytest.mark.parametrize("ell", ELLS)
def test_subgroup_test_against_r_times_p(sim, ell, subgroup_points):
    rnd = random.Random(ell)
    T = torsion_point(ell, rnd)
    pts = [T, bls.g1_add(bls.G1, T)]
    pts += [curve_point(rnd) for _ in range(20)]
    pts += rnd.sample(subgroup_points, 20)
    want = [0 if bls.g1_mul(R, pt) is None else 2 for pt in pts]
    assert want[:2] == [2, 2] and want[22:] == [0] * 20
    assert sim.validate([xy96(pt) for pt in pts]) == want
    got = sim.decode([py_encode(pt) for pt in pts], True)
    assert got == [(0, xy96(pt)) if w == 0 else (2, BAD96) for pt, w in zip(pts, want)]
    assert sim.decode([py_encode(pt) for pt in pts], False) == [(0, xy96(pt)) for pt in pts]


def test_validate_range_curve_and_infinity(sim):
    gx, gy = bls.G1
    cases = [(xy96(None), 0), (xy96(bls.G1), 0), (xy96((gx, P - gy)), 0),
             (xy96((gx, (gy + 1) % P)), 2), (xy96(((gx + 1) % P, gy)), 2),
             (P.to_bytes(48, "little") + gy.to_bytes(48, "little"), 2),
             (gx.to_bytes(48, "little") + (gy + P).to_bytes(48, "little"), 2),
             (bytes(48) + (2).to_bytes(48, "little"), 2), (BAD96, 2)]
    assert sim.validate([c for c, _ in cases]) == [w for _, w in cases]


def test_encode_and_round_trips(sim, golden, subgroup_points):
    rnd = random.Random(3)
    pts = [None] + subgroup_points[:60] + [bls.g1_neg(q) for q in subgroup_points[:60]] + [curve_point(rnd) for _ in range(20)]
    xys = [xy96(q) for q in pts]
    enc = sim.encode(xys)
    assert enc == [(0, py_encode(q)) for q in pts]
    # decode o encode = identity on valid points (no subgroup test: the random curve points are outside it)
    assert sim.decode([e for _, e in enc], False) == [(0, xy) for xy in xys]
    # encode o decode = identity on canonical encodings
    canon = [bytes.fromhex(v["compressed"]) for v in golden]
    dec = sim.decode(canon, True)
    assert [st for st, _ in dec] == [0] * len(canon)
    assert sim.encode([xy for _, xy in dec]) == [(0, e) for e in canon]
    # invalid affine input: coordinate >= p, off the curve, the decoder's own 0xFF marker
    gx, gy = bls.G1
    bad = [xy96((gx, (gy + 1) % P)), P.to_bytes(48, "little") + gy.to_bytes(48, "little"),
           gx.to_bytes(48, "little") + P.to_bytes(48, "little"), BAD96, bytes(48) + (1).to_bytes(48, "little")]
    assert sim.encode(bad) == [(2, BAD48)] * len(bad)
