"""Case generator for the verifier's U = s*G - c*pk and V = s*H - c*Gamma (vrfhip_test_verify_uv on the device, hs_verify_uv
and its counterparts in the host simulation).  A plain module, shared by tests/test_gpu_verify_uv.py and
tests/test_hostsim_verify_uv.py.

Every point has a known discrete logarithm -- pk = a*G, H = h*G, Gamma = a*H -- so the expected values are
U = (s - c*a)*G and V = (s - c*a)*h*G, computed with the oracles' integer arithmetic only (oracle.vrf_oracle, oracle.sw_oracle,
oracle.bsw_oracle); on a slice of every set U and V are also computed literally, as s*G - c*pk and s*H - c*Gamma by the
oracles' double-and-add, and the two ways must agree.  Nothing here calls the library.

The scalars sit where the ladders' recodings change shape (the issue text lists them): c = 2^(8L) - 1 whose signed radix-16
recoding carries into window 2L, runs of -8 digits, 16-bit chunks 0x7fff / 0x8000 / 0xffff that ripple a carry through every
row of the device's 16-bit comb, the 65th digit and the 33rd comb row of secp256r1, GLV halves of the largest magnitude a
seeded search finds and halves that are zero, and (c, s, a) for which U and V are the neutral element.

cases(suite, L) -> Cases: wire arrays pk, input, output, c, s (and x || y forms), expected u, v, status.  A suite's cases for
a challenge length L hold only challenges below 2^(8L): those are compared by value."""
import math
import os
import random
import sys
from functools import lru_cache

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import bsw_oracle as bo, sw_oracle as so, vrf_oracle as vo  # noqa: E402
from tools import gen_constants as gc  # noqa: E402

SUITES = ("bandersnatch", "jubjub", "ed25519", "baby_jubjub", "secp256r1", "bandersnatch_sw")
DEFAULT_L = {"bandersnatch": 32, "jubjub": 32, "ed25519": 16, "baby_jubjub": 32, "secp256r1": 16, "bandersnatch_sw": 32}
# the non-default challenge lengths a descriptor sets: 16 on the GLV suite, 31 and 32 on one suite without an endomorphism
EXTRA_L = {"bandersnatch": (16,), "ed25519": (31, 32)}
GLV_FLOOR_LOG2 = 125.8                       # the largest half the search keeps must reach this
GLV_CAP = int("77" * 16, 16)                 # the most scalar_recode_signed4_128 can take
GLV_SEARCH = 1 << 20
N_LITERAL = 32
N_RANDOM = 128


class Group:
    """One suite's group and wire format, on top of its oracle."""

    def __init__(self, suite):
        self.suite = suite
        self.sw = suite in ("secp256r1", "bandersnatch_sw")
        if suite == "secp256r1":
            self.r, self.G, self.cofactor, self.pt_bytes, self.big_endian = so.N, so.G, 1, 33, True
            self.mul, self.add, self.neg, self.enc_in = so.mul, so.add, so.neg, so.point_encode
            self.identity, self.identity_on_wire = None, False
        elif suite == "bandersnatch_sw":
            self.r, self.G, self.cofactor, self.pt_bytes, self.big_endian = bo.R, bo.G, bo.COFACTOR, 33, False
            self.mul, self.add, self.neg, self.enc_in = bo.mul, bo.add, bo.neg, bo.point_encode
            self.identity, self.identity_on_wire = None, True
        else:
            S = {"bandersnatch": lambda: vo.BANDERSNATCH, "jubjub": vo.jubjub_params, "ed25519": vo.ed25519_params,
                 "baby_jubjub": vo.baby_jubjub_params}[suite]()
            self.S = S
            self.r, self.G, self.cofactor, self.pt_bytes, self.big_endian = S.r, (S.gx, S.gy), S.cofactor, 32, False
            self.mul = lambda k, p: vo.te_mul(S, k, p)
            self.add = lambda p, q: vo.te_add(S, p, q)
            self.neg = lambda p: vo.te_neg(S, p)
            self.enc_in = lambda p: vo.point_encode(S, p)
            self.identity, self.identity_on_wire = vo.te_identity(), True
        self.glv = suite in ("bandersnatch", "bandersnatch_sw")
        self._g = {}

    def gmul(self, k):
        """k*G, remembered (pk, H and Gamma repeat across cases)"""
        k %= self.r
        if k not in self._g:
            self._g[k] = self._gmul_windows(k) if self.suite == "secp256r1" else self.mul(k, self.G)
        return self._g[k]

    def _gmul_windows(self, k):
        """k*G as a sum of the oracle's additions over a table of j * 16^w * G: sw_oracle's affine double-and-add takes
        ~380 modular inversions per product, this takes 64 (its own double-and-add stays the reference of _check_literal)"""
        if not hasattr(self, "_win"):
            self._win, base = [], self.G
            for _ in range(64):
                row = [None, base]
                for _ in range(14):
                    row.append(self.add(row[-1], base))
                self._win.append(row)
                base = self.add(row[15], base)
        acc = None
        for w in range(64):
            acc = self.add(acc, self._win[w][(k >> (4 * w)) & 15])
        return acc

    def enc_out(self, p):
        """what the readout kernels write: the encoding the challenge hash takes, padded to the point width"""
        if self.suite == "secp256r1" and p is None:
            return bytes(33)
        return self.enc_in(p)

    def scalar(self, k):
        return int(k).to_bytes(32, "big" if self.big_endian else "little")

    def xy(self, p):
        """x || y as the x || y entry points take it (32-byte little-endian canonical integers); None for a point without one"""
        if p is None:
            return None
        return p[0].to_bytes(32, "little") + p[1].to_bytes(32, "little")

    def undecodable(self):
        """a wire string that is no point: the first small abscissa / ordinate without a root"""
        for t in range(2, 1000):
            if self.suite == "secp256r1":
                raw = b"\x02" + t.to_bytes(32, "big")
                try:
                    so.point_decode(raw)
                except ValueError:
                    return raw
            elif self.suite == "bandersnatch_sw":
                raw = t.to_bytes(32, "little") + b"\x00"
                if not bo.point_decode(raw)[0]:
                    return raw
            else:
                raw = t.to_bytes(32, "little")
                if vo.point_decode(self.S, raw) is None:
                    return raw
        raise AssertionError("no undecodable string found")

    def off_subgroup(self, p):
        """p + the point of order 2 (cofactor > 1): on the curve, outside the prime-order subgroup"""
        S = vo.BANDERSNATCH if self.suite == "bandersnatch_sw" else self.S
        t = p if self.suite != "bandersnatch_sw" else vo.sw_to_te(S, p)
        t = ((-t[0]) % S.q, (-t[1]) % S.q)
        assert vo.te_is_on_curve(S, t) and not vo.te_in_prime_subgroup(S, t)
        return bo.point_encode(vo.te_to_sw(S, t)) if self.suite == "bandersnatch_sw" else vo.point_encode(S, t)


@lru_cache(maxsize=None)
def group(suite):
    return Group(suite)


# ---- Bandersnatch GLV: fr.cuh glv_decompose_bs, restated on integers --------------------------------------------------
_GLV = gc.glv_constants()


def glv_decompose(k):
    """(k1, k2), signed, as the device splits k: Babai rounding with the 2^256-scaled multipliers of constants.gen.h"""
    g = _GLV
    c1 = g["sg1"] * ((k * g["g1"] + (1 << 255)) >> 256)
    c2 = g["sg2"] * ((k * g["g2"] + (1 << 255)) >> 256)
    k1 = k - c1 * g["a1"] - c2 * g["a2"]
    k2 = -c1 * g["b1"] - c2 * g["b2"]
    assert (k1 + k2 * g["lam"] - k) % vo.BANDERSNATCH.r == 0
    return k1, k2


@lru_cache(maxsize=None)
def glv_scalars():
    """[(tag, k)]: the 32 scalars with the largest half among GLV_SEARCH seeded ones, one per sign pair, halves that are zero
    and halves that are small.  Asserts the floor the search must reach and the cap the recoding can take."""
    r, lam = vo.BANDERSNATCH.r, _GLV["lam"]
    rng = random.Random(0x474C56)
    k, step = rng.randrange(r), rng.randrange(r)
    best = []
    floor_kept = 0
    for _ in range(GLV_SEARCH):
        k += step
        if k >= r:
            k -= r
        k1, k2 = _glv_fast(k)
        m = max(abs(k1), abs(k2))
        if m > floor_kept:
            best.append((m, k))
            if len(best) > 64:
                best.sort(reverse=True)
                del best[32:]
                floor_kept = best[-1][0]
    best.sort(reverse=True)
    best = best[:32]
    assert math.log2(best[0][0]) >= GLV_FLOOR_LOG2, math.log2(best[0][0])
    out = [("glv-max%02d" % i, kk) for i, (_, kk) in enumerate(best)]
    signs = {}
    while len(signs) < 4:
        kk = rng.randrange(r)
        k1, k2 = glv_decompose(kk)
        if k1 and k2:
            signs.setdefault((k1 < 0, k2 < 0), kk)
    out += [("glv-sign%d%d" % (a, b), kk) for (a, b), kk in sorted(signs.items())]
    out += [("glv-k2=0", 12345), ("glv-k2=0-big", (1 << 120) + 977), ("glv-k1=0", lam), ("glv-k1=0-neg", r - lam),
            ("glv-small", (3 + 5 * lam) % r), ("glv-small-neg", (r - 7 + 2 * lam) % r), ("glv-small-mixed", (9 - 4 * lam) % r)]
    for tag, kk in out:
        k1, k2 = glv_decompose(kk)
        assert abs(k1) < GLV_CAP and abs(k2) < GLV_CAP, tag
    assert glv_decompose(12345) == (12345, 0) and glv_decompose(lam) == (0, 1) and glv_decompose(r - lam) == (0, -1)
    return tuple(out)


def _glv_fast(k, _g=_GLV):
    c1 = _g["sg1"] * ((k * _g["g1"] + (1 << 255)) >> 256)
    c2 = _g["sg2"] * ((k * _g["g2"] + (1 << 255)) >> 256)
    return k - c1 * _g["a1"] - c2 * _g["a2"], -c1 * _g["b1"] - c2 * _g["b2"]


def glv_max_log2():
    return max(math.log2(max(abs(x) for x in glv_decompose(k))) for tag, k in glv_scalars() if tag.startswith("glv-max"))


# ---- scalars ----------------------------------------------------------------------------------------------------------
def _below(v, r):
    """v with its top bits cleared until it is below r"""
    while v >= r:
        v &= (1 << (v.bit_length() - 1)) - 1
    return v


def response_values(g):
    r = g.r
    bits = r.bit_length()
    out = [("s=0", 0), ("s=1", 1), ("s=2", 2), ("s=r-1", r - 1), ("s=r-2", r - 2), ("s=(r-1)/2", (r - 1) // 2),
           ("s=(r+1)/2", (r + 1) // 2)]
    for k in sorted(set(range(16, bits, 16)) | {bits - 1}):
        out += [("s=2^%d%+d" % (k, d), (1 << k) + d) for d in (-1, 0, 1) if (1 << k) + d < r]
    for name, pat in (("7", "77"), ("8", "88"), ("f", "ff"), ("78", "78"), ("87", "87")):
        out.append(("s=nib-%s" % name, _below(int(pat * 32, 16), r)))
    for pat in ("7fff", "8000", "ffff", "8001"):
        out.append(("s=chunk-%s" % pat, _below(int(pat * 16, 16), r)))
    if g.suite == "secp256r1":
        rng = random.Random(0x503235)
        n88 = int("88" * 32, 16)                    # sw_recode adds it: k >= 2^256 - n88 carries out of nibble 63 (digit 64 = 1)
        n80 = int("80" * 32, 16)                    # sw_recode8 adds it: k >= 2^256 - n80 carries out of byte 31 (comb row 32)
        out += [("s=88-pattern", n88), ("s=nib63-nocarry", (1 << 256) - n88 - 1), ("s=nib63-carry", (1 << 256) - n88),
                ("s=nib63-carry+1", (1 << 256) - n88 + 1), ("s=byte31-nocarry", (1 << 256) - n80 - 1),
                ("s=byte31-carry", (1 << 256) - n80), ("s=80-pattern", n80), ("s=n-2^32", r - (1 << 32))]
        out += [("s=n-rand%d" % i, r - 1 - rng.randrange(1 << 32)) for i in range(8)]
    assert all(0 <= v < r for _, v in out)
    return out


def challenge_values(g, L):
    r, top = g.r, 1 << (8 * L)
    vals = [("c=0", 0), ("c=1", 1), ("c=2^8L-1", top - 1), ("c=2^(8L-1)", top >> 1), ("c=2^(8L-1)-1", (top >> 1) - 1),
            ("c=8..8", int("88" * L, 16)), ("c=7..7", int("77" * L, 16)), ("c=f..f", int("ff" * L, 16))]
    if L == 32:
        vals += [(t + "-mod-r", v % r) for t, v in vals if v >= r]
    assert all(0 <= v < top for _, v in vals)
    return vals


# ---- the case sets ----------------------------------------------------------------------------------------------------
class Cases:
    """Arrays of one (suite, L) set; row i is case tags[i].  u, v, status: what the verifier's ladders must give."""

    def __init__(self, g, L, rows):
        self.suite, self.L, self.n = g.suite, L, len(rows)
        self.tags = [t for t, *_ in rows]
        pw = g.pt_bytes
        arr = lambda xs, w: np.frombuffer(b"".join(xs), np.uint8).reshape(len(xs), w).copy()
        self.pk, self.input, self.output = (arr([rw[k] for rw in rows], pw) for k in (1, 2, 3))
        self.c, self.s = (arr([rw[k] for rw in rows], 32) for k in (4, 5))
        self.u, self.v = (arr([rw[k] for rw in rows], pw) for k in (6, 7))
        self.status = np.array([rw[8] for rw in rows], np.uint8)
        # x || y forms of the rows whose three points have affine coordinates (all but a neutral pk / Gamma)
        self.xy_rows = np.array([i for i, rw in enumerate(rows) if rw[9] is not None], np.int64)
        self.pk_xy, self.input_xy, self.output_xy = (arr([rows[i][9][k] for i in self.xy_rows], 64) for k in range(3))


def _items(g, L):
    """[(tag, a, h, c, s)] of the valid cases"""
    r = g.r
    rng = random.Random("verify-uv %s %d" % (g.suite, L))
    top = min(1 << (8 * L), r) if L == 32 else 1 << (8 * L)
    rs = lambda: rng.randrange(1, r)
    rc = lambda: rng.randrange(1, top)
    a0, h0, c0, s0 = rs(), rs(), rc(), rs()
    items = [(t, a0, h0, c0, v) for t, v in response_values(g)]
    items += [(t, a0, h0, v, s0) for t, v in challenge_values(g, L)]
    if g.glv:
        for t, k in glv_scalars():
            items.append((t + "-as-s", a0, h0, c0, k))
            if k < (1 << (8 * L)):
                items.append((t + "-as-c", a0, h0, k, s0))
    # points
    c1, s1 = rc(), rs()
    if g.identity_on_wire:
        items.append(("a=0", 0, h0, c1, s1))
    items += [("a=1", 1, h0, c1, s1), ("a=r-1", r - 1, h0, c1, s1), ("h=1", a0, 1, c1, s1), ("a=1,h=1", 1, 1, c1, s1)]
    for i in range(4):
        a, h, c = rs(), rs(), rc()
        items += [("uv=O-%d" % i, a, h, c, c * a % r), ("uv=+G-%d" % i, a, h, c, (c * a + 1) % r),
                  ("uv=-G-%d" % i, a, h, c, (c * a - 1) % r)]
    items += [("uv=O,a=1", 1, h0, c1, c1 % r), ("uv=O,c=2^8L-1", a0, h0, (1 << (8 * L)) - 1, ((1 << (8 * L)) - 1) * a0 % r)]
    items += [("rand%03d" % i, rs(), rs(), rc(), rs()) for i in range(N_RANDOM)]
    return items


def _row(g, tag, a, h, c, s):
    r = g.r
    pk, H, gamma = g.gmul(a), g.gmul(h), g.gmul(a * h)
    t = (s - c * a) % r
    U, V = g.gmul(t), g.gmul(t * h)
    xy = [g.xy(p) for p in (pk, H, gamma)]
    return (tag, g.enc_in(pk), g.enc_in(H), g.enc_in(gamma), g.scalar(c), g.scalar(s), g.enc_out(U), g.enc_out(V), 0,
            None if any(x is None for x in xy) else xy)


def _check_literal(g, items):
    """U and V as the verifier's own formula, by the oracle's double-and-add, against the discrete-log way"""
    step = max(1, len(items) // N_LITERAL)
    picked = items[::step]
    assert len(picked) >= N_LITERAL
    for tag, a, h, c, s in picked:
        pk, H = g.gmul(a), g.gmul(h)
        gamma = g.mul(a, H)
        U = g.add(g.mul(s, g.G), g.neg(g.mul(c % g.r, pk)))
        V = g.add(g.mul(s, H), g.neg(g.mul(c % g.r, gamma)))
        t = (s - c * a) % g.r
        assert gamma == g.gmul(a * h) and U == g.gmul(t) and V == g.gmul(t * h), (g.suite, tag)


@lru_cache(maxsize=None)
def cases(suite, L=None):
    """The whole set of one suite at challenge length L (default: the suite's own), invalid items last."""
    g = group(suite)
    L = DEFAULT_L[suite] if L is None else L
    items = _items(g, L)
    assert all(c < (1 << (8 * L)) and s < g.r for _, _, _, c, s in items)
    assert len(items) < 800
    _check_literal(g, items)
    rows = [_row(g, *it) for it in items]
    # invalid items: status 2, zero bytes
    rng = random.Random("verify-uv invalid %s" % suite)
    a, h, c, s = (rng.randrange(1, g.r) for _ in range(4))
    c %= 1 << (8 * L)
    pk, H, gamma = (g.enc_in(p) for p in (g.gmul(a), g.gmul(h), g.gmul(a * h)))
    z = bytes(g.pt_bytes)
    rows.append(("bad:s=r", pk, H, gamma, g.scalar(c), g.scalar(g.r), z, z, 2, None))
    rows.append(("bad:gamma", pk, H, g.undecodable(), g.scalar(c), g.scalar(s), z, z, 2, None))
    if g.cofactor > 1:
        rows.append(("bad:pk-cofactor", g.off_subgroup(g.gmul(a)), H, gamma, g.scalar(c), g.scalar(s), z, z, 2, None))
    return Cases(g, L, rows)


class KeyedCases:
    """Every challenge case of the set above under each of three keys of an 8-key set (a = 0 where the wire format has the
    neutral element, a = 1, a = r - 1 among them), and one item whose index names no key (status 2)."""

    def __init__(self, suite, L=None):
        g = group(suite)
        L = DEFAULT_L[suite] if L is None else L
        r = g.r
        rng = random.Random("verify-uv keyed %s %d" % (suite, L))
        keys = [0 if g.identity_on_wire else 2, 1, r - 1] + [rng.randrange(1, r) for _ in range(5)]
        self.keys = np.frombuffer(b"".join(g.enc_in(g.gmul(a)) for a in keys), np.uint8).reshape(8, g.pt_bytes).copy()
        h, s = rng.randrange(1, r), rng.randrange(1, r)
        cs = challenge_values(g, L)
        if g.glv and L == 32:
            cs = cs + [(t, k) for t, k in glv_scalars()[:8]]
        rows, idx = [], []
        for t, c in cs:
            for ki in (0, 1, 2):
                rows.append(_row(g, "%s,key%d" % (t, ki), keys[ki], h, c, s))
                idx.append(ki)
        for ki in range(3, 8):
            rows.append(_row(g, "rand,key%d" % ki, keys[ki], h, rng.randrange(1 << (8 * L)) % r, rng.randrange(r)))
            idx.append(ki)
        z = bytes(g.pt_bytes)
        last = rows[-1]
        rows.append(("bad:index", last[1], last[2], last[3], last[4], last[5], z, z, 2, None))
        idx.append(8)
        self.cases = Cases(g, L, rows)
        self.key_index = np.array(idx, np.uint32)


@lru_cache(maxsize=None)
def keyed_cases(suite, L=None):
    return KeyedCases(suite, L)
