"""Case generator for the provers (vrfhip_ietf_prove_batch / vrfhip_pedersen_prove_batch on the device; hs_ / hj_ / hx_ / hp_ /
hb_prove_cases in the host simulation).  A plain module, shared by tests/test_gpu_prove_cases.py and
tests/test_hostsim_prove_cases.py; it imports only the oracles and verify_uv_cases.  Nothing here calls the library.

Every case is a secret sk and a given input H.  H has a known discrete logarithm, H = h*G (the one exception is H = the blinding
base, whose logarithm nobody knows: there Gamma is sk*B by the Python oracle's additions), so pk = sk*G and Gamma = (sk*h mod r)*G
follow from the Python oracles' integer arithmetic alone; on a slice of N_LITERAL cases both are also computed literally, as sk*G
and sk*H by the oracles' double-and-add, and the two ways must agree.  Everything behind a hash -- c, s, and for Pedersen pk_com, R,
Ok, s, sb and the blinding factor -- comes from the C oracle (plain double-and-add), configured like the test contexts: its own
blinding base on Bandersnatch, the test base elsewhere, every point class subgroup-checked.  Its status is the expected status.

The secrets sit where the provers' recodings change shape; each family is built by a function that ASSERTS, on integers and
with the small recoders below (signed radix-16, the 16-bit and 8-bit combs, secp256r1's fold, the GLV split), that its members
have the property they are named for.  A family that comes out empty is an error.  Families (tags carry the family before ':'):

  small     0, 1, 2, 7, 8, 9, 15, 16, 17, r-1, r-2, r-8, r-9, (r-1)/2, (r+1)/2; secp256r1: (n-3)/2 and (n+3)/2 as well (for an
            odd n, (n+1)/2 and (n-1)/2 are already the smallest k above n/2 and the largest below it)
  nib       the largest value below r whose nibbles are all 7, all 8, all 9, alternate 7/8 (both phases); the smallest and the
            largest value below r whose recoding carries into the top window (the Edwards orders are below 2^253, so no
            canonical scalar carries OUT of nibble 63 there; on secp256r1 that is the fold family)
  fold      secp256r1: |k'| = 0x77..78 (the smallest magnitude that takes the `top && j == 3 && i == 15` branch of sw_quad_mul),
            0x77..77 (its neighbour that does not), (n-1)/2 (the largest that does), each as k and as n - k
  stream    2^64, 2^128, 2^192 alone; each minus one; 2^(64 j) +- 8; -8 in the last digit of stream j - 1 with its carry into the
            first of stream j; four equal streams of 16 digits; only the top stream (secp256r1: all below n/2, the fold keeps them)
  comb      16-bit chunks 0x7fff / 0x8000 / 0xffff in every row, in row 0 only, in row 14 only (row 15 takes the carry of a chunk
            >= 0x8000, and no canonical scalar of an Edwards suite fills it);
            2^(16 w) and 2^(16 w) - 1 for every w; bytes 0x7f / 0x80 / 0xff throughout (the 8-bit comb of the host simulation and
            sw_recode8); secp256r1: 2^256 - 0x80..80 and the value below it (comb row 32)
  glv       Bandersnatch, bandersnatch_sw: k2 = 0, k1 = 0 (small multiples of lambda), the four sign pairs, and the N_GLV_MAX
            secrets of the largest half verify_uv_cases' seeded search of 2^20 finds (its floor and cap are asserted there)
  range     r, r + 1, 2^253, 2^255, 2^256 - 1: refused exactly where the value is >= r (on secp256r1 2^253 and 2^255 are secrets)
  rand      N_RANDOM random secrets

Given inputs, crossed with INPUT_SECRETS (1, 2, r-1, (r+1)/2, the all-8 nibble value, one random secret, 0): G, -G, 2G, the
blinding base, h*G for two random h, H = pk of the same item (not for sk = 0: that is the neutral input again), the neutral
element in the encodings the codec has for it, one undecodable string, and one point outside the prime-order subgroup where the
cofactor is above one.  The three lengths of ad (0, 16, 200 bytes) go with the whole set.  The count is made odd (one more random
case if need be), so that the last lane is part full at 2, 4 and 8 proofs per lane.

cases(suite) -> Cases.  A refused item's expected outputs are zero bytes; the oracle writes no `input` for it, so none is expected."""
import os
import random
import sys
from functools import lru_cache

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import bsw_oracle as bo, c_oracle as co, sw_oracle as so, vrf_oracle as vo  # noqa: E402
from verify_uv_cases import DEFAULT_L, SUITES, _below, glv_decompose, glv_scalars, group  # noqa: E402,F401
from pedersen_c_cases import CURVE_ID, blinding  # noqa: E402

N_RANDOM = 128
N_LITERAL = 32
N_GLV_MAX = 16
MAX_CASES = 500
ADS = (b"", bytes(range(16)), bytes((7 * i + 3) & 255 for i in range(200)))
MSG_LEN = 24
THREADS = min(8, os.cpu_count() or 1)
IETF_KEYS = ("output", "c", "s", "pk", "input")
PED_KEYS = ("output", "pk_com", "r", "ok", "s", "sb", "blinding", "input")


# ---- the recoders, restated on integers ---------------------------------------------------------------------------------------
def rec16(k):
    """fr.cuh scalar_recode_signed4 / p256_core.cuh sw_recode: (digits d_w in [-8, 7] for w = 0..63, carry into each window,
    carry out of nibble 63)"""
    digits, carries, c = [], [], 0
    for w in range(64):
        carries.append(c)
        v = ((k >> (4 * w)) & 15) + 8 + c
        c = v >> 4
        digits.append((v & 15) - 8)
    assert sum(d << (4 * w) for w, d in enumerate(digits)) + (c << 256) == k
    return digits, carries, c


def comb_digits(k, bits):
    """vrf_core.cuh gcomb_digit with a window of `bits`: (signed digits, carry into each row, carry out of the top row)"""
    digits, carries, c = [], [], 0
    for w in range(256 // bits):
        carries.append(c)
        chunk = ((k >> (bits * w)) & ((1 << bits) - 1)) + c
        c = 1 if chunk >= 1 << (bits - 1) else 0
        digits.append(chunk - (c << bits))
    assert sum(d << (bits * w) for w, d in enumerate(digits)) + (c << 256) == k
    return digits, carries, c


def rec8_p256(k):
    """p256_core.cuh sw_recode8: (byte digits in [-128, 127], digit 32)"""
    x = k + int("80" * 32, 16)
    digits = [((x >> (8 * w)) & 255) - 128 for w in range(32)]
    assert sum(d << (8 * w) for w, d in enumerate(digits)) + ((x >> 256) << 256) == k
    return digits, x >> 256


def fold(k, n):
    """p256_core.cuh sw_scalar_fold: (|k'|, negated)"""
    return (n - k, True) if n - k < k else (k, False)


def quad_digits(k, n):
    """the 64 digits sw_quad_mul walks (the top fix applied) and the sign of the fold"""
    mag, neg = fold(k, n)
    d, _, top = rec16(mag)
    if top:
        assert d[63] == -8
        d[63] = 8
    assert sum(x << (4 * w) for w, x in enumerate(d)) == mag
    return d, neg, top


# ---- the families ---------------------------------------------------------------------------------------------------------------
def fam_small(g):
    r = g.r
    out = [(str(v), v) for v in (0, 1, 2, 7, 8, 9, 15, 16, 17)]
    out += [("r-1", r - 1), ("r-2", r - 2), ("r-8", r - 8), ("r-9", r - 9), ("(r-1)/2", (r - 1) // 2), ("(r+1)/2", (r + 1) // 2)]
    if g.suite == "secp256r1":
        out += [("(n-3)/2", (r - 3) // 2), ("(n+3)/2", (r + 3) // 2)]
        for t, v in out:
            assert fold(v, r)[1] == (2 * v > r), t
        assert fold((r + 1) // 2, r) == ((r - 1) // 2, True) and fold((r - 1) // 2, r) == ((r - 1) // 2, False)
        assert fold(r - 1, r) == (1, True) and fold(0, r) == (0, False)
    assert all(0 <= v < r for _, v in out)
    return out


def fam_nib(g):
    r = g.r
    out = []
    pat = {"7": "77", "8": "88", "9": "99", "78": "78", "87": "87"}
    for name, p in pat.items():
        v = _below(int(p * 32, 16), r)
        d, car, top = rec16(v)
        lo = slice(0, 60)                        # _below clears bits of the top nibbles only (every r is above 2^248)
        assert [(v >> (4 * w)) & 15 for w in range(60)] == [int(p[1 - (w & 1)], 16) for w in range(60)], name
        if name == "7":
            assert d[lo] == [7] * 60 and not any(car[lo])
        elif name == "8":
            assert d[0] == -8 and d[1:60] == [-7] * 59 and all(car[1:60])
        elif name == "9":
            assert d[0] == -7 and d[1:60] == [-6] * 59 and all(car[1:60])
        else:
            assert d[lo].count(-8) >= 29, (name, d)          # the runs of -8: 7 + 8 + carry and 8 + 8
        out.append(("all-" + name, v))
    t = ((r - 1).bit_length() - 1) // 4          # the top window of a canonical scalar
    lo_v = (1 << (4 * t)) - int("8" * t, 16)     # 0x77..78: k + 0x88..8 reaches 16^t
    hi_v = r - 1 if rec16(r - 1)[1][t] else (((r - 1) >> (4 * t)) << (4 * t)) - 1
    assert 0 < lo_v < hi_v < r
    assert rec16(lo_v)[1][t] == 1 and rec16(lo_v - 1)[1][t] == 0 and rec16(hi_v)[1][t] == 1
    assert all(rec16(v)[1][t] == 0 for v in range(hi_v + 1, min(hi_v + 3, r)))
    out += [("carry-top-min", lo_v), ("carry-top-min-1", lo_v - 1), ("carry-top-max", hi_v)]
    return out


def fam_fold(g):
    """secp256r1 only: the branch `top && j == 3 && i == 15` of sw_quad_mul, from both sides of the fold"""
    n = g.r
    lo = (1 << 256) - int("8" * 64, 16)          # 0x77..78: the smallest value whose recoding carries out of nibble 63
    assert lo == int("7" * 63 + "8", 16) and lo <= (n - 1) // 2
    out = []
    for name, mag, takes in (("top-min", lo, 1), ("top-min-1", lo - 1, 0), ("top-max", (n - 1) // 2, 1)):
        assert rec16(mag)[2] == takes and fold(mag, n) == (mag, False) and fold(n - mag, n) == (mag, True)
        for t, k in ((name, mag), (name + ",n-k", n - mag)):
            d, neg, top = quad_digits(k, n)
            assert top == takes and neg == (k != mag) and (d[63] == 8) == bool(takes), t
            out.append((t, k))
    return out


def fam_stream(g):
    r = g.r
    n = r if g.suite == "secp256r1" else None
    dig = (lambda k: quad_digits(k, n)[0]) if n else (lambda k: rec16(k)[0])
    out = []
    for j in (1, 2, 3):
        b = 1 << (64 * j)
        d = dig(b)
        assert d[16 * j] == 1 and sum(map(abs, d)) == 1                     # three streams add the neutral entry in every window
        out.append(("2^%d" % (64 * j), b))
        d = dig(b - 1)
        assert d[0] == -1 and d[16 * j] == 1 and sum(map(abs, d)) == 2      # ... f recodes to 16 - 1 with a carry through every window
        out.append(("2^%d-1" % (64 * j), b - 1))
        d = dig(b + 8)
        assert d[0] == -8 and d[1] == 1 and d[16 * j] == 1
        out.append(("2^%d+8" % (64 * j), b + 8))
        d = dig(b - 8)
        assert d[0] == -8 and d[16 * j - 1] == 0 and d[16 * j] == 1 and all(x == 0 for x in d[1:16 * j])
        out.append(("2^%d-8" % (64 * j), b - 8))
        v = b - (8 << (64 * j - 4))                                          # 0x8 in the last nibble of stream j - 1: -8 there, +1 above
        d = dig(v)
        assert d[16 * j - 1] == -8 and d[16 * j] == 1 and sum(map(abs, d)) == 9
        out.append(("2^%d-8*16^%d" % (64 * j, 16 * j - 1), v))
    rng = random.Random("prove-cases stream %s" % g.suite)
    w = rng.randrange(1 << 56, min(r >> 192, 7 << 60))
    same = w * (1 + (1 << 64) + (1 << 128) + (1 << 192))
    d = dig(same)
    assert same < r and d[0:16] == d[16:32] == d[32:48] == d[48:64] and any(d[0:16])
    out.append(("four-equal", same))
    top_only = rng.randrange(1, r >> (193 if n else 192)) << 192               # secp256r1: below n/2, so that the fold keeps it
    d = dig(top_only)
    assert top_only < r and not any(d[0:48]) and any(d[48:64])
    out.append(("top-only", top_only))
    if n:
        assert all(fold(v, n) == (v, False) for _, v in out)
    return out


def fam_comb(g):
    r = g.r
    out = []
    for p in (0x7fff, 0x8000, 0xffff):
        v = _below(sum(p << (16 * w) for w in range(16)), r)
        d, car, _ = comb_digits(v, 16)
        assert [(v >> (16 * w)) & 0xffff for w in range(15)] == [p] * 15
        assert all(car[1:16]) if p >= 0x8000 else (not any(car) and d[:15] == [p] * 15)
        out.append(("every-row-%04x" % p, v))
        top = max(w for w in range(15) if (p << (16 * w)) < r)         # row 14: row 15 holds the carry of a chunk >= 0x8000
        assert top == 14
        for w in (0, top):
            v = p << (16 * w)
            d, car, _ = comb_digits(v, 16)
            assert [x != 0 for x in d].count(True) == (1 if p < 0x8000 else 2) and d[w] == (p if p < 0x8000 else p - 0x10000)
            assert p < 0x8000 or d[w + 1] == 1
            out.append(("row%d-%04x" % (w, p), v))
    for w in range(16):
        v = 1 << (16 * w)
        if v < r:
            d, _, _ = comb_digits(v, 16)
            assert d[w] == 1 and sum(map(abs, d)) == 1
            out.append(("2^%d" % (16 * w), v))
        if w:
            d, car, _ = comb_digits(v - 1, 16)
            assert d[0] == -1 and d[w] == 1 and sum(map(abs, d)) == 2 and all(car[1:w + 1])
            out.append(("2^%d-1" % (16 * w), v - 1))
    for p in (0x7f, 0x80, 0xff):
        v = _below(int("%02x" % p * 32, 16), r)
        d, car, _ = comb_digits(v, 8)
        assert [(v >> (8 * w)) & 255 for w in range(31)] == [p] * 31
        assert all(car[1:32]) if p >= 0x80 else (not any(car) and d[:31] == [p] * 31)
        out.append(("every-byte-%02x" % p, v))
    if g.suite == "secp256r1":
        edge = (1 << 256) - int("80" * 32, 16)
        assert rec8_p256(edge) == ([-128] * 32, 1) and rec8_p256(edge - 1) == ([127] * 32, 0) and edge < r
        out += [("row32", edge), ("row32-1", edge - 1), ("row32+1", edge + 1)]
    return out


def fam_glv(g):
    r, lam = g.r, None
    out, signs = [], set()
    n_max = 0
    for tag, k in glv_scalars():
        if tag.startswith("glv-max"):
            if n_max >= N_GLV_MAX:
                continue
            n_max += 1
        out.append((tag[4:], k))
        if tag == "glv-k1=0":
            lam = k
    assert n_max == N_GLV_MAX and lam is not None and glv_decompose(lam) == (0, 1)
    out += [("k1=0,%d*lam" % j, j * lam % r) for j in (2, 3, 5, -2)]
    for tag, k in out:
        k1, k2 = glv_decompose(k)
        if tag.startswith("k1=0"):
            assert k1 == 0 and k2 != 0 and abs(k2) <= 5, tag
        if tag.startswith("k2=0"):
            assert k2 == 0 and k1 == k, tag
        if tag.startswith("sign"):
            assert k1 and k2
            signs.add((k1 < 0, k2 < 0))
    assert len(signs) == 4
    return out


def fam_range(g):
    r = g.r
    out = [("r", r), ("r+1", r + 1), ("2^253", 1 << 253), ("2^255", 1 << 255), ("2^256-1", (1 << 256) - 1)]
    assert sum(v >= r for _, v in out) == (3 if g.suite == "secp256r1" else 5)
    return out


def fam_rand(g):
    rng = random.Random("prove-cases rand %s" % g.suite)
    return [("%03d" % i, rng.randrange(1, g.r)) for i in range(N_RANDOM)]


def families(g):
    fams = {"small": fam_small(g), "nib": fam_nib(g), "stream": fam_stream(g), "comb": fam_comb(g), "range": fam_range(g),
            "rand": fam_rand(g)}
    if g.suite == "secp256r1":
        fams["fold"] = fam_fold(g)
    if g.glv:
        fams["glv"] = fam_glv(g)
    for name, members in fams.items():
        assert members, "family %s of %s is empty" % (name, g.suite)
    return fams


# ---- the cases --------------------------------------------------------------------------------------------------------------------
def _neutral_encodings(g):
    if g.suite == "secp256r1":
        return [bytes(33)]                                                     # Sec1 has no 33-byte string for it: refused
    if g.suite == "bandersnatch_sw":
        return [bo.point_encode(None), (7).to_bytes(32, "little") + bytes([bo.FLAG_INF | 1])]      # x and the low flag bits are not read
    e = g.enc_in(g.identity)
    return [e, e[:31] + bytes([e[31] | 0x80])]                                 # (0, 1), and the same with the sign bit of x = 0 set


def _input_items(g, fams):
    """[(tag, sk, kind, h or wire bytes)] of the given-input crossing"""
    r = g.r
    rng = random.Random("prove-cases inputs %s" % g.suite)
    nib8 = dict(fams["nib"])["all-8"]
    secrets = [("1", 1), ("2", 2), ("r-1", r - 1), ("(r+1)/2", (r + 1) // 2), ("all-8", nib8), ("rand", rng.randrange(1, r)), ("0", 0)]
    hs = [rng.randrange(1, r) for _ in range(2)]
    und = g.undecodable()
    off = g.off_subgroup(g.gmul(hs[0])) if g.cofactor > 1 else None
    out = []
    for st, sk in secrets:
        t = "sk=%s," % st
        out += [(t + "H=G", sk, "log", 1), (t + "H=-G", sk, "log", r - 1), (t + "H=2G", sk, "log", 2), (t + "H=B", sk, "B", None)]
        out += [(t + "H=h%d*G" % i, sk, "log", h) for i, h in enumerate(hs)]
        if sk:
            out.append((t + "H=pk", sk, "log", sk))
        out += [(t + "H=O/%d" % i, sk, "neutral", e) for i, e in enumerate(_neutral_encodings(g))]
        out.append((t + "H=undecodable", sk, "raw", und))
        if off is not None:
            out.append((t + "H=off-subgroup", sk, "raw", off))
    return out


def _oracle(suite, pedersen, sk, ad, inputs=None, msgs=None):
    """the C oracle's prover, configured like the test contexts (its process-global suite is put back)"""
    g = group(suite)
    kw = dict(inputs=inputs, msgs=msgs, ad=ad, threads=THREADS)
    if suite == "secp256r1":
        co.p256_set_blinding_base(so.default_blinding_base())
        return (co.p256_pedersen_prove_batch if pedersen else co.p256_ietf_prove_batch)(sk, **kw)
    if suite == "bandersnatch_sw":
        return (co.bsw_pedersen_prove_batch if pedersen else co.bsw_ietf_prove_batch)(sk, **kw)
    co.set_check_mask(15)
    if suite != "bandersnatch":
        S = g.S
        xy = lambda p: p[0].to_bytes(32, "little") + p[1].to_bytes(32, "little")
        co.set_suite_desc(CURVE_ID[suite], S.suite_id, S.h2c_dst, xy((S.gx, S.gy)), xy((S.bx, S.by)), challenge_len=DEFAULT_L[suite])
    else:
        co.set_suite(1)
    try:
        return (co.pedersen_prove_batch if pedersen else co.ietf_prove_batch)(sk, **kw)
    finally:
        co.set_suite(1)


def _zero_refused(res, keys):
    """the oracle leaves a refused item's outputs unwritten: zero bytes are what the library must give"""
    bad = res["status"] != 0
    for k in keys:
        res[k] = res[k].copy()
        res[k][bad] = 0
    return res


class Cases:
    """Arrays of one suite's set; row i is case tags[i] (family before ':').  ietf[a] / ped[a]: the C oracle's proofs under
    ADS[a], refused rows zeroed; pk_int / gamma_int: the integer-arithmetic values of the accepted rows; pk_com_int: sk*G + b*B
    from the oracle's b under ADS[1]; *_msg: the secrets-only rows (secret_rows) proven from msgs under ADS[1]."""

    def family_counts(self):
        out = {}
        for t in self.tags:
            for name in t.split(" | "):                      # a value two families name counts in both
                out[name.split(":")[0]] = out.get(name.split(":")[0], 0) + 1
        return out

    def describe(self):
        return "%s: %d cases (%s), %d refused" % (self.suite, self.n, ", ".join("%s %d" % kv for kv in sorted(self.family_counts().items())),
                                                 int((self.status != 0).sum()))


def _build(suite):
    g = group(suite)
    r = g.r
    fams = families(g)
    Bb = blinding(suite)
    rng = random.Random("prove-cases h %s" % suite)
    # the secrets, each value once (a value two families name keeps both names), with H = h*G for a random h
    by_value, order = {}, []
    for fam, members in fams.items():
        for tag, v in members:
            if v not in by_value:
                by_value[v] = []
                order.append(v)
            by_value[v].append("%s:%s" % (fam, tag))
    items = [(" | ".join(by_value[v]), v, "log", rng.randrange(1, r)) for v in order]
    n_secret = len(items)
    items += [("input:" + t, sk, kind, x) for t, sk, kind, x in _input_items(g, fams)]
    while len(items) % 2 == 0:                                 # an odd count: a part-full last lane at K = 2, 4 and 8
        items.append(("rand:extra%d" % len(items), rng.randrange(1, r), "log", rng.randrange(1, r)))
    assert len(items) < MAX_CASES and len({t for t, *_ in items}) == len(items)
    n = len(items)

    cs = Cases()
    cs.suite, cs.n, cs.n_secret = suite, n, n_secret
    cs.tags = [t for t, *_ in items]
    cs.sk_int = [sk for _, sk, _, _ in items]
    cs.kinds = [k for _, _, k, _ in items]
    arr = lambda xs, w: np.frombuffer(b"".join(xs), np.uint8).reshape(len(xs), w).copy()
    cs.sk = arr([g.scalar(sk) for sk in cs.sk_int], 32)
    H_pts, wires = [], []
    for _, sk, kind, x in items:
        if kind == "log":
            H_pts.append(g.gmul(x))
            wires.append(g.enc_in(H_pts[-1]))
        elif kind == "B":
            H_pts.append(Bb.B)
            wires.append(g.enc_in(Bb.B))
        else:
            H_pts.append(g.identity if kind == "neutral" else "none")
            wires.append(x)
    cs.inputs = arr(wires, g.pt_bytes)

    # the C oracle: both schemes under the three ad
    cs.ietf = [_zero_refused(_oracle(suite, False, cs.sk, ad, inputs=cs.inputs), IETF_KEYS[:4]) for ad in ADS]
    cs.ped = [_zero_refused(_oracle(suite, True, cs.sk, ad, inputs=cs.inputs), PED_KEYS[:7]) for ad in ADS]
    cs.status = cs.ietf[0]["status"].copy()
    assert all((x["status"] == cs.status).all() for x in cs.ietf + cs.ped)
    assert set(np.unique(cs.status)) <= {0, 2}
    cs.accepted = np.flatnonzero(cs.status == 0)
    cs.refused = np.flatnonzero(cs.status != 0)
    # the statuses the integers predict: refused exactly for sk >= r and for the strings that are no point of the subgroup
    for i, (tag, sk, kind, x) in enumerate(items):
        if kind in ("log", "B"):
            assert (cs.status[i] == 2) == (sk >= r), (suite, tag)
        elif kind == "raw":
            assert cs.status[i] == 2, (suite, tag)
        elif sk >= r:
            assert cs.status[i] == 2, (suite, tag)
    assert len(cs.refused) >= 3 and any(cs.kinds[i] == "neutral" for i in (cs.accepted if g.identity_on_wire else cs.refused))

    # pk and Gamma by integer arithmetic
    z = bytes(g.pt_bytes)
    pk_int, gamma_int = [], []
    for i, (tag, sk, kind, x) in enumerate(items):
        if cs.status[i]:
            pk_int.append(z)
            gamma_int.append(z)
            continue
        pk_int.append(g.enc_out(g.gmul(sk)))
        if kind == "log":
            gamma_int.append(g.enc_out(g.gmul(sk * x)))
        elif kind == "B":
            gamma_int.append(g.enc_out(Bb.mul(sk)))
        else:
            gamma_int.append(g.enc_out(g.identity))
    cs.pk_int, cs.gamma_int = arr(pk_int, g.pt_bytes), arr(gamma_int, g.pt_bytes)
    # ... literally, on a slice: sk*G and sk*H by the oracle's double-and-add
    cand = [i for i in cs.accepted if cs.kinds[i] == "log"]
    picked = cand[::max(1, len(cand) // N_LITERAL)]
    assert len(picked) >= N_LITERAL
    for i in picked:
        sk, h = cs.sk_int[i], items[i][3]
        assert g.mul(sk, g.G) == g.gmul(sk) and g.mul(sk, H_pts[i]) == g.gmul(sk * h), (suite, cs.tags[i])
    cs.n_literal = len(picked)
    # pk_com = sk*G + b*B from the oracle's b (ADS[1])
    big = "big" if g.big_endian else "little"
    pc = []
    for i in range(n):
        if cs.status[i]:
            pc.append(z)
        else:
            b = int.from_bytes(cs.ped[1]["blinding"][i].tobytes(), big)
            pc.append(g.enc_out(g.add(g.gmul(cs.sk_int[i]), Bb.mul(b))))
    cs.pk_com_int = arr(pc, g.pt_bytes)

    # what the C oracle's verifier says to the accepted rows' proofs: 0, but for sk = 0 on secp256r1, whose pk (and Gamma) is the
    # point at infinity and has no Sec1 string (33 zero bytes stand for it, and no verifier decodes them): 2
    no_wire = np.array([suite == "secp256r1" and cs.sk_int[i] == 0 for i in cs.accepted])
    cs.round_trip = np.where(no_wire, 2, 0).astype(np.uint8)
    for a, ad in enumerate(ADS):
        assert (verify_with_oracle(suite, False, cs.ietf[a], ad, cs.accepted) == cs.round_trip).all(), (suite, a)
        assert (verify_with_oracle(suite, True, cs.ped[a], ad, cs.accepted)[~no_wire] == 0).all(), (suite, a)
    cs.round_trip_ped = verify_with_oracle(suite, True, cs.ped[1], ADS[1], cs.accepted)      # pk_com = b*B of sk = 0 is finite

    # the secrets-only part from messages
    cs.secret_rows = np.arange(n_secret)
    cs.msgs = arr([("prove-cases %-8s%04d" % (suite[:8], i)).encode()[:MSG_LEN].ljust(MSG_LEN, b".") for i in range(n_secret)], MSG_LEN)
    sks = cs.sk[:n_secret]
    cs.ietf_msg = _zero_refused(_oracle(suite, False, sks, ADS[1], msgs=cs.msgs), IETF_KEYS[:4])
    cs.ped_msg = _zero_refused(_oracle(suite, True, sks, ADS[1], msgs=cs.msgs), PED_KEYS[:7])
    assert (cs.ietf_msg["status"] == cs.status[:n_secret]).all() and (cs.ped_msg["status"] == cs.status[:n_secret]).all()
    return cs


@lru_cache(maxsize=None)
def cases(suite):
    """The whole set of one suite: the secrets (each with a random H = h*G) first, then the given-input crossing."""
    return _build(suite)


def compare(cs, got, want, keys, rows=None, what=""):
    """A prover's result dict against the expectations `want`, byte for byte, status included; rows: which row of `want` (and
    which case) each item of `got` is.  `input` is compared on the accepted rows (module docstring).  Prints one line, fails
    with the first differing cases."""
    rows = np.arange(len(got["status"])) if rows is None else np.asarray(rows)
    sel = lambda a: a[rows]
    wst = sel(want["status"])
    bad = {}
    for k in tuple(keys) + ("status",):
        g_, w_ = np.asarray(got[k]), sel(want[k])
        assert g_.shape == w_.shape, (what, k, g_.shape, w_.shape)
        diff = (g_ != w_) if g_.ndim == 1 else (g_ != w_).any(axis=1)
        if k == "input":
            diff &= wst == 0
        for i in np.flatnonzero(diff):
            bad.setdefault(int(i), []).append(k)
    print("%s %s: %d items, %d refused, %d differ" % (cs.suite, what, len(rows), int((wst != 0).sum()), len(bad)))
    assert not bad, "%s %s: %d items differ, first (case, fields): %s" % (
        cs.suite, what, len(bad), [(cs.tags[rows[i]], f) for i, f in sorted(bad.items())[:8]])


def verify_with_oracle(suite, pedersen, res, ad, rows):
    """the C oracle's verifier on the proofs `res` (a prover's result dict) of the given rows"""
    kw = dict(ad=ad, threads=THREADS)
    a = lambda k: res[k][rows]
    if pedersen:
        args = [a(k) for k in ("input", "output", "pk_com", "r", "ok", "s", "sb")]
        fn = {"secp256r1": co.p256_pedersen_verify_batch, "bandersnatch_sw": co.bsw_pedersen_verify_batch}.get(suite, co.pedersen_verify_batch)
    else:
        args = [a(k) for k in ("pk", "input", "output", "c", "s")]
        fn = {"secp256r1": co.p256_ietf_verify_batch, "bandersnatch_sw": co.bsw_ietf_verify_batch}.get(suite, co.ietf_verify_batch)
    if suite == "secp256r1":
        co.p256_set_blinding_base(so.default_blinding_base())
        return fn(*args, **kw)
    if suite == "bandersnatch_sw":
        return fn(*args, **kw)
    g = group(suite)
    co.set_check_mask(15)
    if suite != "bandersnatch":
        S = g.S
        xy = lambda p: p[0].to_bytes(32, "little") + p[1].to_bytes(32, "little")
        co.set_suite_desc(CURVE_ID[suite], S.suite_id, S.h2c_dst, xy((S.gx, S.gy)), xy((S.bx, S.by)), challenge_len=DEFAULT_L[suite])
    try:
        return fn(*args, **kw)
    finally:
        co.set_suite(1)
