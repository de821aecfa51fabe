"""Case generator for per-proof Pedersen verification with the challenge supplied (vrfhip_test_pedersen_verify_c on the device,
h*_pedersen_verify_c / hp_ped_verify_c in the host simulation).  A plain module, shared by tests/test_gpu_pedersen_c.py and
tests/test_hostsim_pedersen_c.py; it imports only the oracles and verify_uv_cases.  Nothing here calls the library.

The verifier accepts iff  s*H - c*Gamma == Ok  and  s*G + sb*B - c*pk_com == R.  Its real c is a hash of the five points, so an
accepting item at a chosen (c, s, sb) exists only where c is given.  Every point here has a known representation over (G, B):
H = h*G, Gamma = o*G, pk_com = y*G + yb*B (yb = 0 except where pk_com is B itself), and an accepting row has
Ok = (s*h - c*o)*G and R = (s - c*y)*G + (sb - c*yb)*B.  A row carries the representation of the Ok and R it puts on the wire, so
its expected status -- 0 where both equations hold, 1 where one fails -- follows from integers mod r alone (B's logarithm
to the base G is unknown to everyone, so (a, b) -> a*G + b*B is taken to be injective).  On a slice of every set both equations
are also evaluated literally, with the oracle's double-and-add on the points of the row, and the two ways must agree.

Row families (the issue text lists them): the response scalars of verify_uv_cases as s, as sb and as both (the 16-bit chunk
patterns 0x7fff / 0x8000 / 0xffff / 0x8001 through the generator's comb and the blinding base's, r - 1, r - 2, the nibble
patterns, on secp256r1 the nibble-63 / byte-31 carries), its challenge scalars, the GLV scalars as s and as c, points that meet
themselves (pk_com = G, -G, B; H = G; Gamma = +-H; a neutral pk_com or Gamma where the codec can carry one), neutral results
and neutral partial sums, random rows; one rejecting twin per accepting row (six disturbances in turn); rows the decode stage or
the range checks must refuse (status 2); and 32 genuine proofs of the C oracle with their recomputed challenge, and with
that challenge's low bit flipped.

secp256r1: Sec1 has no 33-byte string for the point at infinity, so the rows whose Ok or R is neutral cannot be put on the
wire and are left out on that suite: "Ok=O", "R=O,sb=0", and "c=s=sb=0", which is both at once.  Nothing else is left out,
and _rows asserts that no other row is dropped.  The row with a neutral partial sum (s = c*y, sb != 0) is kept on every suite.

cases(suite, L) -> Cases: wire arrays input, output, pk_com, r, ok, c, s, sb (and x || y forms), expected status."""
import dataclasses
import os
import random
import sys
from functools import lru_cache

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import bsw_oracle as bo, c_oracle as co, sw_oracle as so, vrf_oracle as vo  # noqa: E402
from verify_uv_cases import DEFAULT_L, EXTRA_L, SUITES, challenge_values, glv_scalars, group, response_values  # noqa: E402,F401

N_RANDOM = 64
N_LITERAL = 32
N_TIE = 32
MAX_ROWS = 1600
DISTURBANCES = ("ok+G", "r+G", "r+B", "s+-1", "sb+-1", "c^1")
CURVE_ID = {"bandersnatch": 1, "jubjub": 2, "ed25519": 3, "baby_jubjub": 4}


class Base:
    """k*B by the oracle's additions over a 4-bit window table of j * 16^w * B (the kind Group._gmul_windows keeps for G)"""

    def __init__(self, g, B):
        self.g, self.B, self._win, self._memo = g, B, [], {}
        base = B
        for _ in range(64):
            row = [g.identity, base]
            for _ in range(14):
                row.append(g.add(row[-1], base))
            self._win.append(row)
            base = g.add(row[15], base)

    def mul(self, k):
        k %= self.g.r
        if k not in self._memo:
            acc = self.g.identity
            for w in range(64):
                d = (k >> (4 * w)) & 15
                if d:
                    acc = self.g.add(acc, self._win[w][d])
            self._memo[k] = acc
        return self._memo[k]


@lru_cache(maxsize=None)
def blinding(suite):
    """the blinding base a test context of the suite has: Bandersnatch's pinned one, the oracles' copy of the test base elsewhere"""
    g = group(suite)
    if suite == "secp256r1":
        B = so.default_blinding_base()
    elif suite == "bandersnatch_sw":
        B = bo.BLINDING_BASE
    else:
        B = (g.S.bx, g.S.by)
    return Base(g, B)


@dataclasses.dataclass
class Row:
    tag: str
    family: str
    kind: str              # "accept", one of DISTURBANCES, "invalid", "tie", "tie-c^1"
    wire: tuple            # H, Gamma, pk_com, R, Ok as wire bytes
    c: int
    s: int
    sb: int
    status: int
    pts: tuple = None      # the five points, for the literal check and the x || y forms (None: a row without them)


def _status(r, y, yb, h, o, c, s, sb, ok_d, r_ab):
    """0 where both equations hold for an Ok = ok_d*G and an R = r_ab[0]*G + r_ab[1]*B, else 1"""
    e1 = (s * h - c * o - ok_d) % r == 0
    e2 = (s - c * y - r_ab[0]) % r == 0 and (sb - c * yb - r_ab[1]) % r == 0
    return 0 if e1 and e2 else 1


def _items(g, L):
    """[(family, tag, y, yb, h, o, c, s, sb)] of the accepting rows"""
    r = g.r
    rng = random.Random("pedersen-c %s %d" % (g.suite, L))
    top = 1 << (8 * L)
    rs = lambda: rng.randrange(1, r)
    rc = lambda: rng.randrange(1, min(top, r))
    y0, h0, o0, c0, s0, sb0 = rs(), rs(), rs(), rc(), rs(), rs()
    it = []
    for t, v in response_values(g):
        it.append(("s-edge", t, y0, 0, h0, o0, c0, v, rs()))
        it.append(("sb-edge", "sb" + t[1:], y0, 0, h0, o0, c0, rs(), v))
        it.append(("s+sb-edge", "s,sb" + t[1:], y0, 0, h0, o0, c0, v, v))
    for t, v in challenge_values(g, L):
        it.append(("c-edge", t, y0, 0, h0, o0, v, s0, sb0))
    if g.glv:
        for t, k in glv_scalars():
            it.append(("glv", t + "-as-s", y0, 0, h0, o0, c0, k, sb0))
            if k < top:
                it.append(("glv", t + "-as-c", y0, 0, h0, o0, k, s0, sb0))
    c1, s1, sb1 = rc(), rs(), rs()
    it += [("self", "y=1", 1, 0, h0, o0, c1, s1, sb1), ("self", "y=r-1", r - 1, 0, h0, o0, c1, s1, sb1),
           ("self", "h=1", y0, 0, 1, o0, c1, s1, sb1), ("self", "o=h", y0, 0, h0, h0, c1, s1, sb1),
           ("self", "o=-h", y0, 0, h0, r - h0, c1, s1, sb1), ("self", "pk_com=B", 0, 1, h0, o0, c1, s1, sb1)]
    if g.identity_on_wire:
        it += [("self", "pk_com=O", 0, 0, h0, o0, c1, s1, sb1), ("self", "Gamma=O", y0, 0, h0, 0, c1, s1, sb1)]
    inv_h = pow(h0, -1, r)
    c2 = rc()
    if g.identity_on_wire:            # secp256r1: no wire form of a neutral Ok or R (module docstring)
        it += [("neutral", "Ok=O", y0, 0, h0, o0, c2, c2 * o0 * inv_h % r, sb1),
               ("neutral", "R=O,sb=0", y0, 0, h0, o0, c2, c2 * y0 % r, 0)]
    it += [("neutral", "s=c*y,sb!=0", y0, 0, h0, o0, c2, c2 * y0 % r, sb1)]
    if g.identity_on_wire:
        it += [("neutral", "c=s=sb=0", y0, 0, h0, o0, 0, 0, 0)]
    it += [("rand", "rand%03d" % i, rs(), 0, rs(), rs(), rc(), rs(), rs()) for i in range(N_RANDOM)]
    return it


def _rows(g, L):
    r, Bb = g.r, blinding(g.suite)
    rows = []
    lin = lambda a, b: g.add(g.gmul(a), Bb.mul(b))
    n_acc = 0
    for fam, tag, y, yb, h, o, c, s, sb in _items(g, L):
        H, Gm, pk = g.gmul(h), g.gmul(o), lin(y, yb)
        ok_d, r_ab = (s * h - c * o) % r, ((s - c * y) % r, (sb - c * yb) % r)
        Ok, R = g.gmul(ok_d), lin(*r_ab)
        assert g.identity_on_wire or (Ok is not None and R is not None), (g.suite, tag)      # no row is dropped here
        assert _status(r, y, yb, h, o, c, s, sb, ok_d, r_ab) == 0
        wire = tuple(g.enc_in(p) for p in (H, Gm, pk, R, Ok))
        rows.append(Row(tag, fam, "accept", wire, c, s, sb, 0, (H, Gm, pk, R, Ok)))
        # the rejecting twin: one disturbance, in turn
        kind = DISTURBANCES[n_acc % len(DISTURBANCES)]
        n_acc += 1
        c_, s_, sb_, ok_, rab_ = c, s, sb, ok_d, r_ab
        if kind == "ok+G":
            ok_ = (ok_d + 1) % r
        elif kind == "r+G":
            rab_ = ((r_ab[0] + 1) % r, r_ab[1])
        elif kind == "r+B":
            rab_ = (r_ab[0], (r_ab[1] + 1) % r)
        elif kind == "s+-1":
            s_ = s + 1 if s + 1 < r else s - 1
        elif kind == "sb+-1":
            sb_ = sb + 1 if sb + 1 < r else sb - 1
        else:
            c_ = c ^ 1
        Ok_, R_ = g.gmul(ok_), lin(*rab_)
        assert g.identity_on_wire or (Ok_ is not None and R_ is not None), (g.suite, tag, kind)
        st = _status(r, y, yb, h, o, c_, s_, sb_, ok_, rab_)
        assert st == 1, (g.suite, tag, kind)
        wire_ = tuple(g.enc_in(p) for p in (H, Gm, pk, R_, Ok_))
        rows.append(Row(tag + "/" + kind, fam, kind, wire_, c_, s_, sb_, 1, (H, Gm, pk, R_, Ok_)))
    # invalid rows: status 2
    rng = random.Random("pedersen-c invalid %s %d" % (g.suite, L))
    y, h, o, s, sb = (rng.randrange(1, r) for _ in range(5))
    c = rng.randrange(1, min(1 << (8 * L), r))
    H, Gm, pk, Ok, R = g.gmul(h), g.gmul(o), g.gmul(y), g.gmul(s * h - c * o), lin(s - c * y, sb)
    good = tuple(g.enc_in(p) for p in (H, Gm, pk, R, Ok))
    bad = lambda tag, wire=good, c=c, s=s, sb=sb: rows.append(Row("bad:" + tag, "invalid", "invalid", wire, c, s, sb, 2))
    bad("s=r", s=r)
    bad("sb=r", sb=r)
    if L < 32:
        bad("c=2^8L", c=1 << (8 * L))
    bad("R", wire=good[:3] + (g.undecodable(), good[4]))
    if g.cofactor > 1:
        bad("Ok-cofactor", wire=good[:4] + (g.off_subgroup(Ok),))
    return rows


# ---- genuine proofs: the supplied c against the production hash -----------------------------------------------------------
def _tie_rows(g, L):
    """N_TIE proofs of the C oracle (ad = b""), their challenge recomputed by the Python oracle's challenge function -> status 0;
    the same with the challenge's low bit flipped -> status 1"""
    suite, r = g.suite, g.r
    rng = random.Random("pedersen-c tie %s %d" % (suite, L))
    big = "big" if g.big_endian else "little"
    sk = np.frombuffer(b"".join(rng.randrange(1, r).to_bytes(32, big) for _ in range(N_TIE)), np.uint8).reshape(N_TIE, 32)
    msgs = np.frombuffer(bytes(rng.randrange(256) for _ in range(16 * N_TIE)), np.uint8).reshape(N_TIE, 16)
    if suite == "secp256r1":
        co.p256_set_blinding_base(so.default_blinding_base())
        pr = co.p256_pedersen_prove_batch(sk, msgs=msgs, ad=b"")
        dec = so.point_decode
        chal = lambda pts: so.challenge(pts, b"", challenge_len=L)
    elif suite == "bandersnatch_sw":
        assert L == bo.CHALLENGE_LEN
        pr = co.bsw_pedersen_prove_batch(sk, msgs=msgs, ad=b"")
        dec = lambda b: bo.point_decode(b)[1]
        chal = lambda pts: bo.challenge(pts, b"")
    else:
        S = dataclasses.replace(g.S, challenge_len=L)
        xy = lambda p: p[0].to_bytes(32, "little") + p[1].to_bytes(32, "little")
        co.set_suite_desc(CURVE_ID[suite], S.suite_id, S.h2c_dst, xy((S.gx, S.gy)), xy((S.bx, S.by)), challenge_len=L)
        try:
            pr = co.pedersen_prove_batch(sk, msgs=msgs, ad=b"")
        finally:
            co.set_suite(1)
        dec = lambda b: vo.point_decode(S, b)
        chal = lambda pts: vo.challenge_rfc9381(S, pts, b"")
    assert not pr["status"].any()
    rows = []
    for i in range(N_TIE):
        wire = tuple(pr[k][i].tobytes() for k in ("input", "output", "pk_com", "r", "ok"))
        H, Gm, pk, R, Ok = (dec(b) for b in wire)
        c = chal([pk, H, Gm, R, Ok])
        assert c < (1 << (8 * L))
        s, sb = (int.from_bytes(pr[k][i].tobytes(), big) for k in ("s", "sb"))
        rows.append(Row("tie%02d" % i, "tie", "tie", wire, c, s, sb, 0, (H, Gm, pk, R, Ok)))
        rows.append(Row("tie%02d/c^1" % i, "tie", "tie-c^1", wire, c ^ 1, s, sb, 1, (H, Gm, pk, R, Ok)))
    return rows


# ---- the literal check --------------------------------------------------------------------------------------------------------
def _check_literal(g, rows):
    """Both equations as the verifier states them, by the oracle's own double-and-add on the row's points, against the status the
    integers gave: at least N_LITERAL rows, one of every family and of every kind among them"""
    B = blinding(g.suite).B
    cand = [i for i, rw in enumerate(rows) if rw.pts is not None]
    picked, seen = [], set()
    for i in cand:
        for key in (("f", rows[i].family), ("k", rows[i].kind)):
            if key not in seen:
                seen.add(key)
                picked.append(i)
    assert {k for t, k in seen if t == "k"} >= set(DISTURBANCES) | {"accept", "tie", "tie-c^1"}
    assert {f for t, f in seen if t == "f"} >= {rw.family for rw in rows if rw.pts is not None}
    step = max(1, len(cand) // N_LITERAL)
    picked = sorted(set(picked) | set(cand[::step]))
    assert len(picked) >= N_LITERAL
    for i in picked:
        rw = rows[i]
        H, Gm, pk, R, Ok = rw.pts
        c = rw.c % g.r
        e1 = g.add(g.mul(rw.s, H), g.neg(g.mul(c, Gm))) == Ok
        e2 = g.add(g.add(g.mul(rw.s, g.G), g.mul(rw.sb, B)), g.neg(g.mul(c, pk))) == R
        assert (0 if e1 and e2 else 1) == rw.status, (g.suite, rw.tag, e1, e2)
    return len(picked)


class Cases:
    """Arrays of one (suite, L) set; row i is case tags[i] of kind kinds[i].  status: what the verifier must answer."""

    def __init__(self, g, L, rows, n_literal):
        self.suite, self.L, self.n, self.n_literal = g.suite, L, len(rows), n_literal
        self.tags, self.kinds, self.families = [rw.tag for rw in rows], [rw.kind for rw in rows], [rw.family for rw in rows]
        pw = g.pt_bytes
        arr = lambda xs, w: np.frombuffer(b"".join(xs), np.uint8).reshape(len(xs), w).copy()
        self.input, self.output, self.pk_com, self.r, self.ok = (arr([rw.wire[k] for rw in rows], pw) for k in range(5))
        sc = lambda v: int(v).to_bytes(32, "big" if g.big_endian else "little")
        self.c, self.s, self.sb = (arr([sc(getattr(rw, k)) for rw in rows], 32) for k in ("c", "s", "sb"))
        self.c_int, self.s_int, self.sb_int = ([getattr(rw, k) for rw in rows] for k in ("c", "s", "sb"))
        self.status = np.array([rw.status for rw in rows], np.uint8)
        # x || y forms of the rows whose five points have affine coordinates
        xys = [None if rw.pts is None else [g.xy(p) for p in rw.pts] for rw in rows]
        self.xy_rows = np.array([i for i, x in enumerate(xys) if x is not None and all(v is not None for v in x)], np.int64)
        self.input_xy, self.output_xy, self.pk_com_xy, self.r_xy, self.ok_xy = (
            arr([xys[i][k] for i in self.xy_rows], 64) for k in range(5))

    def points(self, rows=None, xy=False):
        """the five point arrays in the order of the entry point's arguments"""
        a = (self.input_xy, self.output_xy, self.pk_com_xy, self.r_xy, self.ok_xy) if xy else (
            self.input, self.output, self.pk_com, self.r, self.ok)
        return a if rows is None else tuple(x[rows] for x in a)


@lru_cache(maxsize=None)
def cases(suite, L=None):
    """The whole set of one suite at challenge length L (default: the suite's own): accepting rows each followed by its rejecting
    twin, the invalid rows, the genuine proofs."""
    g = group(suite)
    L = DEFAULT_L[suite] if L is None else L
    rows = _rows(g, L) + _tie_rows(g, L)
    assert len(rows) < MAX_ROWS
    assert all(rw.s <= g.r and rw.sb <= g.r and rw.c <= (1 << (8 * L)) for rw in rows)
    n_literal = _check_literal(g, rows)
    return Cases(g, L, rows, n_literal)
