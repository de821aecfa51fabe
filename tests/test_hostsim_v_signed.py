"""CPU: the V half of the GLV suite's IETF verifier -- eight signed affine table entries, walked over a sign-aligned recoding,
normalised by an inversion that rides on pk's inverse root -- compiled for the host (tests/hostsim_vsigned), piece by piece
against Python integers:

- the recoding alone (fr.cuh glv_recode_sac): every half re-sums from its 128 digits; half 0 is walked as half 0 | 1;
- the table and the walk (build_joint_va_table, joint_va_normalise, joint_va_ladder): the entries and V against integer
  arithmetic on the curve, with sums that reach the neutral element, neutral bases and Gamma = psi(H);
- the ride (decode_by_inv_root_ride): x, the verdict and 1 / P;
- the entries as each decode form of the kernels leaves them.

This pins logic, not code generation: the device test is tests/test_gpu_v_signed.py."""
import ctypes
import os
import random
import subprocess

import pytest

import verify_uv_cases as vc
from oracle import vrf_oracle as vo

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim_vsigned")
S = vo.BANDERSNATCH
R, Q = S.r, S.q
LAM = vc._GLV["lam"]
ID = vo.te_identity()


@pytest.fixture(scope="module")
def hv():
    subprocess.run(["make", "-C", HERE, "libhostsim_vsigned.so"], check=True, stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(os.path.join(HERE, "libhostsim_vsigned.so"))
    for f in (lib.hvs_recode, lib.hvs_ride, lib.hvs_decode_entries):
        f.restype = ctypes.c_uint32
    lib.hvs_v.restype = None
    return lib


def scalar_pairs():
    """(c, s) as the wire carries them: zeros, equal, r - 1, at and above r, and 256 seeded random pairs"""
    rng = random.Random(0x5AC)
    top = (1 << 256) - 1
    pairs = [(0, 0), (0, 1), (1, 0), (0, R - 1), (R - 1, 0), (7, 7), (R - 1, R - 1), (R, 5), (R + 1, R - 1), (top, R - 2),
             (5, R), (5, R + 1), (R - 1, top), (2, 1), (1, 2), (LAM, LAM), (R - LAM, 12345)]
    pairs += [(k, k2) for (_, k), (_, k2) in zip(vc.glv_scalars()[:8], vc.glv_scalars()[8:16])]
    pairs += [(rng.randrange(R), rng.randrange(R)) for _ in range(256)]
    return pairs


def reduced(c, s):
    """what load_cs_reduced leaves: c mod r and s, or zeros for a non-canonical s"""
    return (0, 0) if s >= R else (c % R, s)


def _sgn(k):
    return -1 if k < 0 else 1            # a zero half counts as positive, as glv_finish reports it


def recode(hv, mags):
    sgn, u = ctypes.create_string_buffer(16), ctypes.create_string_buffer(48)
    fix = hv.hvs_recode(b"".join(m.to_bytes(16, "little") for m in mags), sgn, u)
    assert fix in (0, 1), "sac_index / sac_neg disagree with the recoded words"
    return int.from_bytes(sgn.raw, "little"), [int.from_bytes(u.raw[16 * j:16 * j + 16], "little") for j in range(3)], fix


def check_recoding(hv, mags):
    sgn, u, fix = recode(hv, mags)
    d = [-1 if (sgn >> i) & 1 else 1 for i in range(128)]
    assert d[127] == 1, mags
    assert fix == (1 - (mags[0] & 1)), mags
    assert sum(d[i] << i for i in range(128)) == mags[0] + fix, mags
    for j in range(3):
        assert sum(((u[j] >> i) & 1) * d[i] << i for i in range(128)) == mags[j + 1], (j, mags)


def test_recoding_resums_every_half(hv):
    edge = [0, 1, 2, 1 << 126, (1 << 127) - 1]
    for m0 in edge:                                   # even and odd half 0, all four equal among them
        for m1 in edge:
            for m2 in edge:
                for m3 in edge:
                    check_recoding(hv, [m0, m1, m2, m3])
    rng = random.Random(0x5AC0)
    for _ in range(64):
        check_recoding(hv, [rng.randrange(1 << 127) for _ in range(4)])
    for c, s in scalar_pairs():
        c, s = reduced(c, s)
        check_recoding(hv, [abs(k) for k in vc.glv_decompose(c) + vc.glv_decompose(s)])


def _xy(p):
    return p[0].to_bytes(32, "little") + p[1].to_bytes(32, "little")


def expected_entries(g, h, gam, c, s):
    """the 8 entries Q0 + u1 Q1 + u2 Q2 + u3 Q3 as x || y || d x y, for H = h*G, Gamma = gam*G"""
    c1, c2 = vc.glv_decompose(c)
    s1, s2 = vc.glv_decompose(s)
    q = [-_sgn(c1) * gam, -_sgn(c2) * LAM * gam, _sgn(s1) * h, _sgn(s2) * LAM * h]       # discrete logarithms of Q0..Q3
    out = []
    for u in range(8):
        p = g.gmul(q[0] + sum(q[t + 1] for t in range(3) if (u >> t) & 1))
        out.append(_xy(p) + (S.d * p[0] * p[1] % Q).to_bytes(32, "little"))
    return out


def run_v(hv, g, h, gam, c, s):
    v, ent = ctypes.create_string_buffer(64), ctypes.create_string_buffer(8 * 96)
    hv.hvs_v(_xy(g.gmul(h)), _xy(g.gmul(gam)), int(c).to_bytes(32, "little"), int(s).to_bytes(32, "little"), v, ent)
    return v.raw, [ent.raw[96 * u:96 * u + 96] for u in range(8)]


def point_rows():
    """(tag, h, gam): discrete logarithms of H and Gamma"""
    rng = random.Random(0x5AC1)
    h = rng.randrange(1, R)
    return [("random", h, rng.randrange(1, R)), ("H=Gamma", h, h), ("H=-Gamma", h, R - h), ("H neutral", 0, h),
            ("Gamma neutral", h, 0), ("both neutral", 0, 0), ("Gamma=psi(H)", h, LAM * h % R), ("Gamma=-psi(H)", h, R - LAM * h % R)]


def test_v_and_its_entries_equal_the_integers(hv):
    g = vc.group("bandersnatch")
    pairs = scalar_pairs()
    rows = point_rows()
    assert g.gmul(0) == ID
    n = 0
    for tag, h, gam in rows:
        for c, s in (pairs if tag == "random" else pairs[:40]):
            cr, sr = reduced(c, s)
            v, ent = run_v(hv, g, h, gam, c, s)
            assert v == _xy(g.gmul(sr * h - cr * gam)), (tag, hex(c), hex(s))
            assert ent == expected_entries(g, h, gam, cr, sr), (tag, hex(c), hex(s))
            n += 1
    assert n >= 256 + 7 * 40
    # all-zero scalars and a zero half 0 give the neutral V: the walk ran with half 0 + 1 and took Q0 back
    assert run_v(hv, g, rows[0][1], rows[0][2], 0, 0)[0] == _xy(ID)
    assert run_v(hv, g, rows[0][1], rows[0][2], 5, R + 1)[0] == _xy(ID)
    assert run_v(hv, g, 5, 3, LAM, 3 * LAM % R)[0] == _xy(g.gmul(3 * LAM * 5 - LAM * 3))      # half 0 of c and of s is zero


def ride(hv, enc, p):
    x, pinv = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32)
    rc = hv.hvs_ride(enc, p.to_bytes(32, "little"), x, pinv)
    return rc, int.from_bytes(x.raw, "little"), int.from_bytes(pinv.raw, "little")


def test_the_inversion_rides_on_the_inverse_root(hv):
    g = vc.group("bandersnatch")
    rng = random.Random(0x5AC2)
    for _ in range(256):
        pt = g.gmul(rng.randrange(1, R))
        p = rng.randrange(1, Q)
        rc, x, pinv = ride(hv, g.enc_in(pt), p)
        assert rc == 3 and x == pt[0], hex(p)
        assert pinv == pow(p, -1, Q), hex(p)
        # r' P = x / num is an inverse root of num den
        num, den = (pt[1] * pt[1] - 1) % Q, (S.d * pt[1] * pt[1] - S.a) % Q
        rp = x * pow(num, -1, Q) % Q
        assert rp * rp * num * den % Q == 1
    # a non-square radicand reports non-square, with and without the ride
    bad = [g.undecodable()]
    while len(bad) < 16:
        raw = rng.randrange(Q).to_bytes(32, "little")
        if vo.point_decode(S, raw) is None:
            bad.append(raw)
    for raw in bad:
        rc, _, _ = ride(hv, raw, rng.randrange(1, Q))
        assert rc == 2, raw.hex()
    # num = 0: x = 0 decodes with either sign flag, as arkworks accepts it, and 1 / P still comes out
    for y in (1, Q - 1):
        for flag in (0, 0x80):
            raw = bytearray(y.to_bytes(32, "little"))
            raw[31] |= flag
            p = rng.randrange(1, Q)
            rc, x, pinv = ride(hv, bytes(raw), p)
            assert rc == 3 and x == 0 and pinv == pow(p, -1, Q), (y, flag)
    # P = 0 (points off the prime-order subgroup only): 1 / P comes out 0
    rc, _, pinv = ride(hv, g.enc_in(g.gmul(77)), 0)
    assert pinv == 0


def decode_entries(hv, form, g, a, h, c, s):
    pts = [g.gmul(a), g.gmul(h), g.gmul(a * h)]
    enc = [_xy(p) for p in pts] if form == 3 else [g.enc_in(p) for p in pts]
    ent = ctypes.create_string_buffer(8 * 96)
    ok = hv.hvs_decode_entries(form, enc[0], enc[1], enc[2], g.scalar(c), g.scalar(s), ent)
    return ok, [ent.raw[96 * u:96 * u + 96] for u in range(8)]


def test_every_decode_form_leaves_the_same_entries(hv):
    """forms: compressed points; H parked by hash-to-curve, then pk and Gamma; the keyed form (H and Gamma, its own inversion);
    x || y inputs (its own inversion) -- for all 16 sign patterns of the GLV halves of c and s"""
    g = vc.group("bandersnatch")
    signs = [k for t, k in vc.glv_scalars() if t.startswith("glv-sign")]
    a, h = 0x1234567 + 3 * LAM % R, 0x7654321
    for form in (0, 1, 2, 3):
        for c in signs:
            for s in signs:
                ok, ent = decode_entries(hv, form, g, a, h, c, s)
                assert ok == 1 and ent == expected_entries(g, h, a * h, c, s), (form, hex(c), hex(s))
    # the neutral element as pk and Gamma (x = 0: the ride's radicand is P^2 alone), and entries that cancel (Gamma = +-H)
    for a0 in (0, 1, R - 1):
        for form in (0, 1, 2):
            ok, ent = decode_entries(hv, form, g, a0, h, signs[1], signs[2])
            assert ok == 1 and ent == expected_entries(g, h, a0 * h, signs[1], signs[2]), (a0, form)
