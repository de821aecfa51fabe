"""CPU: the joint-table IETF verifier of the GLV suite (vrf_core.cuh build_joint_y_table, build_joint_v_table, joint_u_ladder,
joint_v_ladder) compiled for the host (tests/hostsim_joint) and staged as the kernels stage it.

- the whole case sets of tests/verify_uv_cases.py, at the suite's challenge length and at 16, byte for byte: u, v, status;
- the table contents: every JT_V entry is the oracle's subset sum of the four signed bases, every JT_Y entry a*Y + b*psi(Y),
  for all 16 sign patterns of the GLV halves of c and s, through the three decode forms, with the neutral element as pk and
  as Gamma;
- the recodings: signed radix-4 digits in {-1, 0, 1, 2} and the V index bits re-sum to the magnitudes they came from.

As tests/test_hostsim_verify_uv.py, this pins logic, not code generation: the device test is tests/test_gpu_verify_joint.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import verify_uv_cases as vc
from oracle import vrf_oracle as vo

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim_joint")
S = vo.BANDERSNATCH
R = S.r
LAM = vc._GLV["lam"]
CHK_ALL = 7
# (a, b) of the JT_Y entries, in table order
Y_ENTRIES = [(1, 0), (2, 0), (0, 1), (0, 2), (1, 1), (1, -1), (1, 2), (1, -2), (2, 1), (2, -1), (2, 2), (2, -2)]


@pytest.fixture(scope="module")
def hj():
    subprocess.run(["make", "-C", HERE, "libhostsim_joint.so"], check=True, stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(os.path.join(HERE, "libhostsim_joint.so"))
    lib.hjt_verify_uv.restype = ctypes.c_uint32
    lib.hjt_tables.restype = ctypes.c_uint32
    lib.hjt_y_index.restype = ctypes.c_uint32
    lib.hjt_init()
    return lib


@pytest.mark.parametrize("L", [None, 16])
def test_joint_ladders_on_the_whole_set(hj, L):
    cs = vc.cases("bandersnatch", L) if L else vc.cases("bandersnatch")
    assert cs.n < 800
    u, v, st = np.zeros((cs.n, 32), np.uint8), np.zeros((cs.n, 32), np.uint8), np.zeros(cs.n, np.uint8)
    ub, vb = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32)
    for i in range(cs.n):
        st[i] = hj.hjt_verify_uv(cs.L, CHK_ALL, cs.pk[i].tobytes(), cs.input[i].tobytes(), cs.output[i].tobytes(),
                                 cs.c[i].tobytes(), cs.s[i].tobytes(), ub, vb)
        u[i], v[i] = np.frombuffer(ub.raw, np.uint8), np.frombuffer(vb.raw, np.uint8)
    bad = np.flatnonzero((st != cs.status) | (u != cs.u).any(axis=1) | (v != cs.v).any(axis=1))
    assert bad.size == 0, "L=%d: %d cases differ: %s" % (cs.L, bad.size, [(cs.tags[i], int(st[i])) for i in bad[:12]])


def _xy(p):
    return p[0].to_bytes(32, "little") + p[1].to_bytes(32, "little")


def _sgn(k):
    return -1 if k < 0 else 1            # a zero half counts as positive, as glv_finish reports it


def _expected_tables(g, a, h, c, s):
    """affine x || y of the 12 + 15 entries for pk = a*G, H = h*G, Gamma = a*h*G"""
    c1, c2 = vc.glv_decompose(c)
    s1, s2 = vc.glv_decompose(s)
    ys = [g.gmul((ya + yb * LAM) * a) for ya, yb in Y_ENTRIES]
    q = [-_sgn(c1) * a * h, -_sgn(c2) * LAM * a * h, _sgn(s1) * h, _sgn(s2) * LAM * h]       # discrete logarithms of Q0..Q3
    vs = [g.gmul(sum(q[t] for t in range(4) if (m >> t) & 1)) for m in range(1, 16)]
    return ys, vs


def _tables(hj, form, g, a, h, c, s):
    out = ctypes.create_string_buffer(27 * 64)
    enc = [g.enc_in(g.gmul(k)) for k in (a, h, a * h)]
    bad = hj.hjt_tables(form, enc[0], enc[1], enc[2], g.scalar(c), g.scalar(s), out)
    return bad, [out.raw[64 * i:64 * i + 64] for i in range(27)]


def test_table_entries_are_the_oracles_sums(hj):
    g = vc.group("bandersnatch")
    signs = [k for t, k in vc.glv_scalars() if t.startswith("glv-sign")]
    assert len(signs) == 4
    patterns = set()
    a, h = 0x1234567 + 3 * LAM % R, 0x7654321
    for form in (0, 1, 2):
        for c in signs:
            for s in signs:
                patterns.add(tuple(x < 0 for x in vc.glv_decompose(c) + vc.glv_decompose(s)))
                ys, vs = _expected_tables(g, a, h, c, s)
                bad, got = _tables(hj, form, g, a, h, c, s)
                if form == 2:                                  # the keyed decode builds no JT_Y
                    bad &= ~0xfff
                else:
                    assert got[:12] == [_xy(p) for p in ys], (form, hex(c), hex(s))
                assert got[12:] == [_xy(p) for p in vs], (form, hex(c), hex(s))
                assert bad == 0, (form, hex(bad))
    assert len(patterns) == 16
    # the neutral element as pk and as Gamma (a = 0), and as V entries that cancel (a = 1: Q0 + Q2 = -/+H +/- H)
    for a0 in (0, 1, R - 1):
        c, s = signs[1], signs[2]
        ys, vs = _expected_tables(g, a0, h, c, s)
        bad, got = _tables(hj, 0, g, a0, h, c, s)
        assert got == [_xy(p) for p in ys + vs] and bad == 0, a0
    assert _xy(vo.te_identity()) in _tables(hj, 0, g, 0, h, signs[0], signs[0])[1]


def test_joint_y_index_names_every_digit_pair(hj):
    for a in range(-2, 3):
        for b in range(-2, 3):
            r = hj.hjt_y_index(a, b)
            idx, neg = r & 0xff, bool(r >> 8)
            if (a, b) == (0, 0):
                assert idx == 0
                continue
            ea, eb = Y_ENTRIES[idx - 1]
            assert (ea, eb) == ((-a, -b) if neg else (a, b)), (a, b, idx, neg)


def _magnitudes():
    cap = vc.GLV_CAP
    mags = [0, 1, 2, 3, cap, cap - 1]
    mags += [vc._below(int(p * 8, 16), cap) for p in ("5555", "aaaa", "ffff")] + [vc._below((1 << 127) - 1, cap)]
    for t, k in vc.glv_scalars():
        if t.startswith("glv-max"):
            mags += [abs(x) for x in vc.glv_decompose(k)]
    assert all(0 <= m <= cap for m in mags) and len(mags) >= 10 + 64
    return mags


def test_recodings_resum_to_the_magnitude(hj):
    mags = _magnitudes()
    d = (ctypes.c_int8 * 64)()
    for m in mags:
        hj.hjt_digits2(m.to_bytes(16, "little"), d)
        digits = list(d)
        assert set(digits) <= {-1, 0, 1, 2}, hex(m)
        assert sum(x << (2 * w) for w, x in enumerate(digits)) == m, hex(m)
    out = ctypes.create_string_buffer(127)
    for i in range(0, len(mags) - 3):
        four = mags[i:i + 4]
        hj.hjt_vbits(b"".join(m.to_bytes(16, "little") for m in four), out)
        for t in range(4):
            assert sum(((out.raw[bit] >> t) & 1) << bit for bit in range(127)) == four[t], (i, t)
