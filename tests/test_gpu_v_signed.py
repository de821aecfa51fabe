"""GPU (-m gpu): V = s*H - c*Gamma of the GLV suite from the eight signed affine table entries (vrf_core.cuh
build_joint_va_table, joint_va_normalise, joint_va_ladder), read out of the verification kernels (vrfhip_test_verify_uv) and compared
byte for byte with integer arithmetic on the curve -- H and Gamma with independent discrete logarithms, sums that reach the
neutral element, neutral bases, Gamma = psi(H); scalars that are zero, equal, r - 1, at and above r -- at the batch sizes where
a wave is partly empty and where a second workgroup starts; U must stay what it was.  The same rows, and genuine proofs,
through the four verifying entry points against the C oracle's statuses, and one batch with the pre-validated flags set and a
Gamma off the prime-order subgroup in it.

The CPU counterpart, piece by piece, is tests/test_hostsim_v_signed.py."""
import random

import numpy as np
import pytest

import verify_uv_cases as vc
from oracle import c_oracle as co, vrf_oracle as vo

pytestmark = pytest.mark.gpu
S = vo.BANDERSNATCH
R = S.r
LAM = vc._GLV["lam"]
SIZES = (1, 63, 64, 65, 129)


def _arr(xs, w):
    return np.frombuffer(b"".join(xs), np.uint8).reshape(len(xs), w).copy()


class Rows:
    """pk = a*G, H = h*G, Gamma = gam*G with the scalars of each row; expected U, V and status by integers"""

    def __init__(self):
        g = vc.group("bandersnatch")
        rng = random.Random(0x5AC6)
        h = rng.randrange(1, R)
        points = [("random", h, rng.randrange(1, R)), ("H=Gamma", h, h), ("H=-Gamma", h, R - h), ("H neutral", 0, h),
                  ("Gamma neutral", h, 0), ("Gamma=psi(H)", h, LAM * h % R)]
        top = (1 << 256) - 1
        pairs = [(0, 0), (0, 1), (1, 0), (7, 7), (R - 1, R - 1), (R - 1, 0), (R, 5), (top, R - 2), (5, R), (LAM, 3 * LAM % R),
                 (2, 1)] + [(rng.randrange(R), rng.randrange(R)) for _ in range(5)]
        rows = []
        for tag, hh, gam in points:
            for c, s in pairs:
                a = rng.randrange(1, R)
                ok = s < R
                cr, sr = (c % R, s) if ok else (0, 0)
                u, v = g.gmul(sr - cr * a), g.gmul(sr * hh - cr * gam)
                pts = [g.gmul(a), g.gmul(hh), g.gmul(gam)]
                rows.append(("%s c=%x s=%x" % (tag, c, s), [g.enc_in(p) for p in pts], [g.xy(p) for p in pts],
                             int(c).to_bytes(32, "little"), int(s).to_bytes(32, "little"),
                             g.enc_out(u) if ok else bytes(32), g.enc_out(v) if ok else bytes(32), 0 if ok else 2))
        self.g, self.n = g, len(rows)
        self.tags = [r[0] for r in rows]
        self.pk, self.h, self.gamma = (_arr([r[1][k] for r in rows], 32) for k in range(3))
        self.pk_xy, self.h_xy, self.gamma_xy = (_arr([r[2][k] for r in rows], 64) for k in range(3))
        self.c, self.s = _arr([r[3] for r in rows], 32), _arr([r[4] for r in rows], 32)
        self.u, self.v = _arr([r[5] for r in rows], 32), _arr([r[6] for r in rows], 32)
        self.status = np.array([r[7] for r in rows], np.uint8)


@pytest.fixture(scope="module")
def rows():
    return Rows()


@pytest.fixture(scope="module")
def ctx():
    from ark_ec_vrfs_amd import BandersnatchSha512Ell2, Context
    c = Context(0, BandersnatchSha512Ell2)
    yield c
    c.close()


def _tile(n, total, shift):
    return (np.arange(n) + shift) % total


@pytest.mark.parametrize("n", SIZES)
def test_v_equals_the_integers_and_u_is_unchanged(ctx, rows, n):
    for shift in range(0, rows.n, max(n, 1)) if n < rows.n else (0,):        # small batches: every row is run
        r = _tile(n, rows.n, shift)
        u, v, st = ctx.test_verify_uv(rows.pk[r], rows.h[r], rows.gamma[r], rows.c[r], rows.s[r])
        bad = np.flatnonzero((st != rows.status[r]) | (u != rows.u[r]).any(axis=1) | (v != rows.v[r]).any(axis=1))
        assert bad.size == 0, "n=%d: %d items differ, first: %s" % (n, bad.size, [(int(i), rows.tags[r[i]], int(st[i])) for i in bad[:8]])
    if n == 65:                                      # the x || y form and the keyed form build the same table
        r = _tile(n, rows.n, 7)
        u, v, st = ctx.test_verify_uv(rows.pk_xy[r], rows.h_xy[r], rows.gamma_xy[r], rows.c[r], rows.s[r], affine=True)
        assert (st == rows.status[r]).all() and (u == rows.u[r]).all() and (v == rows.v[r]).all()
        ks, kst = ctx.keyset_create(rows.pk)
        try:
            assert not kst.any()
            u, v, st = ctx.test_verify_uv(None, rows.h[r], rows.gamma[r], rows.c[r], rows.s[r], keyset=ks, key_index=r.astype(np.uint32))
            assert (st == rows.status[r]).all() and (u == rows.u[r]).all() and (v == rows.v[r]).all()
        finally:
            ks.close()


def _genuine(n):
    """n genuine proofs from the C oracle: (pk, msgs, H, Gamma, c, s)"""
    rng = np.random.default_rng(0x5AC7)
    sk = np.zeros((n, 32), np.uint8)
    sk[:, :31] = rng.integers(0, 256, (n, 31), dtype=np.uint8)
    msgs = rng.integers(0, 256, (n, 24), dtype=np.uint8)
    co.set_suite(1)
    co.set_check_mask(15)
    p = co.ietf_prove_batch(sk, msgs=msgs)
    pk, h, gamma, c, s = p["pk"], p["input"], p["output"], p["c"], p["s"]
    assert not p["status"].any() and (co.ietf_verify_batch(pk, h, gamma, c, s) == 0).all()
    return pk, msgs, h, gamma, c, s


@pytest.mark.parametrize("n", (65, 129))
def test_statuses_equal_the_c_oracles_on_every_entry_point(ctx, rows, n):
    import torch
    co.set_suite(1)
    co.set_check_mask(15)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ngen = 16
    pk_g, msgs, h_g, gamma_g, c_g, s_g = _genuine(ngen)
    r = _tile(n - ngen, rows.n, 3)
    pk, h, gamma = (np.concatenate([a, b[r]]) for a, b in ((pk_g, rows.pk), (h_g, rows.h), (gamma_g, rows.gamma)))
    c, s = np.concatenate([c_g, rows.c[r]]), np.concatenate([s_g, rows.s[r]])
    c[1] = rows.c[5]                                     # a genuine proof with another challenge: VerificationFailure
    want = co.ietf_verify_batch(pk, h, gamma, c, s)
    assert set(want.tolist()) == {0, 1, 2} and (want[:ngen] == [0, 1] + [0] * (ngen - 2)).all()

    def run(call, *args):
        st = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
        call(*args, st)
        torch.cuda.synchronize()
        return st.cpu().numpy()

    got = run(ctx.ietf_verify_batch_dev, dev(pk), dev(h), dev(gamma), dev(c), dev(s))
    assert (got == want).all(), np.flatnonzero(got != want)[:8]
    # x || y inputs: the rows' own coordinates, the genuine proofs' through the oracle's decoder
    g = rows.g
    xy = lambda enc: g.xy(vo.point_decode(S, enc.tobytes()))
    pk_xy, h_xy, gamma_xy = (np.concatenate([_arr([xy(e) for e in a], 64), b[r]])
                             for a, b in ((pk_g, rows.pk_xy), (h_g, rows.h_xy), (gamma_g, rows.gamma_xy)))
    got = run(ctx.ietf_verify_batch_affine_dev, dev(pk_xy), dev(h_xy), dev(gamma_xy), dev(c), dev(s))
    assert (got == want).all(), np.flatnonzero(got != want)[:8]
    # keyed: the batch's own public keys as the key set
    ks, kst = ctx.keyset_create(pk)
    try:
        assert not kst.any()
        got = run(ctx.ietf_verify_batch_keyed_dev, ks, dev(np.arange(n, dtype=np.uint32)), dev(h), dev(gamma), dev(c), dev(s))
        assert (got == want).all(), np.flatnonzero(got != want)[:8]
    finally:
        ks.close()
    # from alpha: H is hashed on the device, so every row takes a message and the oracle's H for it
    m_all = np.concatenate([msgs, np.random.default_rng(0x5AC8).integers(0, 256, (n - ngen, 24), dtype=np.uint8)])
    h_a = _arr([co.hash_to_curve(m.tobytes()) for m in m_all], 32)
    want_a = co.ietf_verify_batch(pk, h_a, gamma, c, s)
    assert (want_a[:ngen] == want[:ngen]).all()
    got = run(lambda *a: ctx.ietf_verify_batch_alpha_dev(a[0], a[1], 24, *a[2:]), dev(pk), dev(m_all), dev(gamma), dev(c), dev(s))
    assert (got == want_a).all(), np.flatnonzero(got != want_a)[:8]


def test_an_off_subgroup_gamma_stays_inside_its_item(ctx, rows):
    """pre-validated flags set: nothing tests Gamma's subgroup, the product of the table's Z coordinates may vanish and the
    item's entries may be anything -- its neighbours' statuses are what they were and the call returns"""
    n = 129
    pk_g, _, h_g, gamma_g, c_g, s_g = _genuine(16)
    r = _tile(n - 16, rows.n, 11)
    pk, h, gamma = (np.concatenate([a, b[r]]) for a, b in ((pk_g, rows.pk), (h_g, rows.h), (gamma_g, rows.gamma)))
    c, s = np.concatenate([c_g, rows.c[r]]), np.concatenate([s_g, rows.s[r]])
    before = ctx.ietf_verify_batch(pk, h, gamma, c, s)
    g = rows.g
    victims = (3, 70)                       # one per workgroup of 64
    for i in victims:
        gamma[i] = np.frombuffer(g.off_subgroup(vo.point_decode(S, gamma[i].tobytes())), np.uint8)
    ctx.set_prevalidated(True)
    try:
        after = ctx.ietf_verify_batch(pk, h, gamma, c, s)
        u, v, st = ctx.test_verify_uv(pk, h, gamma, c, s)
    finally:
        ctx.set_prevalidated(False)
    keep = np.setdiff1d(np.arange(n), victims)
    assert (after[keep] == before[keep]).all() and (after[list(victims)] != 0).all()
    assert (st[keep] == np.where(before[keep] == 2, 2, 0)).all()
