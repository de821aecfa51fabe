"""The bucket pass of the multi-scalar multiplications (msm_buckets.cuh) at the inputs where its SCHEDULE -- the counting sort,
the equal chunks, the head chains, the reduction over the buckets -- can go wrong rather than the group law: the same crafted
cases through `VariableBaseMSM::msm` on the twisted-Edwards curves (one suite per base-field build: Bandersnatch, Ed25519,
Baby-JubJub; two buckets per lane), on secp256r1 and on BLS12-381 G1.

Expected values come from discrete logs: the bases are drawn from a pool of 16 points a_i G, so the result is
(sum_i k_i a_i mod r) G -- one scalar multiplication of the Python oracle per case."""
import random

import numpy as np
import pytest

from oracle import bls_oracle as bls
from oracle import sw_oracle as sw
from oracle import vrf_oracle as o

pytestmark = pytest.mark.gpu

POOL = 16


def le32(v):
    return int(v).to_bytes(32, "little")


class EdwardsMsm:
    """Signed 11-bit windows, 1024 buckets on 512 lanes, groups of at most 8192 points (msm_groups)."""
    C, TWO_GROUPS, INF = 11, 8193, le32(0) + le32(1)              # no point at infinity: the identity is an ordinary point

    def __init__(self, S, suite):
        from ark_ec_vrfs_amd import Context
        self.S, self.r = S, S.r
        self.ctx = Context(0) if suite is None else Context(0, suite=suite)
        self.G = (S.gx, S.gy)

    def mul(self, k):
        return o.te_mul(self.S, k, self.G)

    def neg(self, P):
        return o.te_neg(self.S, P)

    def enc(self, P):
        return le32(P[0]) + le32(P[1])

    def run(self, bases, ks):
        return self.ctx.msm(np.frombuffer(b"".join(bases), np.uint8).reshape(-1, 64),
                            np.frombuffer(b"".join(le32(k) for k in ks), np.uint8).reshape(-1, 32))

    def want(self, log):
        P = self.mul(log) if log else (0, 1)
        return o.point_encode(self.S, P), self.enc(P)


class P256Msm:
    """Signed 10-bit windows, 512 buckets, groups of at most 4096 points (p256::msm_groups)."""
    C, TWO_GROUPS, INF, r = 10, 4097, bytes(64), sw.N

    def __init__(self):
        from ark_ec_vrfs_amd import Context, Secp256r1Sha256Tai
        self.ctx = Context(0, Secp256r1Sha256Tai)

    def mul(self, k):
        return sw.mul(k, sw.G)

    def neg(self, P):
        return sw.neg(P)

    def enc(self, P):
        return le32(P[0]) + le32(P[1])

    def run(self, bases, ks):
        return self.ctx.msm(np.frombuffer(b"".join(bases), np.uint8).reshape(-1, 64),
                            np.frombuffer(b"".join(int(k).to_bytes(32, "big") for k in ks), np.uint8).reshape(-1, 32))

    def want(self, log):
        if not log:
            return bytes(33), bytes(64)
        P = self.mul(log)
        return sw.point_encode(P), self.enc(P)


class G1Msm:
    """Signed 10-bit windows, 512 buckets, groups of at most 2048 points (g1_msm_groups), scalars not folded."""
    C, TWO_GROUPS, INF, r = 10, 2049, bytes(96), bls.R

    def __init__(self):
        from ark_ec_vrfs_amd import Context
        self.ctx = Context(0)
        assert self.ctx._lib.vrfhip_test_g1_msm_groups(self.ctx.handle, self.TWO_GROUPS, 1, 26) == 2
        assert self.ctx._lib.vrfhip_test_g1_msm_groups(self.ctx.handle, self.TWO_GROUPS - 1, 1, 26) == 1

    def mul(self, k):
        return bls.g1_mul(k, bls.G1)

    def neg(self, P):
        return bls.g1_neg(P)

    def enc(self, P):
        return int(P[0]).to_bytes(48, "little") + int(P[1]).to_bytes(48, "little")

    def run(self, bases, ks):
        return self.ctx.g1_msm(np.frombuffer(b"".join(bases), np.uint8).reshape(-1, 96),
                               np.frombuffer(b"".join(le32(k) for k in ks), np.uint8).reshape(-1, 32))

    def want(self, log):
        return self.enc(self.mul(log)) if log else bytes(96)


def _make(name):
    from ark_ec_vrfs_amd import BabyJubJubSha512Tai, Ed25519Sha512Tai
    if name == "bandersnatch":
        return EdwardsMsm(o.BANDERSNATCH, None)
    if name == "ed25519":
        return EdwardsMsm(o.ed25519_params(), Ed25519Sha512Tai)
    if name == "babyjubjub":
        return EdwardsMsm(o.baby_jubjub_params(), BabyJubJubSha512Tai)
    return P256Msm() if name == "secp256r1" else G1Msm()


@pytest.fixture(scope="module", params=["bandersnatch", "ed25519", "babyjubjub", "secp256r1", "g1"])
def msm(request):
    """The MSM under test with its pool: logs a_i, the points a_i G and -a_i G in the entry point's base format."""
    m = _make(request.param)
    rnd = random.Random(1100 + len(request.param))
    m.logs = [rnd.randrange(1, m.r) for _ in range(POOL)]
    pts = [m.mul(a) for a in m.logs]
    m.pos = [m.enc(P) for P in pts]
    m.negs = [m.enc(m.neg(P)) for P in pts]
    yield m
    m.ctx.close()


def _check(m, idx, ks, signs=None):
    """sum_i k_i (+-)P_idx[i] through the MSM against its discrete log; idx[i] = None: the neutral element."""
    signs = signs or [1] * len(idx)
    bases = [m.INF if i is None else (m.pos if s > 0 else m.negs)[i] for i, s in zip(idx, signs)]
    log = sum(s * k * m.logs[i] for i, k, s in zip(idx, ks, signs) if i is not None) % m.r
    assert m.run(bases, ks) == m.want(log)


def _windows(m, v):
    """The scalar whose windows below bit 250 all hold v."""
    return sum(v << (m.C * w) for w in range(250 // m.C))


@pytest.mark.parametrize("n", [1, 2, 511, 512, 513])
def test_fewer_points_than_lanes_and_chunks_of_one(msm, n):
    """n <= 513 points in 512 lanes: lanes without a chunk (cnt = 0), chunk = 1, and the first n that gives chunk = 2 in a
    window whose points are spread thinly."""
    rnd = random.Random(n)
    _check(msm, [rnd.randrange(POOL) for _ in range(n)], [rnd.randrange(msm.r) for _ in range(n)])


def test_two_point_groups_the_second_one_ragged(msm):
    """The first n that makes two point groups: the second one holds a single point (*_groups: the max_g line)."""
    n = msm.TWO_GROUPS
    rnd = random.Random(21)
    _check(msm, [rnd.randrange(POOL) for _ in range(n)], [rnd.randrange(msm.r) for _ in range(n)])


def test_two_point_groups_of_128_bit_scalars(msm):
    """128-bit scalars only at the two-group size: every bucket of the high windows stays empty."""
    n = msm.TWO_GROUPS
    rnd = random.Random(22)
    _check(msm, [rnd.randrange(POOL) for _ in range(n)], [rnd.randrange(1 << 128) for _ in range(n)])


def test_every_scalar_equal_one_head_chain_through_all_lanes(msm):
    """n = 2048 with one scalar: each window's points fall into ONE bucket, every lane's chunk is the continuation of the
    previous lane's run, so the head chain runs through all 512 lanes and every other bucket is empty."""
    n = 2048
    rnd = random.Random(23)
    k = rnd.randrange(1, msm.r)
    _check(msm, [rnd.randrange(POOL) for _ in range(n)], [k] * n)


def test_two_scalars_in_adjacent_buckets(msm):
    """Scalars from a set of two whose buckets are adjacent in every window: runs that start and end inside a chunk next to
    runs that continue across lanes, at an uneven split so that the boundary falls inside a lane's chunk."""
    n = 2048
    rnd = random.Random(24)
    half = 1 << (msm.C - 1)
    k0 = sum(rnd.randrange(1, half - 1) << (msm.C * w) for w in range(250 // msm.C))
    k1 = k0 + _windows(msm, 1)                                            # every window one bucket further, no carry
    _check(msm, [rnd.randrange(POOL) for _ in range(n)], [k0 if rnd.randrange(3) else k1 for _ in range(n)])


@pytest.mark.parametrize("negated", [False, True], ids=["below_half_order", "negated_mod_r"])
@pytest.mark.parametrize("plus", [0, 1], ids=["last_bucket_no_carry", "negative_digits_carry_chain"])
def test_window_values_at_the_sign_boundary(msm, plus, negated):
    """Every window 2^(C-1): the last bucket, no carry.  Every window 2^(C-1) + 1: a negative digit in every window and a
    carry through all of them.  Both below half the group order, where the fold leaves them alone, and negated mod r,
    where it (or, on G1, the unfolded recoding of r - k) does not."""
    n = 700
    rnd = random.Random(25 + plus)
    k = _windows(msm, (1 << (msm.C - 1)) + plus)
    assert k < msm.r // 2
    _check(msm, [rnd.randrange(POOL) for _ in range(n)], [msm.r - k if negated else k] * n)


def test_p_p_and_minus_p_in_one_bucket_and_an_identity_sum(msm):
    """One scalar over P, P, -P: a bucket meets a doubling and a cancellation; P and -P alone: the sum is the identity."""
    rnd = random.Random(27)
    k = rnd.randrange(1, msm.r)
    _check(msm, [3, 3, 3], [k] * 3, [1, 1, -1])
    _check(msm, [5, 5], [k] * 2, [1, -1])
    _check(msm, [3, 3, 3, 5, 5], [k] * 5, [1, -1, 1, -1, 1])


def test_neutral_element_among_the_bases(msm):
    """secp256r1 and G1 take the point at infinity as a base: its digits are zero and its slot is never read.  On the
    twisted-Edwards curves the neutral element (0, 1) is an ordinary affine point that lands in buckets like any other."""
    n = 513
    rnd = random.Random(28)
    idx = [None if j % 7 == 3 else rnd.randrange(POOL) for j in range(n)]
    _check(msm, idx, [rnd.randrange(1, msm.r) for _ in range(n)])
    _check(msm, [None, None], [1, msm.r - 1])
