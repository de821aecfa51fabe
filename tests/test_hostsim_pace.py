"""CPU: the evenly paced divsteps rounds of fe.cuh (jac_steps_paced under jacobi_limbs and fe_inv<false>) and the
decompression by inverse root of vrf_core.cuh (decode_by_inv_root), compiled for the host as a stand-alone program
(tests/hostsim_pace), once per base field of the Edwards suites, plain and under the undefined-behaviour sanitizer,
against Python integers.

- the symbol against pow(x, (q - 1) / 2, q) and the inverse against pow(a, -1, q) (0 -> 0) on 0, 1, 2, q - 1, q, q + 1, the
  powers of two, values with long runs of low zero bits, the inputs that needed the most rounds among 1.2e5 random ones
  (found once, listed below) and 10^4 seeded random values.  No input of that set may reach the exponentiation fallback;
  the largest round count is printed (pytest -s).  q - 2^k rides the slow cycle of the paced rounds (two steps per trip):
  its values are checked too, and for the symbol a give-up (2) is a legal answer there, as the rounds of 29 single steps
  give up on some of them (tests/test_divsteps.py).
- the decompression against oracle.vrf_oracle.point_decode for both sign flags: the same x byte for byte or the same
  rejection, on points of the curve, y with no point, the y with d y^2 = a where the field has one, y = 1 and y = q - 1
  (x = 0) and y >= q; Ed25519's field under both sign conventions.

This pins logic; the device test is tests/test_gpu_decode_paced.py."""
import os
import random
import re
import subprocess

import pytest

from oracle import vrf_oracle as vo

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim_pace")
C_FE = os.path.join(os.path.dirname(HERE), os.pardir, "ark_ec_vrfs_amd", "csrc", "fe.cuh")
JAC_VAR_ROUNDS = int(re.search(r"constexpr int JAC_VAR_ROUNDS = (\d+);", open(C_FE).read()).group(1))
Q_BLS, Q_25519, Q_BN254 = vo.Q, vo.Q_25519, vo.Q_BN254

# field build -> (q, Montgomery radix, the inputs of the largest round count in 1.2e5 random values: the three largest
# "rounds" bytes of `hostsim_pace_f<field> jac` and `... inv` over [random.Random(1000 + field).randrange(q) for 120000],
# found with JAC_NITER = 8; a change of the trip count wants them found again,
# for the symbol (35, 35, 34 / 35, 34, 34 / 36, 34, 34 rounds) and for the inverse (35, 35, 34 / as the symbol / 35, 34, 34))
FIELDS = {
    0: (Q_BLS, 1 << 261,
        [0x6cb2d8e8bfd0d76c22b0545ecfade2c12e4a6fa95012dc327bb685b66ce28019,
         0xa870f7a6f0effec8937e0d9366cc9e1f97d2e9809d9a84da6f180014f6ec9d,
         0x349652a894b40ace5e89595d7b8bb40d487ecb42be39885bce3ebd0b15e45846],
        [0x1ed892bacbf20978f3d08627115089720afce8fbfc8a89e4ba6316564c297f88,
         0x979b1e94c97b32c27556d0b3a9c2c8ed630a41dc63f2ab7eaf75cec0ca1174e,
         0x53f33b1a34af9515bb84808737f0f52f6adfb474b8a857003c0babf3dc016ac7]),
    1: (Q_25519, 1,
        [0x67c419243a9e03c51fb875a082b6247f48f12808d3aff5c83c6a7f450abd6eeb,
         0x47d261a34e6c730f5176f3d93c2ca83ea1c5a2b2283634d9c80acf1d353113e4,
         0x24c6587aa908eb84d1f17c9ea60183da6834c6444aa7f1a60276a439af25d116],
        []),
    2: (Q_BN254, 1 << 261,
        [0x197da4803e34fb863b71630ed4f488b57814277da285963a802465258f430259,
         0x2e5658ffe6b15371634e11b8ed1ce6fa8e8c7562c78f605eaca802c4a358a395,
         0x2babc5926b6dd5794443e6a769ba38a0c63b43940ca63b505ae3c0e83824c436],
        [0x183590df1c6b7f005f0ea82b91cc7943aeb07949dc7baee574ae8d89311a00b7,
         0x26a5dfd29c75415c231e69cc9b8b3b4e59817af6be8cb67b4f15761b457577d3,
         0x261c83228eea7d85a3a1c64e475df7a1d2defcda9734103d56dce100f0487e3b]),
}
# field build -> [(suite of the oracle, SuiteStr::flags)]
SUITES = {
    0: [(vo.BANDERSNATCH, 0)],
    1: [(vo.ed25519_params(), 0), (vo.ed25519_rfc9381_params(), 1)],
    2: [(vo.baby_jubjub_params(), 0)],
}


@pytest.fixture(scope="module")
def built():
    subprocess.run(["make", "-C", HERE, "-j4"], check=True, stdout=subprocess.DEVNULL)


@pytest.fixture(params=["", "_ubsan"], ids=["plain", "ubsan"])
def variant(request):
    return request.param


def _run(field, variant, args, values):
    prog = os.path.join(HERE, "hostsim_pace_f%d%s" % (field, variant))
    r = subprocess.run([prog] + args, input=b"".join(v.to_bytes(32, "little") for v in values), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-2000:]          # the sanitizer build aborts on its first finding
    return r.stdout


def _inputs(field, worst):
    """(the set that must not reach the fallback, q - 2^k)"""
    q = FIELDS[field][0]
    rnd = random.Random(7700 + field)
    xs = [0, 1, 2, q - 1, q, q + 1]
    xs += [1 << k for k in range(256) if (1 << k) < 2 * q]
    xs += [(rnd.randrange(q >> k) | 1) << k for k in range(8, 250, 2)]          # long runs of low zero bits
    xs += worst
    xs += [rnd.randrange(q) for _ in range(10_000)]
    assert all(0 <= x < 2 * q and x < 1 << 256 for x in xs)
    return xs, [q - (1 << k) for k in range(1, 250)]


@pytest.mark.parametrize("field", sorted(FIELDS))
def test_symbol_against_the_euler_criterion(built, variant, field):
    q, _, worst, _ = FIELDS[field]
    xs, slow = _inputs(field, worst)
    out = _run(field, variant, ["jac"], xs + slow)
    assert len(out) == 2 * (len(xs) + len(slow))
    most = 0
    for i, x in enumerate(xs + slow):
        got, rounds = int.from_bytes(out[2 * i:2 * i + 1], "little", signed=True), out[2 * i + 1]
        e = pow(x % q, (q - 1) // 2, q)
        want = -1 if e == q - 1 else e
        if i < len(xs):
            assert got != 2, "field %d: %s reached the fallback after %d rounds" % (field, hex(x), rounds)
            most = max(most, rounds)
        assert got == want or (i >= len(xs) and got == 2), (field, hex(x), got, want, rounds)
    print("field %d%s: symbol, most rounds %d of %d" % (field, variant, most, JAC_VAR_ROUNDS))
    assert most < JAC_VAR_ROUNDS


@pytest.mark.parametrize("field", sorted(FIELDS))
def test_inverse_against_pow(built, variant, field):
    q, _, worst_sym, worst_inv = FIELDS[field]
    xs, slow = _inputs(field, worst_sym + worst_inv)
    out = _run(field, variant, ["inv"], xs + slow)
    assert len(out) == 33 * (len(xs) + len(slow))
    most = 0
    for i, x in enumerate(xs + slow):
        got, rounds = int.from_bytes(out[33 * i:33 * i + 32], "little"), out[33 * i + 32]
        want = pow(x % q, -1, q) if x % q else 0
        assert got == want, (field, hex(x), hex(got), rounds)
        if i < len(xs):
            assert rounds != 255, "field %d: %s reached the fallback" % (field, hex(x))
            most = max(most, rounds)
    print("field %d%s: inverse, most rounds %d of %d" % (field, variant, most, JAC_VAR_ROUNDS))
    assert most < JAC_VAR_ROUNDS


def _decode_cases(S, seed):
    """y values: on the curve and off it, d y^2 = a, x = 0, y >= q; each goes in with both sign flags."""
    q = S.q
    rnd = random.Random(seed)
    ys = [rnd.randrange(q) for _ in range(400)]                  # about half have a point
    ys += [0, 1, q - 1, 2, q - 2]                                # y = +-1: x = 0
    y2 = S.a * pow(S.d, -1, q) % q                               # den = d y^2 - a = 0
    r = vo.fsqrt(y2, q)
    n_den0 = 0
    if r is not None:
        ys += [r, q - r]
        n_den0 = 2
    ys += [y for y in (q, q + 1, q + 2, (1 << 255) - 1) if y < 1 << 255]          # not canonical
    return ys, n_den0


@pytest.mark.parametrize("field", sorted(SUITES))
def test_decompression_by_inverse_root(built, variant, field):
    for S, flags in SUITES[field]:
        ys, n_den0 = _decode_cases(S, 8800 + field)
        encs = [y | (f << 255) for y in ys for f in (0, 1)]
        out = _run(field, variant, ["dec", str(flags)], encs)
        assert len(out) == 33 * len(encs)
        accepted = zero_x = 0
        for i, e in enumerate(encs):
            want = vo.point_decode(S, e.to_bytes(32, "little"))
            ok, x = out[33 * i], out[33 * i + 1:33 * i + 33]
            assert ok == (want is not None), (S.name, hex(e), ok)
            if want is not None:
                assert x == want[0].to_bytes(32, "little"), (S.name, hex(e))
                assert vo.te_is_on_curve(S, want)
                accepted += 1
                zero_x += want[0] == 0
        # the case groups are all there: points and non-points, x = 0 under either flag (RFC 8032's convention refuses
        # x = 0 with the flag set), and the vanishing denominator where the field has one (Ed25519's and Baby-JubJub's
        # a / d is a non-residue: none; Bandersnatch has it)
        assert 300 < accepted < len(encs) - 300
        assert zero_x == (2 if flags & 1 else 4)
        if field == 0:
            assert n_den0 == 2
