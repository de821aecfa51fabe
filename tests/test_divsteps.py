"""CPU: the Jacobi symbol and the inversion of fe.cuh (positive divsteps, several per iteration) compiled for the host
(tests/hostsim) for all four base fields, against Python big ints and against a model of the rounds of single steps.

Each round of jacobi_limbs / fe_inv runs JAC_K = 29 divsteps on the low words and gives up (2, then the callers take
the exponentiation) after JAC_MAX_ROUNDS = 40 rounds.  The model below runs those rounds one step at a time, so the
results, the give-ups included, must match it exactly."""
import ctypes
import os
import random
import subprocess

import pytest

from oracle import vrf_oracle as o

HS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim")
P256 = 0xffffffff00000001000000000000000000000000ffffffffffffffffffffffff
JAC_K, JAC_MAX_ROUNDS = 29, 40
N_RANDOM = 100_000

# field -> (library, prefix, byte order, q, Montgomery radix R: the divsteps see the canonical image x R mod q)
FIELDS = {
    "bls12_381_fr": ("libhostsim.so", "hs", "little", o.BANDERSNATCH.q, 1 << 261),
    "2^255-19": ("libhostsim_f1.so", "hx", "little", (1 << 255) - 19, 1),
    "bn254_fr": ("libhostsim_f2.so", "hx", "little",
                 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001, 1 << 261),
    "p256": ("libhostsim_p256.so", "hp", "big", P256, 1 << 261),
}


@pytest.fixture(scope="module", params=sorted(FIELDS))
def field(request):
    so, pre, order, q, radix = FIELDS[request.param]
    subprocess.run(["make", "-C", HS, "-j4", so], check=True, stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(os.path.join(HS, so))
    if hasattr(lib, pre + "_init"):
        getattr(lib, pre + "_init")()
    jac, inv = getattr(lib, pre + "_fe_jacobi"), getattr(lib, pre + "_fe_inv")
    buf = ctypes.create_string_buffer(32)

    def jacobi(x):
        return jac(x.to_bytes(32, order))

    def inverse(x):
        inv(x.to_bytes(32, order), buf)
        return int.from_bytes(buf.raw, order)

    return request.param, q, radix % q, jacobi, inverse


def _euler(x, q):
    a = x % q
    return 0 if a == 0 else (1 if pow(a, (q - 1) // 2, q) == 1 else -1)


def _model(q, g):
    """jacobi_limbs on the canonical image g, one divstep at a time: (symbol or 2, rounds run)."""
    if g == 0:
        return 0, 0
    f, eta, sign = q, -1, 0
    for rnd in range(1, JAC_MAX_ROUNDS + 1):
        for _ in range(JAC_K):
            if g & 1 and eta < 0:
                sign ^= (f & g) >> 1 & 1
                f, g, eta = g, f, -eta
            if g & 1:
                g += f
            g >>= 1
            eta -= 1
            sign ^= ((f >> 1) ^ (f >> 2)) & 1
        if f == 1:
            return (-1 if sign else 1), rnd
    return 2, JAC_MAX_ROUNDS


def _from_image(g, q, radix):
    """The input whose canonical image is g."""
    return g * pow(radix, -1, q) % q


def _edge_inputs(q, radix, rnd):
    xs = [0, 1, 2, 3, 5, 7, 9, 16, q - 1, q - 2, q, q + 1, 2 * q - 1, (q - 1) // 2, (q + 1) // 2]
    xs += list(range(2, 200)) + [1 << k for k in range(0, 256, 5)] + [q - (1 << k) for k in range(0, 250, 7)]
    # the same shapes as images, i.e. as the operands the divsteps actually start from
    xs += [_from_image(g, q, radix) for g in [1, 2, 3, q - 1, q - 2, (q - 1) // 2] + [1 << k for k in range(0, 255, 9)]]
    # the inputs that need the most rounds among a random sample
    sample = [rnd.randrange(1, q) for _ in range(3000)]
    sample.sort(key=lambda g: -_model(q, g)[1])
    xs += [_from_image(g, q, radix) for g in sample[:40]]
    return [x % (1 << 256) for x in xs]


def test_jacobi_symbol_matches_the_single_step_rounds(field):
    name, q, radix, jacobi, _ = field
    rnd = random.Random(31)
    edge = _edge_inputs(q, radix, rnd)
    gave_up = 0
    for x in edge + [rnd.randrange(q) for _ in range(2000)]:
        want, _ = _model(q, x % q * radix % q)
        got = jacobi(x % q if name == "p256" else x)
        assert got == want, (name, hex(x), got, want)
        assert want == 2 or want == _euler(x, q)
        gave_up += want == 2
    for _ in range(N_RANDOM):
        x = rnd.randrange(q)
        got = jacobi(x)
        if got == 2:                                    # rounds exhausted: the model must agree
            assert _model(q, x * radix % q)[0] == 2, (name, hex(x))
        else:
            assert got == _euler(x, q), (name, hex(x), got)
    if name == "2^255-19":
        assert gave_up >= 1                             # q - 2 needs more than 40 rounds there


def test_inverse_over_random_and_edge_inputs(field):
    name, q, radix, _, inverse = field
    rnd = random.Random(32)
    edge = _edge_inputs(q, radix, rnd)
    for x in edge:
        xr = x % q if name == "p256" else x
        assert inverse(xr) == pow(x % q, q - 2, q), (name, hex(x))
    for _ in range(N_RANDOM):
        x = rnd.randrange(1, q)
        assert inverse(x) * x % q == 1, (name, hex(x))
