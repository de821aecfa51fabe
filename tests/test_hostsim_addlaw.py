"""CPU: the fused sum of two products a*b + c*d with one reduction (fe.cuh: fe_mul2) and the twisted Edwards addition laws
built on it (te.cuh: te_add_cached, te_add_affine), compiled for the host once per base field (tests/hostsim_addlaw) and
compared with Python integers.

fe_mul2 takes raw lazy limbs: the test feeds 0, 1 and q - 1, operands whose every limb sits at the maximum its Fe<L, V>
type allows (at the operand types te.cuh uses and at the primitive's own limit L1 L2 + L3 L4 = 6), and random limbs, and
checks the residue, the limb bound and the value bound of what comes back.  The addition laws are compared as affine
points with oracle.vrf_oracle.te_add on Bandersnatch, JubJub, Ed25519 and Baby-JubJub."""
import ctypes
import os
import random
import subprocess

import pytest

from oracle import vrf_oracle as o

HERE = os.path.dirname(os.path.abspath(__file__))
SIM = os.path.join(HERE, "hostsim_addlaw")
NL, LW = 9, 29
Q_P256 = (1 << 256) - (1 << 224) + (1 << 192) + (1 << 96) - 1
FIELD_Q = {0: o.Q, 1: o.Q_25519, 2: o.Q_BN254, 3: Q_P256}
# operand types (L, V) of a, b, c, d per combination (hostsim_addlaw.hip: ha_mul2)
COMBOS = {0: ((1, 5), (1, 5), (1, 5), (2, 8)), 1: ((1, 5), (1, 5), (1, 25), (2, 8)), 2: ((2, 8), (2, 8), (1, 25), (2, 8))}
CURVES = {"bandersnatch": (0, 0, lambda: o.BANDERSNATCH), "jubjub": (0, 1, o.jubjub_params),
          "ed25519": (1, 0, o.ed25519_params), "baby_jubjub": (2, 0, o.baby_jubjub_params)}

_libs = {}


def lib(field):
    if field not in _libs:
        name = "libhostsim_addlaw_f%d.so" % field
        subprocess.run(["make", "-C", SIM, name], check=True, stdout=subprocess.DEVNULL)
        _libs[field] = ctypes.CDLL(os.path.join(SIM, name))
    return _libs[field]


def limbs_of(x):
    """exact limbs of an integer < 2^261"""
    return [(x >> (LW * i)) & ((1 << LW) - 1) for i in range(NL - 1)] + [x >> (LW * (NL - 1))]


def value_of(limbs):
    return sum(v << (LW * i) for i, v in enumerate(limbs))


def limb_cap(L):
    return L * ((1 << 29) + (1 << 13)) - 1


def top_cap(low, L, V, q):
    """the largest top limb that keeps low limbs + top * 2^232 below V q and inside the limb bound"""
    return min(limb_cap(L), (V * q - 1 - value_of(low + [0])) >> (LW * (NL - 1)))


def max_operand(L, V, q):
    low = [limb_cap(L)] * (NL - 1)
    return low + [top_cap(low, L, V, q)]


def random_operand(rnd, L, V, q):
    low = [rnd.randrange(limb_cap(L) + 1) for _ in range(NL - 1)]
    return low + [rnd.randrange(top_cap(low, L, V, q) + 1)]


def run_mul2(field, combo, items):
    n = len(items)
    flat = [v for it in items for op in it for v in op]
    assert all(0 <= v < 1 << 32 for v in flat)
    src = (ctypes.c_uint32 * (4 * NL * n))(*flat)
    dst = (ctypes.c_uint32 * (NL * n))()
    l = lib(field)
    l.ha_mul2.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    vout = l.ha_mul2(combo, n, src, dst)
    return vout, [list(dst[NL * i:NL * i + NL]) for i in range(n)]


@pytest.mark.parametrize("field", [0, 1, 2, 3])
@pytest.mark.parametrize("combo", [0, 1, 2])
def test_fe_mul2_against_integers(field, combo):
    q = FIELD_Q[field]
    kind = lib(field).ha_field_kind()
    assert kind == {0: 0, 1: 2, 2: 1, 3: 1}[field]
    rinv = 1 if kind == 2 else pow(1 << (LW * NL), -1, q)
    types = COMBOS[combo]
    assert types[0][0] * types[1][0] + types[2][0] * types[3][0] <= 6
    rnd = random.Random(1000 * field + combo)
    special = [limbs_of(v) for v in (0, 1, q - 1)]
    items = [(a, b, c, d) for a in special for b in special for c in special for d in special]
    mx = [max_operand(L, V, q) for L, V in types]
    items.append(tuple(mx))
    for mask in range(1, 15):                          # the maximum in some places, small values in the others
        items.append(tuple(mx[j] if mask >> j & 1 else special[(mask + j) % 3] for j in range(4)))
    items += [tuple(random_operand(rnd, L, V, q) for L, V in types) for _ in range(3000)]
    items += [tuple(limbs_of(rnd.randrange(q)) for _ in range(4)) for _ in range(500)]
    vout, got = run_mul2(field, combo, items)
    vsum = types[0][1] * types[1][1] + types[2][1] * types[3][1]
    if kind == 2:
        assert vout == 2
    else:
        assert vout == 1 + -(-vsum * q // (1 << (LW * NL)))          # 1 + ceil((V1 V2 + V3 V4) q / R)
    for (a, b, c, d), r in zip(items, got):
        want = (value_of(a) * value_of(b) + value_of(c) * value_of(d)) * rinv % q
        assert value_of(r) % q == want
        assert all(v < (1 << 29) + 8 for v in r) and value_of(r) < vout * q


def b32(x):
    return x.to_bytes(32, "little")


def run_add(field, curve, affine, neg, need_t, P, z1, Qp, z2):
    l = lib(field)
    l.ha_add.argtypes = [ctypes.c_int] * 4 + [ctypes.c_char_p] * 4 + [ctypes.c_char_p]
    out = ctypes.create_string_buffer(64)
    rc = l.ha_add(curve, affine, neg, need_t, b32(P[0]) + b32(P[1]), b32(z1), b32(Qp[0]) + b32(Qp[1]), b32(z2), out)
    return rc, (int.from_bytes(out.raw[:32], "little"), int.from_bytes(out.raw[32:], "little"))


@pytest.mark.parametrize("name", sorted(CURVES))
def test_addition_laws_against_affine_addition(name):
    field, curve, params = CURVES[name]
    S = params()
    rnd = random.Random(name)
    G = (S.gx, S.gy)
    assert o.te_is_on_curve(S, G)
    P, Qp = o.te_mul(S, rnd.randrange(1, S.r), G), o.te_mul(S, rnd.randrange(1, S.r), G)
    ident = o.te_identity()
    cases = [(P, Qp), (Qp, P), (P, P), (P, o.te_neg(S, P)), (P, ident), (ident, P), (ident, ident), (G, G)]
    cases += [(o.te_mul(S, rnd.randrange(1, S.r), G), o.te_mul(S, rnd.randrange(1, S.r), G)) for _ in range(8)]
    for A, B in cases:
        for neg in (0, 1):
            want = o.te_add(S, A, o.te_neg(S, B) if neg else B)
            for affine, need_t in ((0, 0), (0, 1), (1, 1)):
                for z1, z2 in ((1, 1), (rnd.randrange(1, S.q), rnd.randrange(1, S.q))):
                    rc, got = run_add(field, curve, affine, neg, need_t, A, z1, B, z2)
                    assert rc == 1 and got == want, (name, A, B, neg, affine, need_t, z1, z2)
    # the unified law doubles, and P + (-P) is the identity
    assert run_add(field, curve, 0, 0, 1, P, 1, P, 1)[1] == o.te_mul(S, 2, P)
    assert run_add(field, curve, 0, 1, 1, P, 1, P, 1)[1] == ident
    assert run_add(field, curve, 1, 1, 1, P, 1, P, 1)[1] == ident
