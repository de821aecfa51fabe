"""CPU: the cases of tests/pedersen_c_cases.py through the host build of the per-proof Pedersen verifier with the challenge
supplied (tests/hostsim: hs_ / hj_ / hx_pedersen_verify_c, hb_pedersen_verify_c, hp_ped_verify_c -- the decode items, the
override the device's set_c kernels apply, pedersen_verify_straus_item<S, 0 / 1> and pedersen_verify_finish_item, on secp256r1
p256_ped_verify_eq_h / _eq_g), status for status against the discrete-log algebra of the generator.

This pins the window logic of the Pedersen ladders -- straus4<S, 4> and <S, 2>, straus2 and win_mul from
challenge_top_window, the two comb walks, the 65th digit and 33rd comb row of secp256r1 -- and the finish stages for anyone
without a card, and makes a failure of tests/test_gpu_pedersen_c.py readable: logic fails in both builds, code generation and
the 16-bit combs on the device only (VRF_GCOMB_BITS=8 here, and fe.cuh mac<true> differs under __HIP_DEVICE_COMPILE__ only).
Building a set runs the generator's self-checks (pedersen_c_cases._check_literal and the assertions of _rows)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pedersen_c_cases as pc

HS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim")
# suite -> (library, entry point, setter of the decode stage's subgroup-test mask or None when the call takes it / has none)
HOST = {"bandersnatch": ("libhostsim.so", "hs_pedersen_verify_c", "hs_set_check_mask_prove"),
        "jubjub": ("libhostsim_jj.so", "hj_pedersen_verify_c", "hj_set_check_mask"),
        "ed25519": ("libhostsim_f1.so", "hx_pedersen_verify_c", "hx_set_check_mask"),
        "baby_jubjub": ("libhostsim_f2.so", "hx_pedersen_verify_c", "hx_set_check_mask"),
        "secp256r1": ("libhostsim_p256.so", "hp_ped_verify_c", None),
        "bandersnatch_sw": ("libhostsim_bsw.so", "hb_pedersen_verify_c", None)}
CHK_PED = 2 | 4 | 8                          # input, output, proof points: what a default context tests


def _run(suite, cs):
    libname, fn, setter = HOST[suite]
    subprocess.run(["make", "-C", HS, "-j4", libname], check=True, stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(os.path.join(HS, libname))
    f = getattr(lib, fn)
    if suite == "secp256r1":
        B = pc.blinding(suite).B
        lib.hp_set_blinding_base(B[0].to_bytes(32, "big") + B[1].to_bytes(32, "big"))
    st = np.zeros(cs.n, np.uint8)
    if setter:
        getattr(lib, setter)(CHK_PED)
    try:
        for i in range(cs.n):
            args = [x[i].tobytes() for x in cs.points() + (cs.c, cs.s, cs.sb)]
            st[i] = f(cs.L, CHK_PED, *args) if suite == "bandersnatch_sw" else f(cs.L, *args)
    finally:
        if setter:
            getattr(lib, setter)(0)          # the libraries are shared with the other host-simulation tests of this process
    bad = np.flatnonzero(st != cs.status)
    print("%s L=%d: %d rows, %d differ" % (suite, cs.L, cs.n, bad.size))
    assert bad.size == 0, "%s L=%d: %d rows differ, first: %s" % (
        suite, cs.L, bad.size, [(int(i), cs.tags[i], int(st[i]), int(cs.status[i])) for i in bad[:8]])


@pytest.mark.parametrize("suite", pc.SUITES)
def test_host_verifier_on_the_whole_set(suite):
    _run(suite, pc.cases(suite))


@pytest.mark.parametrize("suite,L", [(s, L) for s, ls in pc.EXTRA_L.items() for L in ls])
def test_host_verifier_at_other_challenge_lengths(suite, L):
    _run(suite, pc.cases(suite, L))


@pytest.mark.parametrize("suite", pc.SUITES)
def test_the_set_holds_what_it_must(suite):
    """every family and every disturbance is there, every accepting row has its rejecting twin, and the set stays small"""
    cs = pc.cases(suite)
    g = pc.group(suite)
    assert cs.n < pc.MAX_ROWS and cs.n_literal >= pc.N_LITERAL
    kinds = set(cs.kinds)
    assert kinds >= set(pc.DISTURBANCES) | {"accept", "invalid", "tie", "tie-c^1"}
    assert set(cs.families) >= {"s-edge", "sb-edge", "s+sb-edge", "c-edge", "self", "neutral", "rand", "tie", "invalid"} | (
        {"glv"} if g.glv else set())
    acc = [i for i, k in enumerate(cs.kinds) if k == "accept"]
    assert all(cs.status[i] == 0 and cs.status[i + 1] == 1 and cs.tags[i + 1].startswith(cs.tags[i] + "/") for i in acc)
    assert cs.kinds.count("tie") == cs.kinds.count("tie-c^1") == pc.N_TIE
    tags = set(cs.tags)
    want = {"s=c*y,sb!=0", "y=1", "y=r-1", "h=1", "o=h", "o=-h", "pk_com=B", "bad:s=r", "bad:sb=r", "bad:R"}
    if g.identity_on_wire:
        want |= {"Ok=O", "R=O,sb=0", "c=s=sb=0", "pk_com=O", "Gamma=O"}
    if g.cofactor > 1:
        want |= {"bad:Ok-cofactor"}
    if cs.L < 32:
        want |= {"bad:c=2^8L"}
    assert tags >= want, want - tags
