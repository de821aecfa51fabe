"""CPU: the cases of tests/verify_uv_cases.py through the host build of the verification ladders (tests/hostsim:
hs_verify_uv, hj_verify_uv, hx_verify_uv, hp_verify_uv, hb_verify_uv -- verify_straus_item<S, 0 / 1> and the secp256r1
counterparts on tables built the way the decode stage builds them), byte for byte against the oracles' integer arithmetic.

This pins the recodings and the window logic -- challenge_top_window, the carries of the signed digits, the GLV split --
for anyone without a card, and makes a failure of tests/test_gpu_verify_uv.py readable: logic fails in both builds, code
generation on the device only.  It does not stand in for the GPU test: the host build has neither the chained field products
(fe.cuh mac<true> under __HIP_DEVICE_COMPILE__) nor the 16-bit fixed-base comb (VRF_GCOMB_BITS=8 here)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import verify_uv_cases as vc

HS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim")
# suite -> (library, entry point, setter of the decode stage's subgroup-test mask or None when the call takes it)
HOST = {"bandersnatch": ("libhostsim.so", "hs_verify_uv", "hs_set_check_mask"),
        "jubjub": ("libhostsim_jj.so", "hj_verify_uv", "hj_set_check_mask"),
        "ed25519": ("libhostsim_f1.so", "hx_verify_uv", "hx_set_check_mask"),
        "baby_jubjub": ("libhostsim_f2.so", "hx_verify_uv", "hx_set_check_mask"),
        "secp256r1": ("libhostsim_p256.so", "hp_verify_uv", None),
        "bandersnatch_sw": ("libhostsim_bsw.so", "hb_verify_uv", None)}
CHK_ALL = 7                                  # pk, H, Gamma: what a default context tests


def _run(suite, cs):
    libname, fn, setter = HOST[suite]
    subprocess.run(["make", "-C", HS, "-j4", libname], check=True, stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(os.path.join(HS, libname))
    f = getattr(lib, fn)
    pw = cs.pk.shape[1]
    u, v, st = np.zeros((cs.n, pw), np.uint8), np.zeros((cs.n, pw), np.uint8), np.zeros(cs.n, np.uint8)
    ub, vb = ctypes.create_string_buffer(pw), ctypes.create_string_buffer(pw)
    if setter:
        getattr(lib, setter)(CHK_ALL)
    try:
        for i in range(cs.n):
            args = [cs.pk[i].tobytes(), cs.input[i].tobytes(), cs.output[i].tobytes(), cs.c[i].tobytes(), cs.s[i].tobytes(), ub, vb]
            st[i] = f(cs.L, CHK_ALL, *args) if suite == "bandersnatch_sw" else f(cs.L, *args)
            u[i], v[i] = np.frombuffer(ub.raw, np.uint8), np.frombuffer(vb.raw, np.uint8)
    finally:
        if setter:
            getattr(lib, setter)(0)          # the libraries are shared with the other host-simulation tests of this process
    bad = np.flatnonzero((st != cs.status) | (u != cs.u).any(axis=1) | (v != cs.v).any(axis=1))
    assert bad.size == 0, "%s L=%d: %d cases differ: %s" % (suite, cs.L, bad.size, [(cs.tags[i], int(st[i])) for i in bad[:12]])


@pytest.mark.parametrize("suite", vc.SUITES)
def test_host_ladders_on_the_whole_set(suite):
    _run(suite, vc.cases(suite))


@pytest.mark.parametrize("suite,L", [(s, L) for s, ls in vc.EXTRA_L.items() for L in ls])
def test_host_ladders_at_other_challenge_lengths(suite, L):
    _run(suite, vc.cases(suite, L))


def test_glv_model_is_the_device_split():
    """glv_decompose of the generator against fr.cuh glv_decompose_bs on every kept scalar, and the figures the issue asks
    the generator to reach"""
    subprocess.run(["make", "-C", HS, "-j4", "libhostsim.so"], check=True, stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(os.path.join(HS, "libhostsim.so"))
    out = ctypes.create_string_buffer(34)
    for tag, k in vc.glv_scalars():
        lib.hs_glv_decompose(k.to_bytes(32, "little"), out)
        k1 = int.from_bytes(out.raw[:16], "little") * (-1 if out.raw[16] else 1)
        k2 = int.from_bytes(out.raw[17:33], "little") * (-1 if out.raw[33] else 1)
        assert (k1, k2) == vc.glv_decompose(k), tag
    assert vc.glv_max_log2() >= vc.GLV_FLOOR_LOG2
