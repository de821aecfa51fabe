"""CPU: the Pedersen per-proof verifier over affine x || y points (pedersen_verify_decode_affine_item, vrf_core.cuh),
compiled for the host (tests/hostsim_affine) and chained through the device's Straus and finish item functions.  It must
give the statuses of the compressed decode on the same points: 0 on the golden vector and on oracle proofs, 1 with s or sb
tampered, 2 with a point off the curve, a coordinate equal to q or (subgroup test on) a small-order shift -- from canonical
and from Montgomery-256 coordinates alike."""
import ctypes
import os
import subprocess

import pytest

from oracle import vrf_oracle as o

S = o.BANDERSNATCH
Q = S.q
HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim_affine")
CHK_ALL = 2 | 4 | 8            # CHK_INPUT | CHK_OUTPUT | CHK_PROOF


@pytest.fixture(scope="module")
def hs():
    subprocess.run(["make", "-C", HERE, "libhostsim_affine.so"], check=True, stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(os.path.join(HERE, "libhostsim_affine.so"))
    lib.hpa_pedersen_verify_affine.restype = ctypes.c_uint32
    lib.hpa_pedersen_verify.restype = ctypes.c_uint32
    lib.hpa_init()
    return lib


def _xy(P, mont=False):
    x, y = P
    if mont:
        x, y = (x << 256) % Q, (y << 256) % Q
    return x.to_bytes(32, "little") + y.to_bytes(32, "little")


def _proofs(kat):
    """(H, Gamma, pk_com, R, Ok as points, s, sb, ad) of the golden Pedersen vector and of two oracle proofs."""
    out = []
    iv = next(v for v in kat["ietf"] if v["seed"] == kat["pedersen"][0]["seed"])
    p = kat["pedersen"][0]
    pts = [o.point_decode(S, bytes.fromhex(h)) for h in (iv["h"], iv["gamma"], p["pk_com"], p["r"], p["ok"])]
    out.append((pts, bytes.fromhex(p["s"]), bytes.fromhex(p["sb"]), bytes.fromhex(p["ad"])))
    for i in (3, 7):
        sk = o.secret_from_seed(S, o.synth_seed(i))
        H = o.data_to_point(S, o.synth_msg(i))
        ad = bytes(range(i * 11))
        gm, (pc, R, Ok, s, sb), _ = o.pedersen_prove(S, sk, H, ad)
        out.append(([H, gm, pc, R, Ok], o.scalar_encode(s), o.scalar_encode(sb), ad))
    return out


def _both(hs, pts, s, sb, ad, mont=False):
    """(affine status, compressed status) of one proof."""
    xy = b"".join(_xy(P, mont) for P in pts)
    st_a = hs.hpa_pedersen_verify_affine(xy, s, sb, ad, len(ad), int(mont))
    enc = b"".join(o.point_encode(S, P) for P in pts)
    st_c = hs.hpa_pedersen_verify(enc, s, sb, ad, len(ad))
    return st_a, st_c


def _small_order_point():
    """A point of order 2 or 4 on the curve (Bandersnatch has cofactor 4)."""
    for P in [(0, Q - 1)]:
        if o.te_is_on_curve(S, P):
            return P
    raise AssertionError("no small-order point")


@pytest.mark.parametrize("mont", [False, True])
def test_affine_decode_accepts_valid_and_rejects_tampered(hs, kat, mont):
    hs.hpa_set_check_mask(CHK_ALL)
    for pts, s, sb, ad in _proofs(kat):
        assert _both(hs, pts, s, sb, ad, mont) == (0, 0)
        for which in ("s", "sb"):
            bad = bytearray(s if which == "s" else sb)
            bad[0] ^= 1
            args = (bytes(bad), sb) if which == "s" else (s, bytes(bad))
            assert _both(hs, pts, *args, ad, mont) == (1, 1), which
        # Gamma and Ok swapped: still valid points, the equations fail
        sw = [pts[0], pts[4], pts[2], pts[3], pts[1]]
        assert _both(hs, sw, s, sb, ad, mont) == (1, 1)


@pytest.mark.parametrize("mont", [False, True])
def test_affine_decode_rejects_points_without_a_compressed_form(hs, kat, mont):
    hs.hpa_set_check_mask(CHK_ALL)
    pts, s, sb, ad = _proofs(kat)[0]
    for p in range(5):
        x, y = pts[p]
        for bad in ((x, (y + 1) % Q), ((x + 1) % Q, y)):           # nudged off the curve
            assert not o.te_is_on_curve(S, bad)
            xy = bytearray(b"".join(_xy(P, mont) for P in pts))
            xy[64 * p:64 * p + 64] = _xy(bad, mont)
            assert hs.hpa_pedersen_verify_affine(bytes(xy), s, sb, ad, len(ad), int(mont)) == 2, (p, bad)
        # a coordinate equal to q (as raw integer: no canonical or Montgomery value is >= q)
        for half in (0, 1):
            xy = bytearray(b"".join(_xy(P, mont) for P in pts))
            xy[64 * p + 32 * half:64 * p + 32 * half + 32] = Q.to_bytes(32, "little")
            assert hs.hpa_pedersen_verify_affine(bytes(xy), s, sb, ad, len(ad), int(mont)) == 2, (p, half)


@pytest.mark.parametrize("mont", [False, True])
def test_affine_decode_subgroup_test_follows_the_check_mask(hs, kat, mont):
    pts, s, sb, ad = _proofs(kat)[1]
    T = _small_order_point()
    for p in range(5):
        shifted = list(pts)
        shifted[p] = o.te_add(S, pts[p], T)
        hs.hpa_set_check_mask(CHK_ALL)
        assert _both(hs, shifted, s, sb, ad, mont) == (2, 2), p
        hs.hpa_set_check_mask(0)                  # PREVALIDATED_ALL: the proof is then just wrong
        assert _both(hs, shifted, s, sb, ad, mont) == (1, 1), p
    hs.hpa_set_check_mask(0)
    assert _both(hs, pts, s, sb, ad, mont) == (0, 0)
    hs.hpa_set_check_mask(CHK_ALL)
