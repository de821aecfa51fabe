"""GPU: the BLS12-381 G1 codec through the C ABI (vrfhip_g1_decode_batch / _validate_batch / _encode_batch, host and _dev
forms) against a decoder of a few lines of Python ints (subgroup membership by r P = O): batches that mix every class of
input at positions straddling the 64-lane and 128-lane boundaries, the subgroup test on and off on torsion shifts, n = 0, and
the chain decode -> pairing check on one stream, where a torsion-shifted point must come out as InvalidData."""
import json
import os
import random

import numpy as np
import pytest

from oracle import bls_oracle as bls

P, R, X_ABS = bls.P, bls.R, bls.X_ABS
HERE = os.path.dirname(os.path.abspath(__file__))
ORDER = P + X_ABS                       # #E(Fp)
ELLS = (3, 11, 10177, 859267, 52437899)  # the primes dividing the cofactor
BAD96 = b"\xff" * 96
SIZES = (1, 64, 65, 129, 333)
_memo = {}


def py_decode(b, check_subgroup=True):
    """(status, 96 bytes) from the format's definition; memoised (r P costs a scalar multiplication in Python)."""
    key = (bytes(b), check_subgroup)
    if key not in _memo:
        _memo[key] = _py_decode(*key)
    return _memo[key]


def _py_decode(b, check_subgroup):
    comp, inf, srt = b[0] >> 7 & 1, b[0] >> 6 & 1, b[0] >> 5 & 1
    x = int.from_bytes(bytes([b[0] & 0x1F]) + b[1:], "big")
    if not comp:
        return 2, BAD96
    if inf:
        return (0, bytes(96)) if not srt and x == 0 else (2, BAD96)
    if x >= P:
        return 2, BAD96
    a = (x ** 3 + 4) % P
    y = pow(a, (P + 1) // 4, P)
    if y * y % P != a:
        return 2, BAD96
    if (y > P - y) != bool(srt):
        y = (P - y) % P
    if check_subgroup and bls.g1_mul(R, (x, y)) is not None:
        return 2, BAD96
    return 0, xy96((x, y))


def py_encode(pt):
    if pt is None:
        return bytes([0xC0]) + bytes(47)
    b = bytearray(pt[0].to_bytes(48, "big"))
    b[0] |= 0x80 | (0x20 if pt[1] > P - pt[1] else 0)
    return bytes(b)


def xy96(pt):
    return bytes(96) if pt is None else pt[0].to_bytes(48, "little") + pt[1].to_bytes(48, "little")


def from_xy96(b):
    return None if not any(b) else (int.from_bytes(b[:48], "little"), int.from_bytes(b[48:], "little"))


def curve_point(rnd):
    while True:
        x = rnd.randrange(P)
        a = (x ** 3 + 4) % P
        y = pow(a, (P + 1) // 4, P)
        if y * y % P == a:
            return (x, y if rnd.getrandbits(1) else (P - y) % P)


def torsion_point(ell, rnd):
    """A point of exact order ell (prime, dividing the cofactor): the ell-part of a random curve point, multiplied by ell
    until one more step would give infinity.  ((#E / ell) Q alone is always infinity where ell^2 | #E and the ell-part of the
    group is not cyclic.)"""
    m = ORDER
    while m % ell == 0:
        m //= ell
    while True:
        T = bls.g1_mul(m, curve_point(rnd))
        if T is None:
            continue
        while bls.g1_mul(ell, T) is not None:
            T = bls.g1_mul(ell, T)
        return T


@pytest.fixture(scope="module")
def pool():
    """Encodings by class, computed once: 'valid' (subgroup points, both sort flags, infinity, the golden file), 'torsion'
    (on the curve, outside the subgroup: T and G + T for every prime l | h, the order-3 point x = 0) and 'malformed'."""
    rnd = random.Random(12381)
    golden = json.load(open(os.path.join(HERE, "golden", "bls12_381_g1_compressed.json")))["vectors"]
    valid = [bytes.fromhex(v["compressed"]) for v in golden]
    acc = bls.g1_mul(rnd.randrange(1, R), bls.G1)
    for _ in range(6):
        acc = bls.g1_add(acc, bls.G1)
        valid += [py_encode(acc), py_encode(bls.g1_neg(acc))]
    torsion = [bytes([0x80]) + bytes(47), bytes([0xA0]) + bytes(47)]
    for ell in ELLS:
        T = torsion_point(ell, rnd)
        torsion += [py_encode(T), py_encode(bls.g1_add(bls.G1, T))]
    g = py_encode(bls.G1)
    raw = lambda x, flags: bytes([flags | (x >> 376)]) + (x & ((1 << 376) - 1)).to_bytes(47, "big")
    nsq = next(x for x in iter(lambda: rnd.randrange(P), None) if pow((x ** 3 + 4) % P, (P - 1) // 2, P) == P - 1)
    malformed = [bytes([g[0] & 0x7F]) + g[1:], bytes([0xE0]) + bytes(47), bytes([0xC0]) + bytes(46) + b"\x01",
                 raw(P, 0x80), raw(P + 1, 0xA0), raw((1 << 381) - 1, 0x80), raw(nsq, 0x80), raw(nsq, 0xA0)]
    assert all(py_decode(e)[0] == 0 for e in valid)
    assert all(py_decode(e)[0] == 2 and py_decode(e, False)[0] == 0 for e in torsion)
    assert all(py_decode(e, on)[0] == 2 for e in malformed for on in (True, False))
    return dict(valid=valid, torsion=torsion, malformed=malformed)


def mixed_batch(pool, n):
    """n encodings cycling through the classes, with the class changing across every 64- and 128-lane boundary."""
    rnd = random.Random(n)
    kinds = ("valid", "torsion", "malformed")
    encs = [rnd.choice(pool[kinds[i % 3]]) for i in range(n)]
    for pos, kind in ((0, "torsion"), (63, "malformed"), (64, "valid"), (127, "torsion"), (128, "valid"), (n - 1, "malformed")):
        if 0 <= pos < n:
            encs[pos] = rnd.choice(pool[kind])
    return encs


def as_u8(items, w):
    return np.frombuffer(b"".join(items), np.uint8).reshape(-1, w).copy()


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_gpu_decode_host_and_dev_forms_equal_the_python_decoder(ctx, pool, n):
    import torch
    encs = mixed_batch(pool, n)
    arr = as_u8(encs, 48)
    for on in (True, False):
        want = [py_decode(e, on) for e in encs]
        xy, st = ctx.g1_decode_batch(arr, check_subgroup=on)
        assert [(int(st[i]), xy[i].tobytes()) for i in range(n)] == want, on
        d_in = torch.from_numpy(arr).cuda()
        d_xy = torch.full((n, 96), 0x5A, dtype=torch.uint8, device="cuda")
        d_st = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")
        ctx.g1_decode_batch_dev(d_in, d_xy, d_st, check_subgroup=on)
        torch.cuda.synchronize()
        assert [(int(s), bytes(x)) for s, x in zip(d_st.cpu().numpy(), d_xy.cpu().numpy())] == want, on
    if n > 1:
        assert {w[0] for w in want} == {0, 2}


@pytest.mark.gpu
def test_gpu_subgroup_flag_on_torsion_shifts(ctx, pool):
    arr = as_u8(pool["torsion"], 48)
    xy1, st1 = ctx.g1_decode_batch(arr, check_subgroup=True)
    xy0, st0 = ctx.g1_decode_batch(arr, check_subgroup=False)
    assert (st1 == 2).all() and (xy1 == 0xFF).all() and (st0 == 0).all()
    assert [x.tobytes() for x in xy0] == [py_decode(e, False)[1] for e in pool["torsion"]]
    # the same points in affine form: the curve test alone passes them (encode), the subgroup test does not (validate)
    assert (ctx.g1_validate_batch(xy0) == 2).all()
    enc, st = ctx.g1_encode_batch(xy0)
    assert (st == 0).all() and [e.tobytes() for e in enc] == pool["torsion"]


@pytest.mark.gpu
@pytest.mark.parametrize("n", (1, 129))
def test_gpu_validate_and_encode(ctx, pool, n):
    import torch
    encs = mixed_batch(pool, n)
    pts = [py_decode(e, False) for e in encs]              # malformed items become the 0xFF marker
    xy = as_u8([b for _, b in pts], 96)
    want_val = [py_decode(e, True)[0] for e in encs]
    want_enc = [(0, e if any(b) else py_encode(None)) if s == 0 else (2, b"\xff" * 48) for e, (s, b) in zip(encs, pts)]
    assert list(ctx.g1_validate_batch(xy)) == want_val
    out, st = ctx.g1_encode_batch(xy)
    assert [(int(st[i]), out[i].tobytes()) for i in range(n)] == want_enc
    d_xy = torch.from_numpy(xy).cuda()
    d_st = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")
    d_out = torch.full((n, 48), 0x5A, dtype=torch.uint8, device="cuda")
    ctx.g1_validate_batch_dev(d_xy, d_st)
    torch.cuda.synchronize()
    assert list(d_st.cpu().numpy()) == want_val
    ctx.g1_encode_batch_dev(d_xy, d_out, d_st)
    torch.cuda.synchronize()
    assert [(int(s), bytes(o)) for s, o in zip(d_st.cpu().numpy(), d_out.cpu().numpy())] == want_enc
    # off the curve and out of range
    gx, gy = bls.G1
    bad = as_u8([xy96((gx, (gy + 1) % P)), P.to_bytes(48, "little") + gy.to_bytes(48, "little")], 96)
    assert list(ctx.g1_validate_batch(bad)) == [2, 2]
    out, st = ctx.g1_encode_batch(bad)
    assert list(st) == [2, 2] and (out == 0xFF).all()


@pytest.mark.gpu
def test_gpu_empty_batch_and_null_arrays(ctx):
    from ark_ec_vrfs_amd import VrfHipError, _lib
    xy, st = ctx.g1_decode_batch(np.empty((0, 48), np.uint8))
    assert xy.shape == (0, 96) and st.shape == (0,)
    assert ctx.g1_validate_batch(np.empty((0, 96), np.uint8)).shape == (0,)
    out, st = ctx.g1_encode_batch(np.empty((0, 96), np.uint8))
    assert out.shape == (0, 48) and st.shape == (0,)
    lib, h = _lib.load(), ctx._h
    assert lib.vrfhip_g1_decode_batch_dev(h, 0, None, 1, None, None, None) == 0
    assert lib.vrfhip_g1_validate_batch_dev(h, 0, None, None, None) == 0
    assert lib.vrfhip_g1_encode_batch_dev(h, 0, None, None, None, None) == 0
    one = np.zeros(96, np.uint8)
    p = one.ctypes.data
    assert lib.vrfhip_g1_decode_batch(h, 1, None, 1, p, p) == -1 and lib.vrfhip_g1_decode_batch(h, 1, p, 1, None, p) == -1
    assert lib.vrfhip_g1_validate_batch(h, 1, p, None) == -1 and lib.vrfhip_g1_encode_batch(h, 1, p, None, p) == -1
    assert lib.vrfhip_g1_decode_batch_dev(h, 1, p, 1, p, None, None) == -1
    assert VrfHipError is not None


@pytest.mark.gpu
def test_gpu_decode_chained_into_the_pairing_check_names_the_torsion_shift(ctx):
    """Compressed G1 items -> decode on the device -> pairing check on the same stream.  An item whose first point is shifted
    by a point of order 11 passes the pairing call when given uncompressed (the gap: the pairing of a torsion point against G2
    is one); decoded with the subgroup test it reaches the pairing call as 0xFF bytes and comes out as InvalidData."""
    import torch
    fx = json.load(open(os.path.join(HERE, "golden", "pairing_items.json")))
    hxb = lambda h: bytes.fromhex(h)
    items = [hxb(h) for h in fx["shared"][:4]] + [hxb(h) for h in fx["shared_bad"][:1]]
    T = torsion_point(11, random.Random(11))
    a = from_xy96(items[0][:96])
    shifted = xy96(bls.g1_add(a, T)) + items[0][96:]
    assert bls.g1_mul(R, from_xy96(shifted[:96])) is not None
    items.append(shifted)
    n = len(items)
    g1 = as_u8(items, 192)
    g2 = np.frombuffer(hxb(fx["shared_g2"]), np.uint8).copy()
    direct = ctx.pairing_check_batch(g1, g2, g2_shared=True)
    assert list(direct[:5]) == [0, 0, 0, 0, 1] and direct[5] != 2
    comp = as_u8([py_encode(from_xy96(it[96 * k:96 * k + 96])) for it in items for k in (0, 1)], 48)      # 2n points
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d_comp = torch.from_numpy(comp).cuda()
        d_g2 = torch.from_numpy(g2).cuda()
        d_xy = torch.zeros((2 * n, 96), dtype=torch.uint8, device="cuda")
        d_dst = torch.zeros((2 * n,), dtype=torch.uint8, device="cuda")
        d_st = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")
        ctx.g1_decode_batch_dev(d_comp, d_xy, d_dst, check_subgroup=True, stream=stream.cuda_stream)
        ctx.pairing_check_batch_dev(d_xy.view(n, 192), d_g2, d_st, g2_shared=True, stream=stream.cuda_stream)
    stream.synchronize()
    assert list(d_st.cpu().numpy()) == [0, 0, 0, 0, 1, 2]
    assert list(d_dst.cpu().numpy()) == [0] * 10 + [2, 0]
    assert bytes(d_xy.cpu().numpy()[:10].reshape(-1)) == b"".join(items[:5])
