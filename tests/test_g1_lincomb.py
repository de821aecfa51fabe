"""GPU: per-item linear combinations of BLS12-381 G1 points through the C ABI (vrfhip_g1_lincomb_batch, host and _dev
forms) against the native C oracle (oracle.c_oracle.g1_mul per term, g1_add per sum, memoised): every split of the terms
between an item's own and the shared bases, batch sizes that put the last item on either side of the 64- and 128-lane
boundaries, invalid terms at the first, a middle and the last position, the output stride, the chain lincomb -> pairing check
on one stream, a batch of more than one launch, and the argument rules."""
import json
import os
import random

import numpy as np
import pytest

from oracle import bls_oracle as bls
from oracle import c_oracle as co

P, R = bls.P, bls.R
HERE = os.path.dirname(os.path.abspath(__file__))
INF, BAD96 = bytes(96), b"\xff" * 96
SHAPES = ((1, 0), (0, 1), (3, 0), (5, 3), (12, 4), (16, 0), (0, 16))
SIZES = (1, 4, 5, 9, 33)
_mul, _sum = {}, {}


def xy96(pt):
    return INF if pt is None else pt[0].to_bytes(48, "little") + pt[1].to_bytes(48, "little")


def neg96(b):
    return b if b == INF else b[:48] + ((P - int.from_bytes(b[48:], "little")) % P).to_bytes(48, "little")


def le32(s):
    return s.to_bytes(32, "little")


def mul(s, b):
    if (s, b) not in _mul:
        _mul[(s, b)] = co.g1_mul(s, b)
    return _mul[(s, b)]


def lincomb(terms):
    """terms: a tuple of (scalar, base96) -> 96 bytes, by the oracle"""
    if terms not in _sum:
        acc = INF
        for s, b in terms:
            acc = co.g1_add(acc, mul(s, b))
        _sum[terms] = acc
    return _sum[terms]


@pytest.fixture(scope="module")
def pool():
    """24 bases from the oracle: 11 multiples of the generator, their negatives, the generator and infinity -- and the
    scalars the items draw from (few, so that the memo of (scalar, base) products stays small)."""
    rnd = random.Random(12381)
    g = xy96(bls.G1)
    pts = [co.g1_mul(rnd.randrange(1, R), g) for _ in range(11)]
    bases = pts + [neg96(p) for p in pts] + [g, INF]
    scalars = [0, 1, R - 1, (1 << 254) - 1] + [rnd.randrange(R) for _ in range(12)]
    return dict(bases=bases, scalars=scalars)


def make_batch(pool, n, k, m, seed=0):
    """(items, shared): items[i] = k own (scalar, base) terms + m scalars for the shared bases"""
    rnd = random.Random(1000 * n + 17 * k + m + seed)
    finite = pool["bases"][:-1]
    shared = [rnd.choice(pool["bases"] if j else finite) for j in range(m)]
    items = []
    for i in range(n):
        own = [(rnd.choice(pool["scalars"]), rnd.choice(pool["bases"])) for _ in range(k)]
        items.append((own, [rnd.choice(pool["scalars"]) for _ in range(m)]))
    return items, shared


def arrays(items, shared, k, m):
    n = len(items)
    u8 = lambda chunks, *shape: np.frombuffer(b"".join(chunks), np.uint8).reshape(*shape).copy()
    b = u8([t[1] for own, _ in items for t in own], n, k, 96) if k else None
    s = u8([le32(t[0]) for own, _ in items for t in own], n, k, 32) if k else None
    sb = u8(shared, m, 96) if m else None
    ss = u8([le32(x) for _, sh in items for x in sh], n, m, 32) if m else None
    return b, s, sb, ss


def want_of(items, shared, invalid=()):
    out = []
    for i, (own, sh) in enumerate(items):
        out.append((2, BAD96) if i in invalid else (0, lincomb(tuple(own) + tuple(zip(sh, shared)))))
    return out


def run_host(ctx, items, shared, k, m):
    out, st = ctx.g1_lincomb_batch(*arrays(items, shared, k, m))
    return [(int(st[i]), out[i].tobytes()) for i in range(len(items))]


def run_dev(ctx, items, shared, k, m):
    import torch
    n = len(items)
    t = [None if a is None else torch.from_numpy(a).cuda() for a in arrays(items, shared, k, m)]
    d_out = torch.full((n, 96), 0x5A, dtype=torch.uint8, device="cuda")
    d_st = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")
    ctx.g1_lincomb_batch_dev(*t, d_out, d_st)
    torch.cuda.synchronize()
    return [(int(s), bytes(o)) for s, o in zip(d_st.cpu().numpy(), d_out.cpu().numpy())]


@pytest.mark.gpu
@pytest.mark.parametrize("k,m", SHAPES)
def test_gpu_host_and_dev_forms_equal_the_oracle(ctx, pool, k, m):
    for n in SIZES:
        items, shared = make_batch(pool, n, k, m)
        want = want_of(items, shared)
        assert run_host(ctx, items, shared, k, m) == want, n
        assert run_dev(ctx, items, shared, k, m) == want, n


@pytest.mark.gpu
def test_gpu_sums_through_the_corners_of_the_addition_law(ctx, pool):
    """s P + (r - s) P = infinity (all-zero output), P and -P with one scalar, one base in every term, a base at infinity with
    a non-zero scalar, all scalars zero"""
    B, s = pool["bases"], pool["scalars"][5]
    items = [([(s, B[0]), (R - s, B[0]), (0, B[1])], []), ([(s, B[2]), (s, neg96(B[2])), (s, INF)], []),
             ([(s, B[3])] * 3, []), ([(s, INF), (R - 1, INF), (1, B[4])], []), ([(0, B[0]), (0, B[1]), (0, INF)], [])]
    want = want_of(items, [])
    assert [w[1] for w in want][:2] == [INF, INF] and want[4][1] == INF and want[3][1] == B[4]
    assert run_host(ctx, items, [], 3, 0) == want


@pytest.mark.gpu
@pytest.mark.parametrize("k,m", ((5, 3), (16, 0), (0, 16), (1, 0)))
def test_gpu_invalid_terms_mark_exactly_their_items(ctx, pool, k, m):
    gx, gy = bls.G1
    kinds = [("base", P.to_bytes(48, "little") + gy.to_bytes(48, "little")), ("base", xy96((gx, (gy + 1) % P))),
             ("scalar", R), ("scalar", (1 << 256) - 1)]
    n, t = 9, k + m
    positions = sorted({0, t // 2, t - 1})
    for pos in positions:
        for ki, (what, val) in enumerate(kinds):
            items, shared = make_batch(pool, n, k, m, seed=pos)
            targets = {0, 3, 4, n - 1}
            if pos >= k and what == "base":
                shared[pos - k] = val                      # an invalid shared base: every item
                targets = set(range(n))
            else:
                for i in targets:
                    own, sh = items[i]
                    if pos < k:
                        own[pos] = (val, own[pos][1]) if what == "scalar" else (own[pos][0], val)
                    else:
                        sh[pos - k] = val
            want = want_of(items, shared, invalid=targets)
            got = run_dev(ctx, items, shared, k, m) if ki % 2 else run_host(ctx, items, shared, k, m)
            assert got == want, (pos, what)


@pytest.mark.gpu
def test_gpu_out_stride(ctx, pool):
    import torch
    n, k, m = 9, 3, 2
    ia, sa = make_batch(pool, n, k, m, seed=1)
    ib, sb_ = make_batch(pool, n, k, m, seed=2)
    buf = torch.full((n, 192), 0x5A, dtype=torch.uint8, device="cuda")
    st = torch.full((2, n), 0x5A, dtype=torch.uint8, device="cuda")
    for half, (items, shared) in enumerate(((ia, sa), (ib, sb_))):
        t = [torch.from_numpy(a).cuda() for a in arrays(items, shared, k, m)]
        ctx.g1_lincomb_batch_dev(*t, buf.view(-1)[96 * half:], st[half], out_stride=192)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert [bytes(r[:96]) for r in got] == [w[1] for w in want_of(ia, sa)]
    assert [bytes(r[96:]) for r in got] == [w[1] for w in want_of(ib, sb_)]
    assert not st.cpu().numpy().any()
    # a third call into a wider slot leaves the sentinel between the results alone; so does stride 100
    for stride in (288, 100):
        wide = torch.full((n, stride), 0x5A, dtype=torch.uint8, device="cuda")
        t = [torch.from_numpy(a).cuda() for a in arrays(ia, sa, k, m)]
        ctx.g1_lincomb_batch_dev(*t, wide, st[0], out_stride=stride)
        torch.cuda.synchronize()
        w = wide.cpu().numpy()
        assert [bytes(r[:96]) for r in w] == [x[1] for x in want_of(ia, sa)] and (w[:, 96:] == 0x5A).all(), stride


@pytest.mark.gpu
def test_gpu_lincomb_chained_into_the_pairing_check(ctx):
    """Each half X of a pairing item is rebuilt on the device as u X'' + s P + (r - s) P with X'' = [1/u] X, straight into
    the n x 192 item array, and the pairing check follows on the same stream.  A sixth item with one scalar = r reaches the
    pairing call as 0xFF bytes."""
    import torch
    fx = json.load(open(os.path.join(HERE, "golden", "pairing_items.json")))
    items = [bytes.fromhex(h) for h in fx["shared"][:4]] + [bytes.fromhex(h) for h in fx["shared_bad"][:1]]
    items.append(items[0])
    n = len(items)
    g2 = np.frombuffer(bytes.fromhex(fx["shared_g2"]), np.uint8).copy()
    rnd = random.Random(192)
    Pt = co.g1_mul(rnd.randrange(1, R), xy96(bls.G1))
    halves = []
    for half in (0, 1):
        bases, scalars = [], []
        for i, it in enumerate(items):
            X = it[96 * half:96 * half + 96]
            u, s = rnd.randrange(1, R), rnd.randrange(1, R)
            X2 = co.g1_mul(pow(u, -1, R), X)
            assert co.g1_mul(u, X2) == X
            bases.append(X2 + Pt + Pt)
            scalars.append(le32(u) + le32(s) + le32(R if (i == 5 and half == 1) else R - s))
        halves.append((np.frombuffer(b"".join(bases), np.uint8).reshape(n, 3, 96).copy(),
                       np.frombuffer(b"".join(scalars), np.uint8).reshape(n, 3, 32).copy()))
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d_g2 = torch.from_numpy(g2).cuda()
        d_items = torch.full((n, 192), 0x5A, dtype=torch.uint8, device="cuda")
        d_lst = torch.full((2, n), 0x5A, dtype=torch.uint8, device="cuda")
        d_st = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")
        for half, (b, s) in enumerate(halves):
            ctx.g1_lincomb_batch_dev(torch.from_numpy(b).cuda(), torch.from_numpy(s).cuda(), None, None,
                                     d_items.view(-1)[96 * half:], d_lst[half], out_stride=192, stream=stream.cuda_stream)
        ctx.pairing_check_batch_dev(d_items, d_g2, d_st, g2_shared=True, stream=stream.cuda_stream)
    stream.synchronize()
    assert list(d_st.cpu().numpy()) == [0, 0, 0, 0, 1, 2]
    got = d_items.cpu().numpy()
    assert bytes(got[:5].reshape(-1)) == b"".join(items[:5])
    assert bytes(got[5]) == items[0][:96] + BAD96
    assert d_lst.cpu().numpy().tolist() == [[0] * 6, [0] * 5 + [2]]


@pytest.mark.gpu
def test_gpu_batch_of_more_than_one_launch(ctx, pool):
    import torch
    n = (1 << 20) + 3
    pairs = [(pool["scalars"][4 + j], pool["bases"][j]) for j in range(4)]
    b4 = torch.from_numpy(np.frombuffer(b"".join(b for _, b in pairs), np.uint8).reshape(4, 1, 96).copy()).cuda()
    s4 = torch.from_numpy(np.frombuffer(b"".join(le32(s) for s, _ in pairs), np.uint8).reshape(4, 1, 32).copy()).cuda()
    want4 = torch.from_numpy(np.frombuffer(b"".join(mul(s, b) for s, b in pairs), np.uint8).reshape(4, 96).copy()).cuda()
    reps = n // 4 + 1
    d_b, d_s = b4.repeat(reps, 1, 1)[:n].contiguous(), s4.repeat(reps, 1, 1)[:n].contiguous()
    d_out = torch.full((n, 96), 0x5A, dtype=torch.uint8, device="cuda")
    d_st = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")
    ctx.g1_lincomb_batch_dev(d_b, d_s, None, None, d_out, d_st)
    torch.cuda.synchronize()
    assert bool((d_st == 0).all())
    assert bool((d_out == want4.repeat(reps, 1)[:n]).all())


@pytest.mark.gpu
def test_gpu_empty_batch_and_bad_arguments(ctx):
    from ark_ec_vrfs_amd import _lib
    lib, h = _lib.load(), ctx._h
    err = lambda: lib.vrfhip_last_error().decode()
    assert lib.vrfhip_g1_lincomb_batch(h, 0, 3, None, None, 2, None, None, None, None) == 0
    assert lib.vrfhip_g1_lincomb_batch_dev(h, 0, 3, None, None, 2, None, None, None, 96, None, None) == 0
    buf = np.zeros(17 * 96, np.uint8)
    sc, out = np.zeros(17 * 32, np.uint8), np.full(96, 0x5A, np.uint8)
    st = np.full(1, 0x5A, np.uint8)
    p, q, o, s = buf.ctypes.data, sc.ctypes.data, out.ctypes.data, st.ctypes.data
    host = lib.vrfhip_g1_lincomb_batch
    dev = lambda *a: lib.vrfhip_g1_lincomb_batch_dev(h, *a, None)
    for k, m in ((0, 0), (17, 0), (0, 17), (9, 8), (16, 1)):
        assert host(h, 1, k, p, q, m, p, q, o, s) == -1 and "k + m" in err(), (k, m)
        assert dev(1, k, p, q, m, p, q, o, 96, s) == -1 and "k + m" in err(), (k, m)
    for stride in (92, 98, 0):
        assert dev(1, 1, p, q, 0, None, None, o, stride, s) == -1 and "out_stride" in err(), stride
    for args in ((1, None, q, 0, None, None, o, s), (1, p, None, 0, None, None, o, s), (1, p, q, 1, None, q, o, s),
                 (1, p, q, 1, p, None, o, s), (1, p, q, 0, None, None, None, s), (1, p, q, 0, None, None, o, None)):
        assert host(h, 1, *args) == -1 and "NULL" in err(), args
        assert dev(1, *args[:7], 96, args[7]) == -1 and "NULL" in err(), args
    assert (out == 0x5A).all() and st[0] == 0x5A
    # a NULL array whose count is 0 is fine: infinity with scalar 0
    assert host(h, 1, 1, p, q, 0, None, None, o, s) == 0 and st[0] == 0 and not out.any()
    assert host(h, 1, 0, None, None, 1, p, q, o, s) == 0 and st[0] == 0 and not out.any()
