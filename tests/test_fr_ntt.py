"""GPU: vrfhip_fr_domain_*, vrfhip_fr_ntt_batch*, vrfhip_kzg_commit_evals_batch*, vrfhip_kzg_open_evals_batch* -- radix-2
transforms over Fr of BLS12-381 on a resident domain, and KZG commitments and openings of polynomials given as evaluations --
against Python integers (tests/fr_ntt_ref.py: a recursive transform checked against direct evaluation) and, for points, the
native C oracle under the toy tau of tests/test_kzg_commit_open.py.  Every comparison is exact.

Sizes: every log_n in 0 .. 14, then the first size of every pass count vrfhip_test_fr_ntt_passes reports and the one before
it, and 2^20 once.  At 2^16 and 2^17 one of the three columns is random (recursive reference) and two are sparse (closed
form), which keeps a case to a few seconds; the kernels do the same work on either."""
import random

import numpy as np
import pytest

import fr_ntt_ref as ref
import test_kzg_commit_open as tk
from oracle import c_oracle as co

pytestmark = pytest.mark.gpu

R = ref.R
EDGE, NE = ref.EDGE_SCALARS, len(ref.EDGE_SCALARS)
MAX_LOG = 20
N_SRS = 2048
EVALS_SHAPES = [(1, 0), (1, 1), (3, 6), (2, 11)]


def arr(cols):
    return np.frombuffer(ref.to_bytes(cols), np.uint8).reshape(len(cols), len(cols[0]), 32).copy()


def ints(a):
    return ref.from_bytes(a.tobytes(), a.shape[0], a.shape[1])


@pytest.fixture(scope="module")
def ctx():
    from ark_ec_vrfs_amd import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pass_sizes(ctx):
    """the first log_n of every pass count up to 2^20, and the one before it"""
    assert ref.self_check()
    passes = [ctx.fr_ntt_passes(n) for n in range(MAX_LOG + 1)]
    assert passes[0] == 1 and passes[11] == 1 and passes[MAX_LOG] in (2, 3)          # 2^11 is one launch
    assert all(b - a in (0, 1) for a, b in zip(passes, passes[1:]))
    firsts = [n for n in range(1, MAX_LOG + 1) if passes[n] != passes[n - 1]]
    return sorted({n for f in firsts for n in (f - 1, f)})


def offset_for(log_n):
    return ref.GENERATOR if log_n % 2 else random.Random(9000 + log_n).randrange(2, R)


def columns(log_n):
    """three columns; up to 2^14 random, edge scalars, random; above: random and two sparse ones"""
    n = 1 << log_n
    rnd = random.Random(8000 + log_n)
    rand = lambda: [rnd.randrange(R) for _ in range(n)]
    if log_n <= 14:
        edge = [EDGE[j % NE] for j in range(n)]
        for q, p in enumerate(sorted({0, n - 1, n // 2, max(n // 2 - 1, 0), min(8, n - 1), min(2048, n - 1), min(2047, n - 1)})):
            edge[p] = (0, 1, R - 1)[q % 3]
        cols = [rand(), edge, rand()]
        return cols, lambda o: [ref.fft(c, o) for c in cols]
    t1 = [(0, rnd.randrange(1, R)), (n // 2 + 1, rnd.randrange(1, R)), (n - 1, R - 1)]
    t2 = [(1, 1), (n // 4 - 1, rnd.randrange(1, R)), (n - 2, rnd.randrange(1, R)), (n // 2, R - 1)]
    cols = [rand(), ref.sparse_column(t1, log_n), ref.sparse_column(t2, log_n)]
    return cols, lambda o: [ref.fft(cols[0], o), ref.sparse_evals(t1, log_n, o), ref.sparse_evals(t2, log_n, o)]


def check_size(ctx, log_n):
    import torch
    cols, want_of = columns(log_n)
    a = arr(cols)
    for offset in (None, offset_for(log_n)):
        dom = ctx.fr_domain_create(log_n, offset)
        assert dom.size() == 1 << log_n and dom.bytes() >= 36 << log_n
        want = arr(want_of(1 if offset is None else offset))
        for k in (1, 3):
            out, st = ctx.fr_ntt_batch(dom, a[:k])
            assert not st.any() and (out == want[:k]).all(), (log_n, offset, k, "forward")
            back, st = ctx.fr_ntt_batch(dom, want[:k], inverse=True)
            assert not st.any() and (back == a[:k]).all(), (log_n, offset, k, "inverse")
            t = torch.from_numpy(a[:k].copy()).cuda()                  # in place through the _dev form, and the round trip
            s = torch.full((k,), 0xEE, dtype=torch.uint8, device="cuda")
            ctx.fr_ntt_batch_dev(dom, t, t, s)
            torch.cuda.synchronize()
            assert not s.cpu().numpy().any() and (t.cpu().numpy() == want[:k]).all(), (log_n, offset, k, "in place")
            ctx.fr_ntt_batch_dev(dom, t, t, s, inverse=True)
            torch.cuda.synchronize()
            assert not s.cpu().numpy().any() and (t.cpu().numpy() == a[:k]).all(), (log_n, offset, k, "round trip")
        dom.close()


@pytest.mark.parametrize("log_n", range(15))
def test_every_size_up_to_2_14(ctx, log_n):
    check_size(ctx, log_n)


@pytest.mark.parametrize("which", range(4))
def test_the_sizes_where_the_pass_count_changes(ctx, pass_sizes, which):
    """the plan gives 11 | 12 and 16 | 17; whatever the device reports is what runs"""
    assert len(pass_sizes) <= 4 and max(pass_sizes) <= 17               # exact comparison is required up to 2^17
    if which < len(pass_sizes):
        check_size(ctx, pass_sizes[which])


def test_the_largest_size(ctx):
    log_n, n = MAX_LOG, 1 << MAX_LOG
    terms = [(0, 3), ((1 << 19) + 1, R - 2), (n - 1, 0x1234567890abcdef)]
    col = arr([ref.sparse_column(terms, log_n)])
    want = arr([ref.sparse_evals(terms, log_n)])
    dom = ctx.fr_domain_create(log_n)
    out, st = ctx.fr_ntt_batch(dom, col)
    assert not st.any() and (out == want).all()
    back, st = ctx.fr_ntt_batch(dom, out, inverse=True)
    assert not st.any() and (back == col).all()
    dom.close()


def test_both_coset_offsets_at_one_size(ctx):
    log_n = 9
    rnd = random.Random(31)
    cols = [[rnd.randrange(R) for _ in range(1 << log_n)] for _ in range(2)]
    for offset in (ref.GENERATOR, rnd.randrange(2, R), R - 1, 1):
        dom = ctx.fr_domain_create(log_n, offset)
        out, st = ctx.fr_ntt_batch(dom, arr(cols))
        assert not st.any() and ints(out) == [ref.fft(c, offset) for c in cols]
        back, _ = ctx.fr_ntt_batch(dom, out, inverse=True)
        assert ints(back) == cols
        dom.close()


def test_refusals(ctx):
    import torch
    from ark_ec_vrfs_amd import Context, Secp256r1Sha256Tai, VrfHipError
    for offset in (0, R, R + 7, (1 << 256) - 1):
        with pytest.raises(VrfHipError):
            ctx.fr_domain_create(4, offset)
    with pytest.raises(VrfHipError):
        ctx.fr_domain_create(MAX_LOG + 1)
    dom = ctx.fr_domain_create(4)
    other = Context(0)
    with pytest.raises(VrfHipError):
        other.fr_ntt_batch(dom, np.zeros((1, 16, 32), np.uint8))                   # a domain of another context
    other.close()
    t = torch.zeros((1, 16, 32), dtype=torch.uint8, device="cuda")
    s = torch.zeros((1,), dtype=torch.uint8, device="cuda")
    for flags in (2, 3, 0x80000000):
        with pytest.raises(VrfHipError):
            ctx.fr_ntt_batch_dev(dom, t, t, s, flags=flags)
    with pytest.raises(VrfHipError):
        ctx.fr_ntt_batch(dom, np.zeros((0, 16, 32), np.uint8))                     # k = 0
    dom.close()
    p256 = Context(0, Secp256r1Sha256Tai)
    with pytest.raises(VrfHipError) as e:
        p256.fr_domain_create(4)
    assert "secp256r1" in str(e.value)
    p256.close()


@pytest.mark.parametrize("log_n", [0, 3, 11, 12, 17])
def test_a_scalar_out_of_range_refuses_its_column_only(ctx, log_n):
    n = 1 << log_n
    rnd = random.Random(6000 + log_n)
    if log_n <= 14:
        p = [rnd.randrange(R) for _ in range(n)]
        want_f = lambda o: ref.fft(p, o)
    else:
        terms = [(0, rnd.randrange(1, R)), (n // 2, rnd.randrange(1, R)), (n - 1, rnd.randrange(1, R))]
        p = ref.sparse_column(terms, log_n)
        want_f = lambda o: ref.sparse_evals(terms, log_n, o)
    bad = lambda j, x: p[:j] + [x] + p[j + 1:]
    a = arr([p, bad(0, R), bad(n // 2, (1 << 256) - 1), bad(n - 1, R + 5), p])
    for offset in (None, offset_for(log_n)):
        dom = ctx.fr_domain_create(log_n, offset)
        want = arr([want_f(1 if offset is None else offset)])[0]
        out, st = ctx.fr_ntt_batch(dom, a)
        assert st.tolist() == [0, 2, 2, 2, 0]
        assert (out[0] == want).all() and (out[4] == want).all() and not out[1:4].any()
        out, st = ctx.fr_ntt_batch(dom, a, inverse=True)
        assert st.tolist() == [0, 2, 2, 2, 0] and (out[0] == out[4]).all() and not out[1:4].any()
        fwd, _ = ctx.fr_ntt_batch(dom, out[:1])
        assert (fwd[0] == a[0]).all()
        dom.close()


# ------------------------------------------------------------------------------------------------ from evaluations
@pytest.fixture(scope="module")
def srs(ctx):
    out, t = [], 1
    for _ in range(N_SRS):
        out.append(co.g1_mul(t, tk.G96))
        t = t * tk.TAU % R
    s = ctx.g1_srs_create(tk.as48(out))
    yield s
    s.close()


@pytest.fixture(scope="module")
def vk():
    return np.frombuffer(tk.G96 + tk.H192 + co.g2_mul(tk.TAU, tk.H192), np.uint8)


def evals_case(k, log_n):
    rnd = random.Random(700 + 31 * log_n + k)
    evals = [[rnd.randrange(R) for _ in range(1 << log_n)] for _ in range(k)]
    return evals, [ref.ifft(e) for e in evals]


@pytest.mark.parametrize("k,log_n", EVALS_SHAPES)
def test_commit_from_evaluations(ctx, srs, k, log_n):
    evals, coeffs = evals_case(k, log_n)
    dom = ctx.fr_domain_create(log_n)
    c48, cxy, st = ctx.kzg_commit_evals_batch(srs, dom, arr(evals))
    h48, hxy, hst = ctx.kzg_commit_batch(srs, arr(coeffs))
    assert not st.any() and not hst.any()
    assert (c48 == h48).all() and (cxy == hxy).all()
    for c in range(k):
        want = tk.mulG(tk.ev(coeffs[c], tk.TAU))
        assert cxy[c].tobytes() == want and c48[c].tobytes() == tk.compress(want), c
    dom.close()


@pytest.mark.parametrize("k,log_n", EVALS_SHAPES)
def test_open_from_evaluations(ctx, srs, vk, k, log_n):
    evals, coeffs = evals_case(k, log_n)
    n, w = 1 << log_n, ref.omega(log_n)
    rnd = random.Random(800 + log_n)
    dom = ctx.fr_domain_create(log_n)
    c48, _, st = ctx.kzg_commit_evals_batch(srs, dom, arr(evals))
    assert not st.any()
    idx = [rnd.randrange(n) for _ in range(k)]
    for kind, zs in (("random", [rnd.randrange(R) for _ in range(k)]), ("zero", [0] * k),
                     ("in the domain", [pow(w, i, R) for i in idx])):
        v, pr, pxy, st = ctx.kzg_open_evals_batch(srs, dom, arr(evals), tk.pts32(zs))
        assert not st.any(), kind
        hv, hpr, hpxy, _ = ctx.kzg_open_batch(srs, arr(coeffs), tk.pts32(zs))
        assert (v == hv).all() and (pr == hpr).all() and (pxy == hpxy).all(), kind
        for c in range(k):
            assert int.from_bytes(v[c].tobytes(), "little") == tk.ev(coeffs[c], zs[c]), (kind, c)
            if kind == "in the domain":
                assert int.from_bytes(v[c].tobytes(), "little") == evals[c][idx[c]], c
            if n > 1:
                assert pxy[c].tobytes() == tk.proof_of(coeffs[c], zs[c])[1], (kind, c)
        assert not ctx.kzg_check_batch(c48, tk.pts32(zs), v, pr, vk).any(), kind
    # one evaluation changed after committing: the opening of that polynomial no longer matches its commitment
    zs = [rnd.randrange(R) for _ in range(k)]
    changed = [list(e) for e in evals]
    j = k - 1
    changed[j][rnd.randrange(n)] = (changed[j][0] + 1 + rnd.randrange(R - 1)) % R if n == 1 else rnd.randrange(R)
    assert changed[j] != evals[j]
    v, pr, _, st = ctx.kzg_open_evals_batch(srs, dom, arr(changed), tk.pts32(zs))
    assert not st.any()
    assert ctx.kzg_check_batch(c48, tk.pts32(zs), v, pr, vk).tolist() == [0] * (k - 1) + [1]
    dom.close()


def test_evaluations_out_of_range_and_refusals(ctx, srs):
    from ark_ec_vrfs_amd import Context, VrfHipError
    log_n, n = 6, 64
    evals, coeffs = evals_case(3, log_n)
    bad = [list(e) for e in evals]
    bad[1][n - 1] = R
    dom = ctx.fr_domain_create(log_n)
    c48, cxy, st = ctx.kzg_commit_evals_batch(srs, dom, arr(bad))
    g48, gxy, _ = ctx.kzg_commit_evals_batch(srs, dom, arr(evals))
    assert st.tolist() == [0, 2, 0] and not c48[1].any() and not cxy[1].any()
    assert (c48[[0, 2]] == g48[[0, 2]]).all() and (cxy[[0, 2]] == gxy[[0, 2]]).all()
    zs = tk.pts32([5, 6, 7])
    v, pr, pxy, st = ctx.kzg_open_evals_batch(srs, dom, arr(bad), zs)
    gv, gpr, gpxy, _ = ctx.kzg_open_evals_batch(srs, dom, arr(evals), zs)
    assert st.tolist() == [0, 2, 0] and not v[1].any() and not pr[1].any() and not pxy[1].any()
    assert (v[[0, 2]] == gv[[0, 2]]).all() and (pr[[0, 2]] == gpr[[0, 2]]).all()
    v, pr, pxy, st = ctx.kzg_open_evals_batch(srs, dom, arr(evals), tk.pts32([5, R, 7]))            # z >= r
    assert st.tolist() == [0, 2, 0] and not v[1].any() and not pr[1].any()
    dom.close()
    big = ctx.fr_domain_create(12)                                                   # larger than the base set
    with pytest.raises(VrfHipError):
        ctx.kzg_commit_evals_batch(srs, big, np.zeros((1, 4096, 32), np.uint8))
    with pytest.raises(VrfHipError):
        ctx.kzg_open_evals_batch(srs, big, np.zeros((1, 4096, 32), np.uint8), tk.pts32([1]))
    big.close()
    other = Context(0)
    odom = other.fr_domain_create(log_n)
    with pytest.raises(VrfHipError):
        ctx.kzg_commit_evals_batch(srs, odom, arr(evals))                            # a domain of another context
    odom.close()
    other.close()


def test_dev_forms_chain_on_one_stream(ctx, srs, vk):
    import torch
    k, log_n = 2, 11
    evals, coeffs = evals_case(k, log_n)
    zs = [3, pow(ref.omega(log_n), 5, R)]
    dom = ctx.fr_domain_create(log_n)
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()
    u8 = lambda *s: torch.full(s, 0xEE, dtype=torch.uint8, device="cuda")
    d_ev, d_z, d_vk = dev(arr(evals)), dev(tk.pts32(zs)), dev(vk.copy())
    c48, cxy, cst, val, p48, p96, pst, chk = u8(k, 48), u8(k, 96), u8(k), u8(k, 32), u8(k, 48), u8(k, 96), u8(k), u8(k)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ctx.kzg_commit_evals_batch_dev(srs, dom, d_ev, c48, cst, out_xy=cxy)
        ctx.kzg_open_evals_batch_dev(srs, dom, d_ev, d_z, val, p48, pst, proof_xy=p96)
        ctx.kzg_check_batch_dev(c48, d_z, val, p48, d_vk, chk)
    stream.synchronize()
    h48, hxy, _ = ctx.kzg_commit_batch(srs, arr(coeffs))
    hv, hpr, hpxy, _ = ctx.kzg_open_batch(srs, arr(coeffs), tk.pts32(zs))
    assert (c48.cpu().numpy() == h48).all() and (cxy.cpu().numpy() == hxy).all() and not cst.cpu().numpy().any()
    assert (val.cpu().numpy() == hv).all() and (p48.cpu().numpy() == hpr).all() and (p96.cpu().numpy() == hpxy).all()
    assert not pst.cpu().numpy().any() and not chk.cpu().numpy().any()
    assert (d_ev.cpu().numpy() == arr(evals)).all()                                  # the caller's evaluations are untouched
    assert int.from_bytes(val[1].cpu().numpy().tobytes(), "little") == evals[1][5]
    dom.close()
