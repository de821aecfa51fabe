"""GPU (-m gpu): chunk invariance of the host-pointer API on every backend of the C ABI layer.

A context with `reserve(64)` cuts a batch of 150 into chunks of 64, 64 and 22; every chunk after the first reads its
slice of each array, of the message offsets and of the per-item ad offsets at `base`.  Variable-length messages (lengths
i % 7, empty ones included) and ad both shared and per item (lengths i % 5) put that arithmetic across a chunk boundary
for the Edwards, bandersnatch_sw and secp256r1 paths: every output byte must equal the unchunked context's, and the
statuses must name exactly the tampered items."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, CHUNK = 150, 64
BACKENDS = ("bandersnatch", "bandersnatch_sw", "secp256r1")


def _make(backend):
    from ark_ec_vrfs_amd import BandersnatchSwSha512Tai, Context, Secp256r1Sha256Tai
    if backend == "bandersnatch":
        return Context(0)
    if backend == "bandersnatch_sw":
        return Context(0, BandersnatchSwSha512Tai, test_blinding_base=True)
    return Context(0, Secp256r1Sha256Tai, test_blinding_base=True)


@pytest.fixture(scope="module", params=BACKENDS)
def pair(request):
    """(unchunked, chunked) contexts of one backend and the batch's secret keys."""
    big, small = _make(request.param), _make(request.param)
    small.reserve(CHUNK)
    seeds = np.array([[(17 * i + 3 * j + 1) & 0xff for j in range(32)] for i in range(N)], dtype=np.uint8)
    sk, _ = big.secret_from_seed_batch(seeds)
    yield big, small, sk
    small.close()
    big.close()


def _same(a, b, what):
    if isinstance(a, dict):
        assert a.keys() == b.keys(), what
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), (what, k)
    else:
        assert a.tobytes() == b.tobytes(), what


def _both(pair, what, call):
    """call(ctx) on the unchunked and on the chunked context: byte-equal outputs; returns the unchunked one's."""
    big, small, _ = pair
    ref, got = call(big), call(small)
    if isinstance(ref, tuple):
        for i, (r, g) in enumerate(zip(ref, got)):
            if isinstance(r, np.ndarray):
                _same(r, g, (what, i))
            else:
                assert r == g, (what, i)
    else:
        _same(ref, got, what)
    return ref


def _exactly(status, bad, what):
    want = np.zeros(N, dtype=bool)
    want[bad] = True
    assert ((status != 0) == want).all(), (what, np.nonzero(status)[0].tolist())


@pytest.mark.parametrize("ad_kind", ["shared", "per_item"])
def test_chunked_equals_unchunked(pair, ad_kind):
    big, small, sk = pair
    msgs = [bytes((i + 31 * k) & 0xff for k in range(i % 7)) for i in range(N)]
    ad = b"chunk-matrix" if ad_kind == "shared" else [bytes((3 * i + k) & 0xff for k in range(i % 5)) for i in range(N)]
    tampered = np.arange(0, N, 9)

    # IETF: prove, verify (valid and tampered), verify from alpha, verify from x || y
    pr = _both(pair, "ietf_prove", lambda c: c.ietf_prove_batch(sk, msgs=msgs, ad=ad))
    assert not pr["status"].any()
    assert 0 < small.workspace_bytes() < big.workspace_bytes()        # the chunked context did work in chunks
    proof = (pr["pk"], pr["input"], pr["output"], pr["c"], pr["s"])
    _exactly(_both(pair, "ietf_verify", lambda c: c.ietf_verify_batch(*proof, ad=ad)), [], "ietf_verify")
    s_bad = pr["s"].copy()
    s_bad[tampered, 0] ^= 1
    _exactly(_both(pair, "ietf_verify tampered",
                   lambda c: c.ietf_verify_batch(pr["pk"], pr["input"], pr["output"], pr["c"], s_bad, ad=ad)),
             tampered, "ietf_verify tampered")
    _exactly(_both(pair, "ietf_verify_alpha",
                   lambda c: c.ietf_verify_batch_alpha(pr["pk"], msgs, pr["output"], pr["c"], pr["s"], ad=ad)),
             [], "ietf_verify_alpha")
    _exactly(_both(pair, "ietf_verify_alpha tampered",
                   lambda c: c.ietf_verify_batch_alpha(pr["pk"], msgs, pr["output"], pr["c"], s_bad, ad=ad)),
             tampered, "ietf_verify_alpha tampered")
    xy = []
    for k in ("pk", "input", "output"):
        st, pts = _both(pair, "point_validate " + k, lambda c: c.point_validate_batch(pr[k], want_xy=True))
        assert not st.any(), k
        xy.append(pts)
    _exactly(_both(pair, "ietf_verify_affine", lambda c: c.ietf_verify_batch_affine(*xy, pr["c"], pr["s"], ad=ad)),
             [], "ietf_verify_affine")
    _exactly(_both(pair, "ietf_verify_affine tampered", lambda c: c.ietf_verify_batch_affine(*xy, pr["c"], s_bad, ad=ad)),
             tampered, "ietf_verify_affine tampered")

    # keyed: four keys; the key of item i changes with the chunk, so an index read at the wrong base names a wrong key
    idx = np.array([(7 * i + i // CHUNK) % 4 for i in range(N)], dtype=np.uint32)
    kp = big.ietf_prove_batch(sk[idx], msgs=msgs, ad=ad)
    ks_bad = kp["s"].copy()
    ks_bad[tampered, 0] ^= 1
    sets = {}
    try:
        for c in (big, small):
            sets[c], kst = c.keyset_create(pr["pk"][:4])
            assert not kst.any()
        _exactly(_both(pair, "ietf_verify_keyed",
                       lambda c: c.ietf_verify_batch_keyed(sets[c], idx, kp["input"], kp["output"], kp["c"], kp["s"], ad=ad)),
                 [], "ietf_verify_keyed")
        _exactly(_both(pair, "ietf_verify_keyed tampered",
                       lambda c: c.ietf_verify_batch_keyed(sets[c], idx, kp["input"], kp["output"], kp["c"], ks_bad, ad=ad)),
                 tampered, "ietf_verify_keyed tampered")
    finally:
        for s in sets.values():
            s.close()

    # Pedersen: prove, verify per proof, verify as one batch (random linear combination)
    pp = _both(pair, "pedersen_prove", lambda c: c.pedersen_prove_batch(sk, msgs=msgs, ad=ad))
    assert not pp["status"].any()
    ped = [pp[k] for k in ("input", "output", "pk_com", "r", "ok", "s", "sb")]
    _exactly(_both(pair, "pedersen_verify", lambda c: c.pedersen_verify_batch(*ped, ad=ad)), [], "pedersen_verify")
    sb_bad = pp["s"].copy()
    sb_bad[tampered, 0] ^= 1
    ped_bad = ped[:5] + [sb_bad, ped[6]]
    _exactly(_both(pair, "pedersen_verify tampered", lambda c: c.pedersen_verify_batch(*ped_bad, ad=ad)),
             tampered, "pedersen_verify tampered")
    seed = bytes(range(32))
    st, batch_ok = _both(pair, "pedersen_verify_rlc", lambda c: c.pedersen_verify_batch_rlc(*ped, ad=ad, seed=seed))
    assert batch_ok is True
    _exactly(st, [], "pedersen_verify_rlc")
    one = pp["s"].copy()
    one[100, 0] ^= 1                              # one item, in the second chunk
    ped_one = ped[:5] + [one, ped[6]]
    st, batch_ok = _both(pair, "pedersen_verify_rlc tampered",
                         lambda c: c.pedersen_verify_batch_rlc(*ped_one, ad=ad, seed=seed))
    assert batch_ok is False
    _exactly(st, [100], "pedersen_verify_rlc tampered")
