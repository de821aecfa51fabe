"""GPU: per-proof Pedersen verification from affine x || y points (vrfhip_pedersen_verify_batch_affine[_dev]) and the x || y
multi-context entry points (vrfhip_{ietf,pedersen}_verify_batch_affine_multi).  On every suite the affine verifier must give,
item for item, the statuses of the compressed verifier on the same points; an affine point with no compressed form (off the
curve, a coordinate equal to q) is InvalidData."""
import numpy as np
import pytest

from oracle import vrf_oracle as o

P256_P = 2 ** 256 - 2 ** 224 + 2 ** 192 + 2 ** 96 - 1
N = 4096 + 37


def _suites():
    import ark_ec_vrfs_amd as m
    return [(m.BandersnatchSha512Ell2, o.BANDERSNATCH.q, True), (m.JubJubSha512Tai, o.jubjub_params().q, True),
            (m.Ed25519Sha512Tai, o.ed25519_params().q, True), (m.BabyJubJubSha512Tai, o.baby_jubjub_params().q, True),
            (m.BandersnatchSwSha512Tai, o.BANDERSNATCH.q, False), (m.Secp256r1Sha256Tai, P256_P, False)]


def _ctx(suite):
    from ark_ec_vrfs_amd import BandersnatchSha512Ell2, Context
    return Context(0, suite, test_blinding_base=suite is not BandersnatchSha512Ell2)


def _le(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), np.uint8)


def _int(a):
    return int.from_bytes(a.tobytes(), "little")


def _to_mont(xy, q):
    out = xy.copy()
    for i in range(xy.shape[0]):
        for h in (0, 32):
            v = _int(xy[i, h:h + 32])
            out[i, h:h + 32] = _le(v * (1 << 256) % q) if v < q else xy[i, h:h + 32]
    return out


def _secrets(ctx, n):
    """n secret keys of the context's suite (`Secret::from_seed`)."""
    return ctx.secret_from_seed_batch(np.stack([np.frombuffer(o.synth_seed(i), np.uint8) for i in range(n)]), with_public=False)[0]


def _batch(ctx, q, edwards):
    """Compressed and affine forms of N Pedersen proofs with mutations; returns (comp, aff, s, sb, ad, no_comp) where
    no_comp marks the items whose affine points have no compressed form."""
    sk = _secrets(ctx, N)
    msgs = [o.synth_msg(i) for i in range(N)]
    ad = b"affine-verify"
    ctx.set_flags(0)
    pc = ctx.pedersen_prove_batch(sk, msgs=msgs, ad=ad)
    ctx.set_flags(ctx.PROVE_POINTS_AFFINE)
    pa = ctx.pedersen_prove_batch(sk, msgs=msgs, ad=ad)
    ctx.set_flags(0)
    assert (pc["status"] == 0).all() and (pa["status"] == 0).all()
    assert (pa["s"] == pc["s"]).all() and (pa["sb"] == pc["sb"]).all()
    st, h_xy = ctx.point_validate_batch(pc["input"], want_xy=True)
    assert (st == 0).all()
    comp = [pc[k].copy() for k in ("input", "output", "pk_com", "r", "ok")]
    aff = [h_xy.copy()] + [pa[k].copy() for k in ("output", "pk_com", "r", "ok")]
    s, sb = pc["s"].copy(), pc["sb"].copy()
    no_comp = np.zeros(N, bool)
    kinds = 6 if edwards else 5
    for i in range(0, N, 5):
        kind, p = (i // 5) % kinds, (i // 3) % 5
        if kind == 0:
            s[i, 1] ^= 2
        elif kind == 1:
            sb[i, 2] ^= 4
        elif kind == 2:                                    # swapped Gamma
            j = (i + 1) % N
            comp[1][i] = pc["output"][j]
            aff[1][i] = pa["output"][j]
        elif kind == 3:                                    # off the curve
            aff[p][i, 32:] = _le((_int(aff[p][i, 32:]) + 1) % q)
            no_comp[i] = True
        elif kind == 4:                                    # a coordinate equal to q
            aff[p][i, (i & 1) * 32:(i & 1) * 32 + 32] = _le(q)
            no_comp[i] = True
        else:                                              # shifted by the 2-torsion point (0, -1): (-x, -y)
            x, y = _int(aff[p][i, :32]), _int(aff[p][i, 32:])
            aff[p][i] = np.concatenate([_le((q - x) % q), _le((q - y) % q)])
            e = _int(comp[p][i])                           # y and the sign of x: both negate
            comp[p][i] = _le(((q - (e & ((1 << 255) - 1))) % q) | (((e >> 255) ^ 1) << 255))
    return comp, aff, s, sb, ad, no_comp


def _expect(ctx, comp, s, sb, ad, no_comp):
    want = ctx.pedersen_verify_batch(*comp, s, sb, ad=ad)
    want[no_comp] = 2
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(6))
def test_pedersen_affine_matches_compressed(idx):
    import torch
    suite, q, edwards = _suites()[idx]
    ctx = _ctx(suite)
    comp, aff, s, sb, ad, no_comp = _batch(ctx, q, edwards)
    want = _expect(ctx, comp, s, sb, ad, no_comp)
    assert (want == 0).sum() > N // 2 and (want == 1).any() and (want == 2).any()
    got = ctx.pedersen_verify_batch_affine(*aff, s, sb, ad=ad)
    assert (got == want).all(), (np.nonzero(got != want)[0][:10], got[got != want][:10], want[got != want][:10])
    # PREVALIDATED_ALL: no subgroup tests on either path
    ctx.set_flags(ctx.PREVALIDATED_ALL)
    want_pv = _expect(ctx, comp, s, sb, ad, no_comp)
    assert (ctx.pedersen_verify_batch_affine(*aff, s, sb, ad=ad) == want_pv).all()
    if edwards:
        assert (want_pv != want).any()                    # the small-order shifts are now VerificationFailure
    # arkworks' in-memory Montgomery limbs
    ctx.set_flags(ctx.COORDS_MONT256)
    aff_m = [_to_mont(a, q) for a in aff]
    assert (ctx.pedersen_verify_batch_affine(*aff_m, s, sb, ad=ad) == want).all()
    ctx.set_flags(0)
    # device pointers, on a stream that is not the default one
    dev = [torch.from_numpy(a).cuda() for a in aff + [s, sb]]
    adt = torch.from_numpy(np.frombuffer(ad, np.uint8).copy()).cuda()
    status = torch.full((N,), 255, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        ctx.pedersen_verify_batch_affine_dev(*dev, status, ad=adt, ad_len=len(ad), stream=stream.cuda_stream)
    stream.synchronize()
    assert (status.cpu().numpy() == want).all()
    # a workspace smaller than the batch: the chunk loop
    ctx.reserve(1000)
    assert (ctx.pedersen_verify_batch_affine(*aff, s, sb, ad=ad) == want).all()
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("idx", [0, 4, 5])
def test_affine_multi_matches_single_context(idx):
    from ark_ec_vrfs_amd import ietf_verify_batch_affine_multi, pedersen_verify_batch_affine_multi
    suite, q, edwards = _suites()[idx]
    c0, c1 = _ctx(suite), _ctx(suite)
    comp, aff, s, sb, ad, no_comp = _batch(c0, q, edwards)
    want = c0.pedersen_verify_batch_affine(*aff, s, sb, ad=ad)
    assert (pedersen_verify_batch_affine_multi([c0, c1], *aff, s, sb, ad=ad) == want).all()
    # rlc_seed: one MSM per slice, the per-proof statuses when a proof is bad
    assert (pedersen_verify_batch_affine_multi([c0, c1], *aff, s, sb, ad=ad, rlc_seed=bytes(range(32))) == want).all()
    # IETF through the x || y multi form
    n = 1000
    sk = _secrets(c0, n)
    msgs = [o.synth_msg(i) for i in range(n)]
    c0.set_flags(c0.PROVE_POINTS_AFFINE)
    r = c0.ietf_prove_batch(sk, msgs=msgs, ad=ad)
    c0.set_flags(0)
    st, h_xy = c0.point_validate_batch(r["input"], want_xy=True)
    ss = r["s"].copy()
    ss[::9, 3] ^= 1
    single = c0.ietf_verify_batch_affine(r["pk"], h_xy, r["output"], r["c"], ss, ad=ad)
    assert (single[::9] != 0).all() and (single[1::9] == 0).all()
    assert (ietf_verify_batch_affine_multi([c0, c1], r["pk"], h_xy, r["output"], r["c"], ss, ad=ad) == single).all()
    c0.close(); c1.close()


@pytest.mark.gpu
def test_affine_multi_refuses_mixed_contexts():
    from ark_ec_vrfs_amd import (BandersnatchSwSha512Tai, Secp256r1Sha256Tai, VrfHipError, ietf_verify_batch_affine_multi,
                                 pedersen_verify_batch_affine_multi)
    z64, z32 = np.zeros((4, 64), np.uint8), np.zeros((4, 32), np.uint8)
    a, b = _ctx(Secp256r1Sha256Tai), _ctx(BandersnatchSwSha512Tai)
    with pytest.raises(VrfHipError, match="disagree"):
        ietf_verify_batch_affine_multi([a, b], z64, z64, z64, z32, z32)
    with pytest.raises(VrfHipError, match="disagree"):
        pedersen_verify_batch_affine_multi([a, b], z64, z64, z64, z64, z64, z32, z32)
    c = _ctx(Secp256r1Sha256Tai)
    c.set_flags(c.COORDS_MONT256)
    with pytest.raises(VrfHipError, match="disagree"):
        ietf_verify_batch_affine_multi([a, c], z64, z64, z64, z32, z32)
    with pytest.raises(VrfHipError, match="disagree"):
        pedersen_verify_batch_affine_multi([a, c], z64, z64, z64, z64, z64, z32, z32, rlc_seed=bytes(32))
    for x in (a, b, c):
        x.close()
