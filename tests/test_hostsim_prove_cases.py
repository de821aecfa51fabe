"""CPU: the cases of tests/prove_cases.py through the host build of the provers (tests/hostsim: hs_ / hj_ / hx_prove_cases =
prove_cases.inc, the three stages of k_prove.hip with K proofs per lane; hp_prove_cases and hb_prove_cases, the stages of
k_p256.hip and k_bsw.hip from a given H), byte for byte against the C oracle's proofs and, for pk and Gamma, against the
integer-arithmetic values of the generator.

This pins the logic of the provers' ladders -- prove_var_mul's four streams, the GLV Straus over {H, psi H} with and without the
all-entries lookup, sw_scalar_fold and the patched top digit of sw_quad_mul, sw_lookup_ct, the comb walks with their rippling
carry (8-bit rows here: VRF_GCOMB_BITS=8; the 16-bit rows exist on the device only), the 33rd row of sw_comb_mul -- and the
shared inversions of prove_prepare_multi, prove_encode_multi and k_bsw_prove_finish for anyone without a card, and makes a failure of
tests/test_gpu_prove_cases.py readable: logic fails in both builds, code generation on the device only.
Building a set runs the generator's self-checks (family properties, literal against integer expectations, non-empty families)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import prove_cases as pc

HS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim")
# suite -> (library, prefix of its entry points, setter of the decode stage's subgroup-test mask or None)
HOST = {"bandersnatch": ("libhostsim.so", "hs", "hs_set_check_mask_prove"),
        "jubjub": ("libhostsim_jj.so", "hj", "hj_set_check_mask"),
        "ed25519": ("libhostsim_f1.so", "hx", "hx_set_check_mask"),
        "baby_jubjub": ("libhostsim_f2.so", "hx", "hx_set_check_mask"),
        "secp256r1": ("libhostsim_p256.so", "hp", None),
        "bandersnatch_sw": ("libhostsim_bsw.so", "hb", None)}
EDWARDS = ("bandersnatch", "jubjub", "ed25519", "baby_jubjub")       # the suites whose stages read k_lane
CHK_INPUT = 2                                # a given H is wire data: what a default context tests in the provers
# out of an Edwards entry: gamma | c | s | pk (pk_com) | h | r | ok | sb | blinding, 32 bytes each
ED_FIELDS = {"output": 0, "c": 1, "s": 2, "pk": 3, "pk_com": 3, "input": 4, "r": 5, "ok": 6, "sb": 7, "blinding": 8}
# ... of the secp256r1 and bandersnatch_sw entries (points 33 bytes)
SW_FIELDS = {"output": (0, 33), "c": (33, 32), "s": (65, 32), "pk": (97, 33), "pk_com": (97, 33), "input": (130, 33),
             "r": (163, 33), "ok": (196, 33), "sb": (229, 32), "blinding": (261, 32)}


def _lib(suite):
    libname = HOST[suite][0]
    subprocess.run(["make", "-C", HS, "-j4", libname], check=True, stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(os.path.join(HS, libname))
    if suite == "secp256r1":
        B = pc.blinding(suite).B
        lib.hp_set_blinding_base(B[0].to_bytes(32, "big") + B[1].to_bytes(32, "big"))
    return lib


def _prove(suite, cs, pedersen, ad, rows=None, K=1, ct=False, msgs=None):
    """the host provers over the given rows of the set (in that order): a result dict like the library's"""
    lib = _lib(suite)
    rows = np.arange(cs.n) if rows is None else np.asarray(rows)
    n = len(rows)
    keys = pc.PED_KEYS if pedersen else pc.IETF_KEYS
    sk = np.ascontiguousarray(cs.sk[rows])
    setter = HOST[suite][2]
    if suite in EDWARDS:
        out, st = np.zeros((n, 288), np.uint8), np.full(n, 9, np.uint8)
        if msgs is None:
            inp = np.ascontiguousarray(cs.inputs[rows])
            src = (None, 0, inp.ctypes.data_as(ctypes.c_void_p))
        else:
            m = np.ascontiguousarray(msgs[rows])
            src = (m.ctypes.data_as(ctypes.c_void_p), m.shape[1], None)
        getattr(lib, setter)(CHK_INPUT)
        try:
            getattr(lib, HOST[suite][1] + "_prove_cases")(K, int(pedersen), int(ct), n, sk.ctypes.data_as(ctypes.c_void_p), *src,
                                                        ad, len(ad), out.ctypes.data_as(ctypes.c_void_p), st.ctypes.data_as(ctypes.c_void_p))
        finally:
            getattr(lib, setter)(0)          # the libraries are shared with the other host-simulation tests of this process
        res = {k: out[:, 32 * ED_FIELDS[k]:32 * ED_FIELDS[k] + 32].copy() for k in keys}
    else:
        assert K == 1 and msgs is None
        out, st = np.zeros((n, 293), np.uint8), np.full(n, 9, np.uint8)
        buf = ctypes.create_string_buffer(293)
        f = getattr(lib, HOST[suite][1] + "_prove_cases")
        for j, i in enumerate(rows):
            a = (int(pedersen), int(ct)) + ((CHK_INPUT,) if suite == "bandersnatch_sw" else ())
            st[j] = f(*a, cs.sk[i].tobytes(), cs.inputs[i].tobytes(), ad, len(ad), buf)
            out[j] = np.frombuffer(buf.raw, np.uint8)
        res = {k: out[:, SW_FIELDS[k][0]:SW_FIELDS[k][0] + SW_FIELDS[k][1]].copy() for k in keys}
    res["status"] = st
    return res


def _check(cs, got, want, pedersen, rows, what):
    """against the C oracle's bytes, and pk / Gamma against the integer-arithmetic values"""
    pc.compare(cs, got, want, pc.PED_KEYS if pedersen else pc.IETF_KEYS, rows, what)
    assert (got["output"] == cs.gamma_int[rows]).all(), what
    if not pedersen:
        assert (got["pk"] == cs.pk_int[rows]).all(), what


@pytest.mark.parametrize("suite", pc.SUITES)
def test_the_set_holds_what_it_must(suite):
    """the generator's self-checks ran (cases() asserts them); every family is there, the count is odd and stays small"""
    cs = pc.cases(suite)
    g = pc.group(suite)
    print(cs.describe())
    fams = cs.family_counts()
    want = {"small", "nib", "stream", "comb", "range", "rand", "input"} | ({"glv"} if g.glv else set()) | (
        {"fold"} if suite == "secp256r1" else set())
    assert set(fams) == want and all(fams[f] > 0 for f in want)
    assert cs.n % 2 == 1 and cs.n % 8 != 0 and 200 < cs.n < pc.MAX_CASES and cs.n_literal >= pc.N_LITERAL
    assert fams["rand"] >= pc.N_RANDOM and fams["range"] == 5 and (not g.glv or fams["glv"] >= pc.N_GLV_MAX + 12)
    assert (cs.status[[i for i, k in enumerate(cs.sk_int) if k >= g.r]] == 2).all()
    assert (cs.status[[i for i, k in enumerate(cs.kinds) if k == "raw"]] == 2).all()
    zero = [i for i, k in enumerate(cs.sk_int) if k == 0 and cs.kinds[i] in ("log", "B")]
    assert len(zero) >= 6 and (cs.status[zero] == 0).all()           # sk = 0 is a secret (Secret::from_scalar takes it)
    # pk_com = sk*G + b*B by the Python oracle's additions is what the C oracle committed to
    assert (cs.pk_com_int == cs.ped[1]["pk_com"]).all()
    assert (cs.pk_int == cs.ietf[0]["pk"]).all() and (cs.gamma_int == cs.ietf[0]["output"]).all()
    # the oracle's own verifier takes its proofs (cases() asserts it under every ad), all but those of sk = 0 on secp256r1
    assert int((cs.round_trip != 0).sum()) == (sum(cs.sk_int[i] == 0 for i in cs.accepted) if suite == "secp256r1" else 0)
    assert ((cs.round_trip_ped != 0) == (cs.round_trip != 0)).all()


@pytest.mark.parametrize("pedersen", (False, True), ids=("ietf", "pedersen"))
@pytest.mark.parametrize("suite", pc.SUITES)
def test_host_provers_on_the_whole_set(suite, pedersen):
    """every case under each of the three ad"""
    cs = pc.cases(suite)
    print(cs.describe())
    want = cs.ped if pedersen else cs.ietf
    for a, ad in enumerate(pc.ADS):
        _check(cs, _prove(suite, cs, pedersen, ad), want[a], pedersen, np.arange(cs.n), "ad %d" % len(ad))


@pytest.mark.parametrize("suite", pc.SUITES)
def test_host_ct_lookups_give_the_same_bytes(suite):
    """win_lookup_t<true> / sw_lookup_ct on the crafted digits (0, +-8, the negated fold): the oracle's bytes again"""
    cs = pc.cases(suite)
    print(cs.describe())
    _check(cs, _prove(suite, cs, False, pc.ADS[1], ct=True), cs.ietf[1], False, np.arange(cs.n), "ct ietf")
    _check(cs, _prove(suite, cs, True, pc.ADS[1], ct=True), cs.ped[1], True, np.arange(cs.n), "ct pedersen")


@pytest.mark.parametrize("K", (1, 2, 4, 8))
@pytest.mark.parametrize("suite", EDWARDS)
def test_host_several_proofs_per_lane(suite, K):
    """prove_encode_multi's shared inversion of 4K Z coordinates: refused items, sk = 0 and neutral inputs at every place within
    a lane's group (the set in its order and rolled by one), the last lane part full; both schemes"""
    cs = pc.cases(suite)
    print(cs.describe())
    rows = np.arange(cs.n)
    for pedersen in (False, True):
        want = (cs.ped if pedersen else cs.ietf)[1]
        for r in (rows, np.roll(rows, 1)):
            _check(cs, _prove(suite, cs, pedersen, pc.ADS[1], r, K=K), want, pedersen, r, "K=%d %s" % (K, "pedersen" if pedersen else "ietf"))


@pytest.mark.parametrize("K", (1, 2, 4, 8))
def test_host_several_proofs_per_lane_from_messages(K):
    """Bandersnatch from messages: prove_prepare_multi's two shared inversions (2K Elligator denominators, K Z of H) as well"""
    cs = pc.cases("bandersnatch")
    print(cs.describe())
    rows = cs.secret_rows
    for pedersen in (False, True):
        want = cs.ped_msg if pedersen else cs.ietf_msg
        for r in (rows, np.roll(rows, 1)):
            got = _prove("bandersnatch", cs, pedersen, pc.ADS[1], r, K=K, msgs=cs.msgs)
            pc.compare(cs, got, want, pc.PED_KEYS if pedersen else pc.IETF_KEYS, r, "msgs K=%d" % K)


@pytest.mark.parametrize("suite", EDWARDS)
def test_host_provers_from_messages(suite):
    """the secrets behind the Elligator and try-and-increment front ends"""
    cs = pc.cases(suite)
    print(cs.describe())
    rows = cs.secret_rows
    pc.compare(cs, _prove(suite, cs, False, pc.ADS[1], rows, msgs=cs.msgs), cs.ietf_msg, pc.IETF_KEYS, rows, "msgs ietf")
    pc.compare(cs, _prove(suite, cs, True, pc.ADS[1], rows, msgs=cs.msgs), cs.ped_msg, pc.PED_KEYS, rows, "msgs pedersen")


def _split(buf, layout):
    """{name: (n, width) array} of a row-major output buffer with the given (name, width) columns"""
    out, off = {}, 0
    for name, w in layout:
        if name:
            out[name] = buf[:, off:off + w].copy()
        off += w
    assert off == buf.shape[1]
    return out


@pytest.mark.parametrize("suite", EDWARDS + ("secp256r1",))
def test_the_entries_the_host_builds_had(suite):
    """The accepted cases through the per-item provers the host builds had before prove_cases.inc (hs_ietf_prove, hs_pedersen_prove,
    hs_ietf_prove_multi with its eight proofs per lane; hj_prove / hx_prove; hp_prove, hp_ped_prove), so that the older
    host-simulation tests' entry points see the crafted secrets too.  These run the ladders on the secret as it stands -- the kernels
    zero one that is not canonical first -- so the refused cases stay with the entries above; the Pedersen and try-and-increment
    entries take messages only."""
    cs = pc.cases(suite)
    print(cs.describe())
    lib = _lib(suite)
    ad = pc.ADS[1]
    acc = cs.accepted
    sec = np.array([i for i in cs.secret_rows if cs.status[i] == 0])
    st0 = {"status": np.zeros(cs.n, np.uint8)}
    if suite == "secp256r1":
        out = np.zeros((len(acc), 261), np.uint8)
        buf = ctypes.create_string_buffer(261)
        for j, i in enumerate(acc):
            assert lib.hp_prove(cs.sk[i].tobytes(), None, 0, cs.inputs[i].tobytes(), ad, len(ad), buf) == 1
            out[j] = np.frombuffer(buf.raw, np.uint8)
        got = _split(out, (("pk", 33), ("input", 33), ("output", 33), ("c", 32), ("s", 32), ("", 98)))
        got["status"] = st0["status"][acc]
        pc.compare(cs, got, cs.ietf[1], pc.IETF_KEYS, acc, "hp_prove")
        out = np.zeros((len(sec), 261), np.uint8)
        for j, i in enumerate(sec):
            assert lib.hp_ped_prove(cs.sk[i].tobytes(), cs.msgs[i].tobytes(), pc.MSG_LEN, ad, len(ad), buf) == 1
            out[j] = np.frombuffer(buf.raw, np.uint8)
        got = _split(out, (("output", 33), ("pk_com", 33), ("r", 33), ("ok", 33), ("s", 32), ("sb", 32), ("blinding", 32), ("input", 33)))
        got["status"] = st0["status"][sec]
        pc.compare(cs, got, cs.ped_msg, pc.PED_KEYS, sec, "hp_ped_prove")
        return
    prefix, setter = HOST[suite][1], HOST[suite][2]
    ietf_cols = (("output", 32), ("c", 32), ("s", 32), ("pk", 32), ("input", 32))
    ped_cols = (("output", 32), ("pk_com", 32), ("r", 32), ("ok", 32), ("s", 32), ("sb", 32), ("blinding", 32))
    buf = ctypes.create_string_buffer(224)
    if suite == "bandersnatch":
        lib.hs_set_check_mask_prove(CHK_INPUT)
        try:
            out = np.zeros((len(acc), 160), np.uint8)
            b = [ctypes.create_string_buffer(32) for _ in range(5)]
            for j, i in enumerate(acc):
                assert lib.hs_ietf_prove(cs.sk[i].tobytes(), None, 0, cs.inputs[i].tobytes(), ad, len(ad), *b) == 1
                out[j] = np.frombuffer(b"".join(x.raw for x in b), np.uint8)
        finally:
            lib.hs_set_check_mask_prove(0)
        got = _split(out, (("output", 32), ("c", 32), ("s", 32), ("input", 32), ("pk", 32)))
        got["status"] = st0["status"][acc]
        pc.compare(cs, got, cs.ietf[1], pc.IETF_KEYS, acc, "hs_ietf_prove")
        sk, msgs = np.ascontiguousarray(cs.sk[sec]), np.ascontiguousarray(cs.msgs[sec])
        out = np.zeros((len(sec), 160), np.uint8)
        lib.hs_ietf_prove_multi(len(sec), sk.ctypes.data_as(ctypes.c_void_p), msgs.ctypes.data_as(ctypes.c_void_p), pc.MSG_LEN, ad, len(ad),
                                out.ctypes.data_as(ctypes.c_void_p))
        got = _split(out, ietf_cols)
        got["status"] = st0["status"][sec]
        pc.compare(cs, got, cs.ietf_msg, pc.IETF_KEYS, sec, "hs_ietf_prove_multi")
        prove = lambda ped, i: lib.hs_pedersen_prove(cs.sk[i].tobytes(), cs.msgs[i].tobytes(), pc.MSG_LEN, ad, len(ad), buf)
        schemes = (True,)
    else:
        prove = lambda ped, i: getattr(lib, prefix + "_prove")(int(ped), cs.sk[i].tobytes(), cs.msgs[i].tobytes(), pc.MSG_LEN, ad, len(ad), buf)
        schemes = (False, True)
    for ped in schemes:
        out = np.zeros((len(sec), 224 if ped else 160), np.uint8)
        for j, i in enumerate(sec):
            assert prove(ped, i) == 1
            out[j] = np.frombuffer(buf.raw[:out.shape[1]], np.uint8)
        got = _split(out, ped_cols if ped else ietf_cols)
        got["status"] = st0["status"][sec]
        keys = tuple(k for k in (pc.PED_KEYS if ped else pc.IETF_KEYS) if k in got)
        pc.compare(cs, got, cs.ped_msg if ped else cs.ietf_msg, keys, sec, "%s_prove %s" % (prefix, "pedersen" if ped else "ietf"))
