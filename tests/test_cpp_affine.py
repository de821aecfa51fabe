"""The affine-point verifiers of the C++ mirror (include/vrfhip.hpp: ietf / pedersen verify, verify_batch,
verify_batch_sharded over utils::XY).  CPU: tests/cpp_affine/affine_test compiles and links against libvrfhip.so.  GPU: it
verifies the Bandersnatch golden vector from x || y points (decoded here by the oracle) and rejects tampered items."""
import os
import subprocess

import pytest

from oracle import vrf_oracle as o

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp_affine")
EXE = os.path.join(HERE, "affine_test")


def _build():
    subprocess.run(["make", "-C", HERE], check=True, stdout=subprocess.DEVNULL)


def _xy(enc_hex):
    x, y = o.point_decode(o.BANDERSNATCH, bytes.fromhex(enc_hex))
    return (x.to_bytes(32, "little") + y.to_bytes(32, "little")).hex()


def test_cpp_affine_builds_and_links(native_built):
    _build()
    assert os.path.exists(EXE)
    out = subprocess.run(["ldd", EXE], capture_output=True, text=True).stdout
    assert "libvrfhip.so" in out and "not found" not in out.split("libvrfhip.so")[1].splitlines()[0]


@pytest.mark.gpu
def test_cpp_affine_kat_and_batches(kat):
    _build()
    p = kat["pedersen"][0]
    v = next(x for x in kat["ietf"] if x["seed"] == p["seed"] and x["alpha"] == p["alpha"])
    args = [v["ad"], _xy(v["pk"]), _xy(v["h"]), _xy(v["gamma"]), v["c"], v["s"],
            p["ad"], _xy(p["pk_com"]), _xy(p["r"]), _xy(p["ok"]), p["s"], p["sb"]]
    r = subprocess.run([EXE] + args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "affine_test ok" in r.stdout
