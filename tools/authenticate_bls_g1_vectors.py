#!/usr/bin/env python3
"""Provenance tool for tests/golden/bls12_381_g1_compressed.json.

The 48-byte compressed form of BLS12-381 G1 points (the zcash serialisation that ark-bls12-381 adopts: x big-endian, bit 7
of byte 0 = compressed, bit 6 = infinity, bit 5 = y is the larger of {y, p - y}) written from the format's definition with
Python big ints.  It imports nothing from this repository, in particular not the oracle or the codec it helps to pin.

What is RECALLED, and how it is authenticated: the generator's published coordinates and its published compressed encoding
(97f1d3a7...db22c6bb) are two separately remembered strings.  The script decodes the encoding from the definition above (one
square root, the sort flag) and requires the result to be the published coordinates, on the curve and of order r.  A
recalled field that does not reproduce is discarded and written as "computed", never adjusted.  Every other vector (infinity,
-G, 2G, further multiples, (r - 1) G, ...) is computed from the authenticated generator.

usage: python tools/authenticate_bls_g1_vectors.py            compare the committed file with what is computed here
       python tools/authenticate_bls_g1_vectors.py --write    (re)write it
"""
import json
import os
import sys

p = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
r = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
# published generator of G1, as recalled
G = (0x17F1D3A73197D7942695638C4FA9AC0FC3688C4F9774B905A14E3A3F171BAC586C55E83FF97A1AEFFB3AF00ADB22C6BB,
     0x08B3F481E3AAA0F1A09E30ED741D8AE4FCF5E095D5D00AF600DB18CB2C04B3EDD03CC744A2888AE40CAA232946C5E7E1)
# its published compressed encoding, as recalled
G_COMPRESSED = "97f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb"


def add(P, Q):
    if P is None:
        return Q
    if Q is None:
        return P
    if P[0] == Q[0]:
        if (P[1] + Q[1]) % p == 0:
            return None
        lam = 3 * P[0] * P[0] * pow(2 * P[1], -1, p) % p
    else:
        lam = (Q[1] - P[1]) * pow(Q[0] - P[0], -1, p) % p
    x = (lam * lam - P[0] - Q[0]) % p
    return (x, (lam * (P[0] - x) - P[1]) % p)


def mul(k, P):
    R = None
    for bit in bin(k)[2:]:
        R = add(R, R)
        if bit == "1":
            R = add(R, P)
    return R


def enc(P):
    if P is None:
        return bytes([0xC0]) + bytes(47)
    b = bytearray(P[0].to_bytes(48, "big"))
    b[0] |= 0x80 | (0x20 if P[1] > p - P[1] else 0)
    return bytes(b)


def dec(s):
    """The format's definition, no subgroup test; None = not an encoding of a curve point."""
    if len(s) != 48 or not s[0] & 0x80:
        return None
    x = int.from_bytes(bytes([s[0] & 0x1F]) + s[1:], "big")
    if s[0] & 0x40:
        return "infinity" if x == 0 and not s[0] & 0x20 else None
    if x >= p:
        return None
    y2 = (x * x * x + 4) % p
    y = pow(y2, (p + 1) // 4, p)
    if y * y % p != y2:
        return None
    return (x, y if (y > p - y) == bool(s[0] & 0x20) else p - y)


def vectors():
    assert p % 4 == 3 and (G[1] * G[1] - G[0] ** 3 - 4) % p == 0, "generator not on y^2 = x^3 + 4"
    assert mul(r, G) is None, "generator order"
    recalled_ok = dec(bytes.fromhex(G_COMPRESSED)) == G and enc(G).hex() == G_COMPRESSED
    print("generator: recalled encoding %s the recalled coordinates" % ("REPRODUCES" if recalled_ok else "does NOT reproduce"))
    out = []

    def put(name, k, P, origin="computed"):
        e = enc(P)
        assert (dec(e) == "infinity") if P is None else (dec(e) == P)
        out.append(dict(name=name, k="%x" % k, compressed=e.hex(),
                        x="%096x" % (P[0] if P else 0), y="%096x" % (P[1] if P else 0), origin=origin))
    put("infinity", 0, None)
    put("G", 1, G, "recalled (encoding and coordinates), reproduced" if recalled_ok else "computed")
    put("-G", r - 1, mul(r - 1, G))
    assert mul(r - 1, G) == (G[0], p - G[1])
    put("2G", 2, mul(2, G))
    for k in (3, 4, 5, 7, 8, 0xD201000000010000, r - 2, (r - 1) // 2, (r + 1) // 2, r // 3):
        put("%xG" % k, k, mul(k, G))
    lead = {v["compressed"][0] for v in out}
    assert lead & {"8", "9"} and lead & {"a", "b"} and "c" in lead, "both sort flags and infinity occur"
    return dict(
        source="tools/authenticate_bls_g1_vectors.py: zcash / ark-bls12-381 compressed G1 encodings, Python big ints",
        format="compressed: 48 bytes, x big-endian, flags in the top three bits of byte 0; x, y: big-endian hex; k: the "
               "multiple of the generator, hex",
        vectors=out)


if __name__ == "__main__":
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "bls12_381_g1_compressed.json")
    doc = vectors()
    if "--write" in sys.argv[1:]:
        with open(path, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        print("wrote", os.path.normpath(path))
        sys.exit(0)
    same = os.path.exists(path) and json.load(open(path)) == doc
    print("committed file %s" % ("matches" if same else "DOES NOT MATCH what this script computes"))
    sys.exit(0 if same else 1)
