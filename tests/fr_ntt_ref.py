"""Python-integer reference of the radix-2 transforms over Fr of BLS12-381 (ark-poly's Radix2EvaluationDomain), shared by
tests/test_hostsim_fr_ntt.py and tests/test_fr_ntt.py: a recursive transform, direct evaluation to check it against, and
closed forms for sparse polynomials at sizes where the recursion takes too long."""
import functools

from oracle import bls_oracle as bls

R = bls.R
TWO_ADICITY = 32
GENERATOR = 7
ROOT = pow(GENERATOR, (R - 1) >> TWO_ADICITY, R)          # TWO_ADIC_ROOT_OF_UNITY of ark-bls12-381's Fr
le = lambda x: int(x).to_bytes(32, "little")


def chunks10(pattern):
    return sum(pattern << (10 * w) for w in range(26)) % (1 << 255) % R


# the scalars of tests/test_hostsim_kzg_prove.py
EDGE_SCALARS = [0, 1, R - 1, chunks10(0x1ff), chunks10(0x200), chunks10(0x3ff)] + \
               [sum(pat << (10 * w) for w in range(25)) for pat in (0x1ff, 0x200, 0x3ff)]


def omega(log_n):
    """group_gen of the domain of size 2^log_n"""
    return pow(ROOT, 1 << (TWO_ADICITY - log_n), R)


def _ntt(a, w):
    n = len(a)
    if n == 1:
        return list(a)
    w2 = w * w % R
    ev, od = _ntt(a[0::2], w2), _ntt(a[1::2], w2)
    out, t, h = [0] * n, 1, n // 2
    for i in range(h):
        x = t * od[i] % R
        out[i] = (ev[i] + x) % R
        out[i + h] = (ev[i] - x) % R
        t = t * w % R
    return out


def fft(coeffs, offset=1):
    """out[i] = p(offset w^i): `fft`, or `coset_fft` on get_coset(offset)"""
    n = len(coeffs)
    log_n = n.bit_length() - 1
    assert n == 1 << log_n
    a, t = [], 1
    for c in coeffs:
        a.append(c * t % R)
        t = t * offset % R
    return _ntt(a, omega(log_n))


def ifft(evals, offset=1):
    """the coefficients of the polynomial of degree < n with these values: `ifft` / `coset_ifft`"""
    n = len(evals)
    log_n = n.bit_length() - 1
    assert n == 1 << log_n
    a = _ntt(list(evals), pow(omega(log_n), -1, R))
    ninv, oinv, t, out = pow(n, -1, R), pow(offset, -1, R), 1, []
    for c in a:
        out.append(c * ninv % R * t % R)
        t = t * oinv % R
    return out


def evaluate(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


def direct(coeffs, offset=1):
    n = len(coeffs)
    w = omega(n.bit_length() - 1)
    return [evaluate(coeffs, offset * pow(w, i, R) % R) for i in range(n)]


def sparse_evals(terms, log_n, offset=1):
    """the n values of sum c X^e for terms = [(e, c), ..] from running powers: O(n len(terms))"""
    n, w = 1 << log_n, omega(log_n)
    steps = [(pow(offset, e, R), pow(w, e, R), c) for e, c in terms]      # (offset w^i)^e = offset^e (w^e)^i
    cur = [o for o, _, _ in steps]
    out = []
    for _ in range(n):
        out.append(sum(c * x for x, (_, _, c) in zip(cur, steps)) % R)
        cur = [x * s % R for x, (_, s, _) in zip(cur, steps)]
    return out


def sparse_column(terms, log_n):
    col = [0] * (1 << log_n)
    for e, c in terms:
        col[e] = c
    return col


@functools.lru_cache(maxsize=None)
def self_check():
    """the recursion against direct evaluation at n <= 64, both domains, and the inverse against the forward"""
    import random
    rnd = random.Random(11)
    for log_n in range(7):
        p = [rnd.randrange(R) for _ in range(1 << log_n)]
        for off in (1, GENERATOR, rnd.randrange(1, R)):
            assert fft(p, off) == direct(p, off), (log_n, off)
            assert ifft(fft(p, off), off) == p
            assert sparse_evals([(j, c) for j, c in enumerate(p)], log_n, off) == direct(p, off)
    return True


def to_bytes(cols):
    return b"".join(le(x) for col in cols for x in col)


def from_bytes(buf, k, n):
    mv = bytes(buf)
    return [[int.from_bytes(mv[(c * n + j) * 32:(c * n + j + 1) * 32], "little") for j in range(n)] for c in range(k)]
