"""Host model of the near-one reciprocal (kmldpc_amd/csrc/bp_common.hpp
rcp_near1) in exact rational arithmetic.

rcp_near1(s) = fma(X2, Y, -s) with X2 = 2 (1 + 2^-26) and Y = 1 - 2^-26 + 2^-52:
the product is 2 + 2^-77 exactly, so the fma rounds 1 + u + 2^-77 once, u = 1 - s.
On every double s with |s - 1| <= 2^-40 (1 + j 2^-52, j <= 2^12, and
1 - k 2^-53, k <= 2^13: 12,289 values) that must be RN(1/s), and equal to the
earlier two-operation form fma(X, Y, 1 - s), X = 1 + 2^-26, X Y = 1 + 2^-78.
float(Fraction) is round-to-nearest-even, so every fma here rounds once.
"""
from fractions import Fraction as F

import pytest

X2 = float.fromhex("0x1.0000004p+1")
X = float.fromhex("0x1.0000004p+0")
Y = float.fromhex("0x1.ffffff8000002p-1")
JMAX, KMAX = 2 ** 12, 2 ** 13


def rn(x):
    return float(x)


def rcp_one_fma(s):
    return rn(F(X2) * F(Y) - F(s))


def rcp_two_ops(s):
    u = rn(F(1) - F(s))
    return rn(F(X) * F(Y) + F(u))


@pytest.fixture(scope="module")
def domain():
    above = [1.0 + j * 2.0 ** -52 for j in range(JMAX + 1)]
    below = [1.0 - k * 2.0 ** -53 for k in range(1, KMAX + 1)]
    # the constructions are exact and these are all the doubles of the range
    assert all(F(s) == 1 + F(j, 2 ** 52) for j, s in enumerate(above))
    assert all(F(s) == 1 - F(k, 2 ** 53) for k, s in enumerate(below, 1))
    s = above + below
    assert len(set(s)) == len(s) == 12289
    assert max(abs(F(v) - 1) for v in s) == F(1, 2 ** 40)
    return above, below


def test_constants():
    assert F(X2) == 2 * (1 + F(1, 2 ** 26)) and F(X2) == 2 * F(X)
    assert F(Y) == 1 - F(1, 2 ** 26) + F(1, 2 ** 52)
    assert F(X2) * F(Y) == 2 + F(1, 2 ** 77)
    assert F(X) * F(Y) == 1 + F(1, 2 ** 78)


def test_one_fma_is_the_correctly_rounded_reciprocal(domain):
    above, below = domain
    for s in above + below:
        r = rcp_one_fma(s)
        assert r == rn(1 / F(s)), s.hex()
        assert r == rcp_two_ops(s), s.hex()


def test_one_minus_s_is_exact(domain):
    above, below = domain
    for s in above + below:
        assert F(1.0 - s) == 1 - F(s), s.hex()


def test_ties_and_fixed_points(domain):
    """s = 1 - k 2^-53: 1 + u = 1 + k 2^-53 is a double for even k (a fixed
    point: the bias is dropped) and a rounding midpoint for odd k, which the
    bias (like the u^2 term of 1/s) breaks upwards whatever the neighbours'
    parity.  s = 1 + j 2^-52: 1 + u = 1 - j 2^-52 is always a double."""
    above, below = domain
    for k, s in enumerate(below, 1):
        want = 1 + F(k + (k & 1), 2 ** 53)
        assert F(rcp_one_fma(s)) == want, k
        if k & 1:  # ties-to-even alone would round half of these down
            assert F(rn(1 + F(k, 2 ** 53))) == 1 + F(k - 1 if k % 4 == 1 else k + 1, 2 ** 53)
    for j, s in enumerate(above):
        assert F(rcp_one_fma(s)) == 1 - F(j, 2 ** 52), j
