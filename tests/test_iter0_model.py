"""The VN phase of BP iteration 0 is the identity on the prior pair (CPU model).

bp_regular.hip (decode_reg's closed form) replaces the first VN phase of a FAST
decode by stores of (p, 1 - p): InitMsg sets every c2v to (0.5, 0.5), and for a
prior in the FAST domain (bp_common.hpp fast_prior_ok: +0, 1, or p and 1 - p
>= lo = 2^(40 dv - 960)) the reference's column recursion
(binaryldpccodec.cc:177-212) then returns the prior pair on every edge.  This
restates the recursion in IEEE doubles (numpy float64: + - * / correctly
rounded, like the reference's SSE2 arithmetic) and checks the identity bit for
bit for every column degree the FAST path admits, and that it fails outside the
domain — why the exact kernel keeps the generic chain.
"""
import math

import numpy as np
import pytest

DEGREES = list(range(1, 24))  # kFastMaxColumnDegree = 23


def vn_iter0(p, dv):
    """One column of degree dv with every c2v = (0.5, 0.5); p: float64 array.
    Returns (v2c0[dv], v2c1[dv], decision)."""
    p = np.asarray(p, np.float64)
    c0 = c1 = np.float64(0.5)
    al = [(p, 1.0 - p)]  # alpha of the first edge (:180-181)
    with np.errstate(all="ignore"):
        for k in range(dv):  # forward (:182-189); al[dv] is the column head's
            n0, n1 = al[k][0] * c0, al[k][1] * c1
            s = n0 + n1
            al.append((n0 / s, n1 / s))
        dec = np.where(al[dv][0] > al[dv][1], 0, 1)  # (:191-194)
        b0 = b1 = np.ones_like(p)  # backward (:197-212)
        v0, v1 = [None] * dv, [None] * dv
        for k in range(dv - 1, -1, -1):
            t0, t1 = al[k][0] * b0, al[k][1] * b1
            s = t0 + t1
            v0[k], v1[k] = t0 / s, t1 / s
            u0, u1 = b0 * c0, b1 * c1
            s = u0 + u1
            b0, b1 = u0 / s, u1 / s
    return v0, v1, dec


def lo_of(dv):
    return math.ldexp(1.0, 40 * dv - 960)


def in_domain(p, lo):
    """bp_common.hpp fast_prior_ok"""
    p = np.asarray(p, np.float64)
    return ((p == 0.0) & ~np.signbit(p)) | (p == 1.0) | ((p >= lo) & (1.0 - p >= lo))


def same_bits(a, b):
    return np.asarray(a, np.float64).view(np.int64) == np.asarray(b, np.float64).view(np.int64)


def specials(dv):
    lo = lo_of(dv)
    below1 = math.nextafter(1.0, 0.0)
    top = below1 if 1.0 - below1 >= lo else 1.0 - lo  # the largest p with 1 - p >= lo
    assert 1.0 - top >= lo and not (1.0 - math.nextafter(top, 1.0) >= lo and math.nextafter(top, 1.0) < 1.0)
    s = [0.0, 1.0, 0.5, math.nextafter(0.5, 0.0), math.nextafter(0.5, 1.0), lo, math.nextafter(lo, 1.0), 1.0 - lo,
         top, 1e-12, 1.0 - 1e-12, 2.0 ** -53, 2.0 ** -54, 1.0 - 2.0 ** -53, 1.0 - 2.0 ** -54]
    s = np.array(s, np.float64)
    must = np.array([0.0, 1.0, 0.5, math.nextafter(0.5, 0.0), math.nextafter(0.5, 1.0), lo, math.nextafter(lo, 1.0),
                     1.0 - lo, top, 1e-12, 1.0 - 1e-12])
    assert in_domain(must, lo).all()
    return s[in_domain(s, lo)]  # (2^-53, 2^-54 and their complements leave the domain at dv = 23)


def randoms(dv, rng, n=100000):
    lo = lo_of(dv)
    u = rng.random(n // 2)  # uniform in value
    e = rng.integers(40 * dv - 960, 0, n // 2)  # uniform in exponent, [lo, 1)
    m = np.ldexp(1.0 + rng.random(n // 2), e)
    m[::2] = 1.0 - m[::2]  # half of them next to 1
    p = np.concatenate([u, m])
    p = p[in_domain(p, lo)]
    assert p.size > 0.9 * n
    return p


@pytest.mark.parametrize("dv", DEGREES)
def test_iter0_vn_phase_is_the_prior_pair(dv):
    rng = np.random.default_rng(1000 + dv)
    p = np.concatenate([specials(dv), randoms(dv, rng)])
    q = 1.0 - p
    v0, v1, dec = vn_iter0(p, dv)
    for k in range(dv):
        bad = ~(same_bits(v0[k], p) & same_bits(v1[k], q))
        assert not bad.any(), (dv, k, p[bad][:4], v0[k][bad][:4], v1[k][bad][:4])
    assert np.array_equal(dec, np.where(p > q, 0, 1)), dv
    assert dec[p == 0.5].all()  # the tie decides 1


def test_iter0_scalar_python_floats_agree():
    """The same recursion on plain Python floats (no numpy) for a few priors:
    the array model above is not an artefact of vectorised arithmetic."""
    for dv in (1, 3, 6, 23):
        lo = lo_of(dv)
        for p in (0.0, 1.0, 0.5, math.nextafter(0.5, 0.0), lo, 1.0 - lo, 1e-12, 0.3, 1.0 - 2.0 ** -53):
            al = [(p, 1.0 - p)]
            for k in range(dv):
                n0, n1 = al[k][0] * 0.5, al[k][1] * 0.5
                al.append((n0 / (n0 + n1), n1 / (n0 + n1)))
            b = (1.0, 1.0)
            for k in range(dv - 1, -1, -1):
                t0, t1 = al[k][0] * b[0], al[k][1] * b[1]
                assert (t0 / (t0 + t1), t1 / (t0 + t1)) == (p, 1.0 - p), (dv, k, p)
                u0, u1 = b[0] * 0.5, b[1] * 0.5
                b = (u0 / (u0 + u1), u1 / (u0 + u1))
            assert (0 if al[dv][0] > al[dv][1] else 1) == (0 if p > 1.0 - p else 1)


@pytest.mark.parametrize("dv", [2, 3, 23])  # (dv = 1 has no forward step to go wrong)
def test_identity_fails_outside_the_fast_domain(dv):
    """Out-of-domain priors the exact kernel may meet: the smallest subnormal
    (its halving rounds to 0), an odd subnormal and the odd normal just above
    2^-1022 (their halvings lose the last bit).  Each breaks the bit-for-bit
    identity on some edge."""
    lo = lo_of(dv)
    for p in (5e-324, 1.5e-323, math.nextafter(2.0 ** -1022, 1.0)):
        arr = np.array([p])
        assert not in_domain(arr, lo)[0]
        v0, v1, _ = vn_iter0(arr, dv)
        assert not all(same_bits(v0[k], arr)[0] and same_bits(v1[k], 1.0 - arr)[0] for k in range(dv)), p
