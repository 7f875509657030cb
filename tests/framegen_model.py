"""Exact host model of the GPU frame generator (kmldpc_amd/csrc/framegen.hip).

The generator is counter based, so every value it draws can be restated on
the host from the definition alone and compared draw for draw:

  * Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as
    easy as 1, 2, 3", SC'11) with the counter (cw lo, cw hi, stream, idx) and
    the key (seed lo, seed hi); cw is the global codeword index.  Streams:
    1 = source bits, 2 = the channel coefficient h, 3 = noise.
  * source bits: the 32-bit output lanes of draws idx = 0, 1, ... of stream 1,
    in the order x, y, z, w, read as one little-endian bit string; info bit n
    is bit n % 32 of lane n / 32 (so a 64-bit word is two lanes, low lane in
    the low half, and two words share one draw).
  * a uniform in (0, 1] from two lanes: the top 53 bits of (hi << 32 | lo),
    plus one, times 2^-53.
  * Box-Muller: (sqrt(-2 ln u1) cos 2 pi u2, sqrt(-2 ln u1) sin 2 pi u2) with
    u1 from lanes (x, y) and u2 from lanes (z, w), high lane first.
  * h = gauss2(stream 2, idx 0) / sqrt 2, one per codeword; the noise of
    symbol j is gauss2(stream 3, idx j) * noise_scale;  y = x h + noise, x the
    constellation point of the MSB-first label.

The Gaussian pair is evaluated in mpmath at GAUSS_PREC bits and rounded to
double once; the few operations after it are individual IEEE double
operations (the library is built with -ffp-contract=off), which numpy float64
reproduces exactly.  gauss2_fast is the same map in numpy float64, for the
statistical tests only.
"""
import functools
import math
from fractions import Fraction

import mpmath
import numpy as np

STREAM_BITS, STREAM_H, STREAM_NOISE = 1, 2, 3
GAUSS_PREC = 120  # bits: the model's own error is 2^-67 ulp of a double, its one rounding aside

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)  # round multipliers
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)  # Weyl key increments
_LO = np.uint64(0xFFFFFFFF)
_32 = np.uint64(32)


def philox4x32_10(ctr, key):
    """Philox4x32-10 of ctr[..., 4] under key[..., 2] (32-bit words held in
    uint64, broadcast against each other); returns uint64 [..., 4]."""
    ctr = np.asarray(ctr, dtype=np.uint64)
    key = np.asarray(key, dtype=np.uint64)
    shape = np.broadcast_shapes(ctr.shape[:-1], key.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(ctr[..., i], shape) for i in range(4))
    k0, k1 = (np.broadcast_to(key[..., i], shape) for i in range(2))
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2  # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> _32) ^ c1 ^ k0, p1 & _LO, (p0 >> _32) ^ c3 ^ k1, p0 & _LO
        k0, k1 = (k0 + _W0) & _LO, (k1 + _W1) & _LO
    return np.stack([c0, c1, c2, c3], axis=-1)


def counter(cw, stream, idx):
    """The Philox counter of draw idx of a stream of codeword cw (uint64 [..., 4])."""
    cw = np.asarray(cw, dtype=np.uint64)
    idx = np.asarray(idx, dtype=np.uint64)
    shape = np.broadcast_shapes(cw.shape, idx.shape)
    cw, idx = np.broadcast_to(cw, shape), np.broadcast_to(idx, shape)
    return np.stack([cw & _LO, cw >> _32, np.full(shape, stream, np.uint64), idx & _LO], axis=-1)


def draw(seed, cw, stream, idx):
    """Four 32-bit lanes (x, y, z, w) of draw idx of a stream of codeword cw."""
    seed = int(seed) & (2**64 - 1)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    return philox4x32_10(counter(cw, stream, idx), key)


def codewords(first_cw, B):
    """Global indices of a batch: first_cw + 0 .. B-1, modulo 2^64."""
    return np.uint64(int(first_cw) & (2**64 - 1)) + np.arange(B, dtype=np.uint64)


def bit_draws(K):
    """Draws of stream 1 that one codeword of K info bits consumes (128 bits each)."""
    return (K + 127) // 128


def counters_of_codeword(cw, K, S):
    """Every counter one codeword consumes, as a list of 4-tuples of ints."""
    c = np.concatenate([counter(cw, STREAM_BITS, np.arange(bit_draws(K))), counter(cw, STREAM_H, [0]),
                        counter(cw, STREAM_NOISE, np.arange(S))])
    return [tuple(int(v) for v in row) for row in c]


def source_bits(seed, first_cw, B, K, active=True):
    """Info bits uu[B][K] (uint8) of codewords first_cw .. first_cw + B - 1; all
    zero when the encoder is inactive (the reference's Encoder zeroes uu then)."""
    if not active or B == 0:
        return np.zeros((B, K), np.uint8)
    lanes = draw(seed, codewords(first_cw, B)[:, None], STREAM_BITS, np.arange(bit_draws(K))[None, :])
    lanes = lanes.reshape(B, -1)  # x, y, z, w of draw 0, then of draw 1, ...
    bits = (lanes[:, :, None] >> np.arange(32, dtype=np.uint64)) & np.uint64(1)  # LSB first
    return bits.reshape(B, -1)[:, :K].astype(np.uint8)


def u01(hi, lo):
    """Exact uniform in (0, 1] from two 32-bit lanes, as a Fraction."""
    v = ((int(hi) << 32) | int(lo)) >> 11
    return Fraction(v + 1, 2**53)


def _to_double(x):
    """An mpf rounded to the nearest double (float() of a wide mpf may truncate)."""
    with mpmath.workprec(53):
        return float(+x)


def gauss2_mp(r):
    """Box-Muller pair of one draw r = (x, y, z, w) as two mpf at GAUSS_PREC bits."""
    u1, u2 = u01(r[0], r[1]), u01(r[2], r[3])
    with mpmath.workprec(GAUSS_PREC):
        rad = mpmath.sqrt(-2 * mpmath.log(mpmath.mpf(u1.numerator) / u1.denominator))
        ang = 2 * mpmath.mpf(u2.numerator) / u2.denominator  # exact: 54 bits at most
        return rad * mpmath.cospi(ang), rad * mpmath.sinpi(ang)


def gauss2(r):
    """gauss2_mp rounded to double once."""
    a, b = gauss2_mp(r)
    return _to_double(a), _to_double(b)


def gauss2_fast(r):
    """The same map in numpy float64 over r[..., 4] (statistics only: not exact)."""
    r = np.asarray(r, dtype=np.uint64)
    u1 = ((((r[..., 0] << _32) | r[..., 1]) >> np.uint64(11)) + np.uint64(1)).astype(np.float64) * 2.0**-53
    u2 = ((((r[..., 2] << _32) | r[..., 3]) >> np.uint64(11)) + np.uint64(1)).astype(np.float64) * 2.0**-53
    rad = np.sqrt(-2.0 * np.log(u1))
    return np.stack([rad * np.cos(2 * np.pi * u2), rad * np.sin(2 * np.pi * u2)], axis=-1)


@functools.lru_cache(maxsize=None)
def _gauss_block(seed, first_cw, B, stream, n):
    """gauss2 of draws idx = 0 .. n-1 of a stream of B codewords: float64 [B][n][2]."""
    r = draw(seed, codewords(first_cw, B)[:, None], stream, np.arange(n)[None, :])
    out = np.array([gauss2([int(v) for v in q]) for q in r.reshape(-1, 4)], dtype=np.float64).reshape(B, n, 2)
    out.setflags(write=False)
    return out


def noise_scale(snr):
    """sigma / sqrt 2 of the channel at snr dB, operation for operation as the
    library's channel_constants computes it."""
    return math.sqrt(math.pow(10.0, -0.1 * snr)) / 1.4142135623730950488016


def labels(cc, bits):
    """Constellation index of each symbol of cc[B][cc_len]: `bits` code bits, MSB first."""
    cc = np.asarray(cc, dtype=np.int64)
    B, S = cc.shape[0], cc.shape[1] // bits
    return (cc[:, :S * bits].reshape(B, S, bits) << np.arange(bits - 1, -1, -1)).sum(axis=2)


def _cmul(ar, ai, br, bi):
    """Complex product in individual double operations: four products, one
    difference, one sum."""
    return ar * br - ai * bi, ar * bi + ai * br


def channel_parts(seed, first_cw, cc, bits, cons, snr):
    """h[B][2], y[B][S][2] and scale[B][S][2], the sum of the magnitudes of the
    three terms of each y component (the unit of its error bound)."""
    cc = np.asarray(cc)
    B, S = cc.shape[0], cc.shape[1] // bits
    cons = np.asarray(cons, dtype=np.float64).reshape(-1, 2)
    seed, first_cw = int(seed), int(first_cw)
    h = _gauss_block(seed, first_cw, B, STREAM_H, 1)[:, 0, :] * math.sqrt(0.5)
    n = _gauss_block(seed, first_cw, B, STREAM_NOISE, S)
    x = cons[labels(cc, bits)]
    xr, xi, hr, hi = x[..., 0], x[..., 1], h[:, None, 0], h[:, None, 1]
    tr, ti = _cmul(xr, xi, hr, hi)
    ns = np.float64(noise_scale(snr))
    sr, si = _cmul(n[..., 0], n[..., 1], ns, np.float64(0.0))  # the noise scale is real
    y = np.stack([tr + sr, ti + si], axis=-1)
    scale = np.stack([np.abs(xr * hr) + np.abs(xi * hi) + np.abs(n[..., 0]) * ns,
                      np.abs(xr * hi) + np.abs(xi * hr) + np.abs(n[..., 1]) * ns], axis=-1)
    return h, y, scale


def channel(seed, first_cw, cc, bits, cons, snr):
    """h[B][2] and y[B][S][2] of codewords first_cw .. whose transmitted bits are
    cc[B][cc_len] (ctx.encode(source_bits(...)), or zeros for an inactive encoder)."""
    return channel_parts(seed, first_cw, cc, bits, cons, snr)[:2]
