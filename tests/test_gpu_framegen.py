"""The GPU frame generator (framegen.hip: Philox source bits, encoder, h draw,
mapping, Box-Muller noise) against the exact host model tests/framegen_model.py,
draw for draw.  Run on an MI355X with -m gpu.

Bars:
  * source bits: bit-exact, for every word-count shape of K and for seeds and
    codeword indices that use the high halves of the key and of the counter.
  * h and y: within an error budget derived from the device math library's
    bounds (below), every symbol of every codeword.
  * the two encoder paths, batch splitting and the load / read-back round
    trip: bit-exact.

Error budget.  One unit below is 2^-52 |v|, an upper bound of the ulp of v, so
that "e ulp" of a library bound is a relative error of at most e units and a
correctly rounded operation adds at most 0.5.  The ROCm headers and installed
documents carry no accuracy table for the device math library, so the figures
are the OpenCL full-profile bounds, which the library is built to meet:
log <= 3 ulp, sinpi / cospi <= 4 ulp; sqrt, the products and the sums are
correctly rounded.

  device Gaussian  rad = sqrt(-2 log u1): 3 / 2 (sqrt halves a relative error)
                   + 0.5 = 2;  rad * cospi(2 u2): 2 + 4 + 0.5 = 6.5
                   (u1, u2 and 2 u2 are exact)
  device h         g * sqrt(0.5): 6.5 + 0.5 = 7 from the exact g * fl(sqrt 0.5)
  model h          one rounding of g to double, one product: 1
  h: device against model                                    N_H = 8
  device noise     g * noise_scale: 7 from exact; model 1: 8 units of |n| * noise_scale
  x * h            each product xr * hr: 8 (h) + 0.5 + 0.5 (the two roundings) = 9
                   units of itself; their difference: + 0.5 + 0.5 units of at
                   most |xr hr| + |xi hi|: 10
  y = x h + n      + 0.5 + 0.5 units of at most the sum of the three
                   magnitudes: 11 for the x h terms, 9 for the noise term
  y: device against model, in units of
     2^-52 (|xr hr| + |xi hi| + |n| noise_scale)              N_Y = 11
(second-order terms are below 1e-14 of a unit).  The bound on y is absolute
because the three terms can cancel.  Where the model's h component is an exact
zero (a half-integer angle) the unit is the other component's magnitude.

Measured on an MI355X, maximum over all cases below: h 1.38 units, y 1.91
units (each case prints its own; run with -s).
"""
import os

import numpy as np
import pytest

import framegen_model as M

import kmldpc_amd as K

pytestmark = pytest.mark.gpu

N_H, N_Y = 8.0, 11.0
UNIT = 2.0**-52

PEG2304 = ("PEG2304regular0.5.txt", "2bits_QPSK.txt", False)
BG2 = ("5GLDPCBG2a3_R12_K960.txt", "4bit_16QAM_Gray.txt", True)
PEG8064 = ("PEG8064regular0.5.txt", "6bits_64QAM_Gray.txt", False)
IRR_QPSK = ("syn_irr1200.txt", "2bits_QPSK.txt", False)
IRR_64 = ("syn_irr1200.txt", "6bits_64QAM_Gray.txt", False)
REG192 = ("syn_reg36_192.txt", "2bits_QPSK.txt", False)
REG240 = ("syn_reg48_240.txt", "4bit_16QAM_Gray.txt", False)
HIGH120 = ("syn_high120.txt", "2bits_QPSK.txt", False)
# the synthetic constellations (tests/golden/make_cons.py): bits = 1 and 3 in channel_kernel
REG192_BPSK = ("syn_reg36_192.txt", "syn_1bit_BPSK.txt", False)
HIGH120_8PSK = ("syn_high120.txt", "syn_3bits_8PSK_Gray.txt", False)  # S = 40

SEED_HI = 0xDEADBEEF00000011  # both key words in use
SEED_HI1 = 0x0000000100000011  # differs from 0x11 in the high key word only

_ctx = {}


def ctx_for(data_dir, code, active=True):
    key = code + (active,)
    if key not in _ctx:
        matrix, modem, is5g = code
        _ctx[key] = K.Context(matrix_file=os.path.join(data_dir, matrix), modem_file=os.path.join(data_dir, modem),
                              is5g=is5g, active=active, max_iter=1, device=0)
    return _ctx[key]


def frames(ctx, snr, B, seed, first_cw):
    ctx.sim_generate(snr, B, seed=seed, first_cw=first_cw)
    return ctx.sim_frames(B)


def _ids(v):
    return v[0][:-4] if isinstance(v, tuple) else str(v)


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- a. source bits

# K = 1152: 18 words (even); 960: 15 (odd); 600: 10 with a 24-bit tail; 96: 2 with a
# 32-bit tail; 60: one partial word
SOURCE_CODES = [(PEG2304, 1152), (BG2, 960), (IRR_QPSK, 600), (REG192, 96), (HIGH120, 60)]
SOURCE_POINTS = [(17, 0), (SEED_HI, 77), (SEED_HI1, 77), (9, 2**32 - 3), (9, 2**63 + 5)]


@pytest.mark.parametrize("seed,first_cw", SOURCE_POINTS, ids=hex)
@pytest.mark.parametrize("code,k", SOURCE_CODES, ids=_ids)
def test_source_bits_equal_the_model(data_dir, code, k, seed, first_cw):
    ctx = ctx_for(data_dir, code)
    assert ctx.K == k
    B = 8  # from 2^32 - 3 the batch crosses the carry into the high counter word
    uu, _, _ = frames(ctx, 2.0, B, seed, first_cw)
    assert np.array_equal(uu, M.source_bits(seed, first_cw, B, ctx.K))


@pytest.mark.parametrize("code", [PEG2304, HIGH120], ids=_ids)
def test_high_counter_and_key_words_reach_the_frames(data_dir, code):
    """Codewords 2^32 apart, and seeds that differ only in the high word, get different frames."""
    ctx = ctx_for(data_dir, code)
    B = 4
    a = frames(ctx, 2.0, B, 9, 5)
    b = frames(ctx, 2.0, B, 9, 2**32 + 5)
    c = frames(ctx, 2.0, B, 0x11, 5)
    d = frames(ctx, 2.0, B, SEED_HI1, 5)
    for p, q in ((a, b), (c, d)):
        for i in range(B):  # every codeword's bits, noise and h
            assert not np.array_equal(p[0][i], q[0][i])
            assert not np.array_equal(p[1][i], q[1][i]) and not np.array_equal(p[2][i], q[2][i])


# ---- b. h and y

CHANNEL_CASES = [(PEG2304, 4), (BG2, 4), (PEG8064, 4), (REG240, 16), (IRR_64, 8), (REG192_BPSK, 16), (HIGH120_8PSK, 16)]
CHANNEL_SEED, CHANNEL_FIRST = SEED_HI, 2**32 + 77
measured = {"h": 0.0, "y": 0.0}


def check_channel(ctx, got, want, snr, what):
    """h and y of the device within N_H / N_Y units of the model's; prints the maxima."""
    (_, y, h), (h_m, y_m, scale) = got, want
    assert np.isfinite(h).all() and np.isfinite(y).all()
    unit_h = np.where(h_m != 0.0, np.abs(h_m), np.abs(h_m[:, ::-1]))
    eh = (np.abs(h - h_m) / (UNIT * unit_h)).max()
    ey = (np.abs(y - y_m) / (UNIT * scale)).max()
    measured["h"], measured["y"] = max(measured["h"], eh), max(measured["y"], ey)
    print(f"{what} snr {snr}: max error h {eh:.3f} of {N_H} units, y {ey:.3f} of {N_Y} units "
          f"(running maxima h {measured['h']:.3f}, y {measured['y']:.3f})")
    assert eh <= N_H and ey <= N_Y


@pytest.mark.parametrize("snr", [2.0, 60.0])
@pytest.mark.parametrize("code,B", CHANNEL_CASES, ids=_ids)
def test_channel_equals_the_model(data_dir, code, B, snr):
    ctx = ctx_for(data_dir, code)
    got = frames(ctx, snr, B, CHANNEL_SEED, CHANNEL_FIRST)
    uu = M.source_bits(CHANNEL_SEED, CHANNEL_FIRST, B, ctx.K)
    assert np.array_equal(got[0], uu)
    want = M.channel_parts(CHANNEL_SEED, CHANNEL_FIRST, ctx.encode(uu), ctx.bits, ctx.constellation(), snr)
    assert want[1].shape == (B, ctx.S, 2)
    check_channel(ctx, got, want, snr, code[0])
    if snr == 60.0:  # the noise is far below half the minimum distance: y / h decides every label
        pts = ctx.constellation()
        x = (got[1][..., 0] + 1j * got[1][..., 1]) / (got[2][:, 0] + 1j * got[2][:, 1])[:, None]
        lab = np.abs(x[:, :, None] - (pts[:, 0] + 1j * pts[:, 1])[None, None, :]).argmin(axis=2)
        assert np.array_equal(lab, M.labels(ctx.encode(uu), ctx.bits))


# ---- c. inactive encoder

@pytest.mark.parametrize("code,B", [(PEG2304, 4), (IRR_64, 8)], ids=_ids)
def test_inactive_encoder(data_dir, code, B):
    """active = 0: uu is all zero and every symbol is constellation point 0; h and
    the noise still follow their streams."""
    ctx = ctx_for(data_dir, code, active=False)
    got = frames(ctx, 2.0, B, CHANNEL_SEED, CHANNEL_FIRST)
    assert not got[0].any() and not M.source_bits(CHANNEL_SEED, CHANNEL_FIRST, B, ctx.K, active=False).any()
    zeros = np.zeros((B, ctx.cc_len), np.uint8)
    want = M.channel_parts(CHANNEL_SEED, CHANNEL_FIRST, zeros, ctx.bits, ctx.constellation(), 2.0)
    check_channel(ctx, got, want, 2.0, code[0] + " inactive")
    # the same draws as the active encoder's: h is bit-identical to it
    act = frames(ctx_for(data_dir, code), 2.0, B, CHANNEL_SEED, CHANNEL_FIRST)
    assert same_bits(got[2], act[2])


# ---- d. both encoder paths

@pytest.mark.parametrize("code", [PEG2304, BG2, PEG8064], ids=_ids)
def test_aligned_and_per_lane_encoders_agree(data_dir, code, monkeypatch):
    """The aligned encoder kernels (the default for these codes) and the
    one-lane-per-bit kernel (KML_ENCODE_LANE, read at every launch) give
    bit-identical frames: one full 64-codeword tile and a tail of one."""
    ctx = ctx_for(data_dir, code)
    B, seed, first = 65, SEED_HI1, 2**32 - 33
    monkeypatch.delenv("KML_ENCODE_LANE", raising=False)
    a = frames(ctx, 2.0, B, seed, first)
    monkeypatch.setenv("KML_ENCODE_LANE", "1")
    b = frames(ctx, 2.0, B, seed, first)
    for p, q in zip(a, b):
        assert same_bits(p, q)
    assert np.array_equal(a[0], M.source_bits(seed, first, B, ctx.K))


# ---- e. batch invariance and edges

@pytest.mark.parametrize("code", [PEG2304, IRR_64, BG2], ids=_ids)
def test_one_codeword_alone_equals_its_row_of_a_batch(data_dir, code):
    ctx = ctx_for(data_dir, code)
    B, seed, first = 8, 9, 2**32 - 3
    whole = frames(ctx, 2.0, B, seed, first)
    for i in (0, 2, 3, 7):  # 3 is the first codeword past the carry
        one = frames(ctx, 2.0, 1, seed, first + i)
        for p, q in zip(whole, one):
            assert same_bits(p[i:i + 1], q)


def test_empty_batch(data_dir):
    ctx = ctx_for(data_dir, REG192)
    frames(ctx, 2.0, 3, 1, 0)
    uu, y, h = frames(ctx, 2.0, 0, 1, 0)
    assert uu.shape == (0, ctx.K) and y.shape == (0, ctx.S, 2) and h.shape == (0, 2)
    c = ctx.sim_decode(2.0, blind=False)
    assert c["tot_blk"] == 0 and c["tot_bit"] == 0 and c["err_bit"] == 0


@pytest.mark.parametrize("code", [IRR_QPSK, HIGH120, REG240, REG192_BPSK], ids=_ids)
def test_load_then_frames_round_trip(data_dir, code):
    """kml_sim_load then kml_sim_frames gives back the frames bit for bit for K off
    the 64-bit grid (600, 60, 121, 96): the tail word's packing and unpacking agree."""
    ctx = ctx_for(data_dir, code)
    assert ctx.K % 64 != 0
    rng = np.random.default_rng(4)
    B = 5
    uu = rng.integers(0, 2, (B, ctx.K)).astype(np.uint8)
    uu[0], uu[1] = 1, 0  # all ones fills the tail word up to bit K - 1 and no further
    y, h = rng.normal(size=(B, ctx.S, 2)), rng.normal(size=(B, 2))
    y[0, 0], h[0] = (-0.0, 5e-324), (np.inf, -1.0)  # raw bit patterns survive
    ctx.sim_load(2.0, uu, y, h, first_cw=2**32 + 1)
    for p, q in zip(ctx.sim_frames(B), (uu, y, h)):
        assert same_bits(p, q)
