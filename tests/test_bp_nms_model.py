"""The normalized min-sum contract (tests/bp_nms_model.py) decodes: CPU checks
of the model itself, on the 5G BG2 K960 code and on syn_irr1200 (the two codes
of tests/test_gpu_nms.py, which holds the GPU kernel to the model bit for bit).

The streams, the model's decodes of them and the random-prior codewords are
made once per session and shared with the GPU tests (read-only).
"""
import math
import os

import numpy as np
import pytest

from bp_nms_model import CLAMP, Graph, nms_model, priors
from oracle import oracle as O

# name: (matrix, is5g, max_iter, modem of the stream, snr of the stream)
# The SNRs come from a scan of the model over 128 seed-17 codewords (share
# converged: bg2 5 dB 0.20, 6 dB 0.31, 7 dB 0.38, 8 dB 0.47, 9 dB 0.58;
# syn_irr1200 10 dB 0.18, 12 dB 0.34, 14 dB 0.52, 16 dB 0.68, 18 dB 0.79).
CODES = {
    "bg2": ("5GLDPCBG2a3_R12_K960.txt", True, 50, "4bit_16QAM_Gray.txt", 7.0),
    "syn_irr1200": ("syn_irr1200.txt", False, 20, "6bits_64QAM_Gray.txt", 14.0),
}
N_STREAM = 128
MIN_SHARE = 0.10  # each stream holds at least this share of converged and of failed codewords (a condition)

_cache = {}


def code(data_dir, name):
    """(oracle code, model graph) of a code, made once."""
    key = ("code", data_dir, name)
    if key not in _cache:
        matrix, is5g, max_iter, _, _ = CODES[name]
        oc = O.Code(os.path.join(data_dir, matrix), is5g, True, False, max_iter)
        _cache[key] = (oc, Graph(oc))
    return _cache[key]


def stream(data_dir, name, n=N_STREAM):
    """The first n seed-17 codewords of the code's stream: frames and the oracle's P0 (read-only)."""
    key = ("stream", data_dir, name, n)
    if key not in _cache:
        _, _, _, modem, snr = CODES[name]
        oc, _ = code(data_dir, name)
        om = O.Modem(os.path.join(data_dir, modem))
        uu, cc, th, y = O.gen_frames(oc, om, snr, n)
        var = 10.0 ** (-0.1 * snr)
        p0 = np.stack([om.demap(y[i], th[i], var) for i in range(n)])
        for a in (uu, cc, th, y, p0):
            a.setflags(write=False)
        _cache[key] = dict(uu=uu, cc=cc, th=th, y=y, p0=p0, snr=snr, modem=modem)
    return _cache[key]


def random_p0(data_dir, name="bg2", n=16):
    """n codewords of uniform-random P0 in (0, 1): they never converge and drive the messages into the clamp."""
    key = ("random", data_dir, name, n)
    if key not in _cache:
        oc, _ = code(data_dir, name)
        p0 = np.random.default_rng(20240607).random((n, oc.cc_len))
        p0.setflags(write=False)
        _cache[key] = p0
    return _cache[key]


def saturated_p0(data_dir, name="bg2"):
    """16 codewords of saturated priors: P0 of exactly 0, 1, 0.5 and 1e-300.
    0-7: an encoded codeword as P0 in {0, 1} with 120 entries inverted (|L| = 27.6 on every column: the
    messages reach the +-256 clamp within a few iterations, and the decode still converges);
    8-11: the same with 200 inverted (too many: the full budget); 12: the all-0.5 codeword;
    13: a codeword with a quarter of its entries at 0.5; 14: with its zeros written as 1e-300;
    15: every entry drawn from {0, 1, 0.5, 1e-300}."""
    key = ("saturated", data_dir, name)
    if key not in _cache:
        oc, _ = code(data_dir, name)
        rng = np.random.default_rng(77)
        uu = rng.integers(0, 2, (16, oc.K)).astype(np.int32)
        cc = np.stack([oc.encode(u) for u in uu])
        p0 = np.where(cc == 0, 1.0, 0.0)
        for b in range(12):
            idx = rng.choice(oc.cc_len, 120 if b < 8 else 200, replace=False)
            p0[b, idx] = 1.0 - p0[b, idx]
        p0[12] = 0.5
        p0[13, rng.random(oc.cc_len) < 0.25] = 0.5
        p0[14] = np.where(p0[14] == 0.0, 1.0e-300, p0[14])
        p0[15] = rng.choice(np.array([0.0, 1.0, 0.5, 1.0e-300]), oc.cc_len)
        p0.setflags(write=False)
        _cache[key] = p0
    return _cache[key]


def model_decode(data_dir, name, p0_key, p0, iter_count, alpha=0.75):
    """The model's decode of a named input at a budget (read-only, made once)."""
    key = ("dec", data_dir, name, p0_key, iter_count, float(np.float32(alpha)))
    if key not in _cache:
        _, g = code(data_dir, name)
        stats = {}
        ret, uh, cch = nms_model(g, p0, iter_count, CODES[name][2], alpha, stats=stats)
        for a in (ret, uh, cch):
            a.setflags(write=False)
        _cache[key] = dict(ret=ret, uu_hat=uh, cc_hat=cch, stats=stats)
    return _cache[key]


def raw_info_bits(g, p0):
    """The hard decisions of the priors alone (a punctured column decides 1, the tie), info bits."""
    hard = np.where(priors(g, p0) > 0, 0, 1).astype(np.uint8)
    return hard[:, g.info_off:g.info_off + g.K]


# ---- tests -----------------------------------------------------------------

@pytest.mark.parametrize("name", list(CODES))
def test_noiseless_codewords_decode(data_dir, name):
    oc, g = code(data_dir, name)
    rng = np.random.default_rng(5)
    uu = rng.integers(0, 2, (8, oc.K)).astype(np.int32)
    cc = np.stack([oc.encode(u) for u in uu])
    p0 = np.where(cc == 0, 0.95, 0.05)
    max_iter = CODES[name][2]
    ret, uh, cch = nms_model(g, p0, max_iter, max_iter)
    assert np.array_equal(uh, uu.astype(np.uint8))
    assert np.array_equal(cch[:, g.punct:], cc.astype(np.uint8))
    if name == "bg2":  # the punctured columns start undecided: a few iterations fill them in
        assert ret.min() >= 2 and ret.max() <= 5
    else:              # every row is satisfied by the first VN phase's decisions
        assert np.all(ret == 1)


@pytest.mark.parametrize("name", list(CODES))
def test_noisy_stream_decodes_and_has_both_outcomes(data_dir, name):
    oc, g = code(data_dir, name)
    s = stream(data_dir, name)
    max_iter = CODES[name][2]
    d = model_decode(data_dir, name, "stream", s["p0"], max_iter)
    uu = s["uu"].astype(np.uint8)
    raw = int((raw_info_bits(g, s["p0"]) != uu).sum())
    dec = int((d["uu_hat"] != uu).sum())
    failed = float(np.mean(d["ret"] == max_iter))
    print(f"{name}: info-bit errors raw {raw} -> decoded {dec}; failed {failed:.3f}")
    assert dec < raw
    assert failed >= MIN_SHARE and 1.0 - failed >= MIN_SHARE, f"stream is one-sided: {failed:.3f} failed"
    # a converged codeword satisfies every check, and the stop rule is the only way below the budget
    conv = d["ret"] < max_iter
    assert all(oc.parity_count(c) == 0 for c in d["cc_hat"][conv])
    assert d["stats"]["finite"]


@pytest.mark.parametrize("name", list(CODES))
def test_alpha_changes_the_decode(data_dir, name):
    s = stream(data_dir, name)
    max_iter = CODES[name][2]
    a = model_decode(data_dir, name, "stream", s["p0"], max_iter, 0.75)
    b = model_decode(data_dir, name, "stream", s["p0"], max_iter, 1.0)
    assert (a["cc_hat"] != b["cc_hat"]).any(axis=1).any()


def test_random_priors_never_converge_and_stay_finite(data_dir):
    """Uniform-random P0 runs the full 50 iterations.  Under this contract its messages stay small (the
    largest |v2c| of these 16 codewords is 14.84 at alpha 0.75 and 15.68 at alpha 1: a check node passes on
    its weakest input), so it is the saturated priors below, not these, that reach the clamp."""
    p0 = random_p0(data_dir)
    d = model_decode(data_dir, "bg2", "random", p0, 50)
    assert np.all(d["ret"] == 50)  # never converged: iter = max_iter
    assert d["stats"]["finite"]
    assert 8.0 < d["stats"]["max_abs_v2c"] < 32.0  # 14.84 at alpha 0.75: far below the clamp at 256
    _, g = code(data_dir, "bg2")
    stats = {}
    nms_model(g, p0, 50, 50, 1.0, stats=stats)
    assert stats["finite"] and 8.0 < stats["max_abs_v2c"] < 32.0  # 15.68 at alpha 1


def test_saturated_priors_reach_the_clamp_and_stay_finite(data_dir):
    """P0 of exactly 0 or 1 is |L| = 27.6; a degree-9 column sums to 248 in one VN phase and to the
    clamp in the next.  Unclamped, 50 such iterations pass FLT_MAX."""
    p0 = saturated_p0(data_dir)
    d = model_decode(data_dir, "bg2", "saturated", p0, 50)
    assert d["stats"]["max_abs_v2c"] == float(CLAMP)
    assert d["stats"]["finite"]
    assert np.all(d["ret"][:8] < 50) and np.all(d["ret"][8:13] == 50)
    _, g = code(data_dir, "bg2")
    L = priors(g, p0)
    # P0 = 1: q = 1 - 1e-12, and 1 - q is the float64 difference, not 1e-12 itself
    hi = 1.0 - 1.0e-12
    assert np.isfinite(L).all() and float(L.max()) == float(np.float32(math.log(hi) - math.log(1.0 - hi)))
    assert float(L.min()) == float(np.float32(math.log(1.0e-12) - math.log(1.0 - 1.0e-12)))
    assert not L[12].any() and not np.signbit(L[12]).any()  # the all-0.5 codeword: every prior +0


@pytest.mark.parametrize("name", list(CODES))
def test_row_order_changes_nothing(data_dir, name):
    _, g = code(data_dir, name)
    s = stream(data_dir, name)
    max_iter = CODES[name][2]
    a = model_decode(data_dir, name, "stream", s["p0"], max_iter)
    ret, uh, cch = nms_model(g, s["p0"][:32], max_iter, max_iter, reverse_rows=True)
    assert np.array_equal(ret, a["ret"][:32])
    assert np.array_equal(uh, a["uu_hat"][:32])
    assert np.array_equal(cch, a["cc_hat"][:32])
