"""The binary16 layered min-sum contract (tests/bp_h16_model.py): CPU checks of the
model itself, on the three codes and the seed-17 streams of
tests/test_bp_lnms_model.py (BG2 + 16QAM 7 dB, syn_irr1200 + 64QAM 14 dB,
syn_qc_l200 + QPSK 3 dB; 128 codewords each).  tests/test_gpu_h16.py holds the
GPU kernel to the model bit for bit.  The model's decodes are made once per
session and shared with the GPU tests (read-only).
"""
import numpy as np
import pytest

import test_bp_lnms_model as LF
import test_bp_nms_model as F
from bp_h16_model import (CLAMP16, alpha16, h16_llr_priors, h16_priors, lnms_h16_llr_model, lnms_h16_model,
                          lnms_h16_rowwise)
from bp_nms_model import priors

CODES = LF.CODES
MIN_SHARE = F.MIN_SHARE

_cache = {}


def h16_decode(data_dir, name, p0_key, p0, iter_count, alpha=0.75):
    """The binary16 model's decode of a named P0 input at a budget (read-only, made once)."""
    key = (data_dir, name, p0_key, iter_count, float(np.float32(alpha)))
    if key not in _cache:
        _, g = LF.code(data_dir, name)
        stats = {}
        ret, uh, cch = lnms_h16_model(g, p0, iter_count, CODES[name][2], alpha, stats=stats)
        for a in (ret, uh, cch):
            a.setflags(write=False)
        _cache[key] = dict(ret=ret, uu_hat=uh, cc_hat=cch, stats=stats)
    return _cache[key]


def h16_llr_decoded(data_dir, name, llr_key, llr, iter_count, alpha=0.75):
    """The binary16 LLR-prior model's decode of a named input at a budget (read-only, made once)."""
    key = ("llr", data_dir, name, llr_key, iter_count, float(np.float32(alpha)))
    if key not in _cache:
        _, g = LF.code(data_dir, name)
        stats = {}
        ret, uh, cch, T = lnms_h16_llr_model(g, llr, iter_count, CODES[name][2], alpha, stats=stats)
        for a in (ret, uh, cch, T):
            a.setflags(write=False)
        _cache[key] = dict(ret=ret, uu_hat=uh, cc_hat=cch, llr_out=T, stats=stats)
    return _cache[key]


# ---- the model against the contract as written -----------------------------

@pytest.mark.parametrize("alpha", [0.75, 1.0])
@pytest.mark.parametrize("name", list(CODES))
def test_vectorised_model_equals_the_row_by_row_loop(data_dir, name, alpha):
    """4 stream codewords, 8 sweeps: bit for bit."""
    _, g = LF.code(data_dir, name)
    p0 = LF.stream(data_dir, name)["p0"][:4]
    max_iter = CODES[name][2]
    a = lnms_h16_model(g, p0, 8, max_iter, alpha)
    b = lnms_h16_rowwise(g, p0, 8, max_iter, alpha)
    for x, y, what in zip(a, b, ("ret", "uu_hat", "cc_hat")):
        assert np.array_equal(x, y), what


@pytest.mark.parametrize("name", list(CODES))
def test_noiseless_codewords_decode(data_dir, name):
    """Priors whose decisions satisfy every check stop before any sweep: ret = 1.  BG2's punctured columns
    start at the tie, so there a sweep or two comes first, as in the f32 model's test."""
    oc, g = LF.code(data_dir, name)
    rng = np.random.default_rng(5)
    uu = rng.integers(0, 2, (8, oc.K)).astype(np.int32)
    cc = np.stack([oc.encode(u) for u in uu])
    p0 = np.where(cc == 0, 0.95, 0.05)
    max_iter = CODES[name][2]
    ret, uh, cch = lnms_h16_model(g, p0, max_iter, max_iter)
    assert np.array_equal(uh, uu.astype(np.uint8))
    assert np.array_equal(cch[:, g.punct:], cc.astype(np.uint8))
    if name == "bg2":  # the punctured columns start undecided: a sweep or two fills them in (as in f32)
        assert ret.min() >= 2 and ret.max() <= 4
    else:
        assert np.all(ret == 1)


# ---- error rate: the pinned table and the condition -------------------------

# stream: (budgets, f32 layered FER, binary16 layered FER), 128 codewords, alpha 0.75
FER_TABLE = {
    "bg2": ((50, 25, 5), (0.6172, 0.6172, 0.7344), (0.6094, 0.6172, 0.7344)),
    "syn_irr1200": ((20, 10, 5), (0.4766, 0.4922, 0.5938), (0.4766, 0.4922, 0.5938)),
    LF.QC: ((20, 10, 5), (0.5391, 0.5625, 0.5859), (0.5391, 0.5625, 0.5859)),
}
TOP_T = {"bg2": 153.25, "syn_irr1200": 284.0, LF.QC: 105.125}


@pytest.mark.parametrize("name", list(FER_TABLE))
def test_fer_table(data_dir, name):
    """Deterministic CPU results: other values mean the contract was built differently.  The condition beside
    the pinned figures: binary16 FER <= f32 FER + 2/128 on every row (a failing decode's bits are arbitrary,
    so two codewords of slack)."""
    budgets, f32, f16 = FER_TABLE[name]
    s = LF.stream(data_dir, name)
    uu = s["uu"]
    top = 0.0
    for b, e32, e16 in zip(budgets, f32, f16):
        d32 = LF.layered_decode(data_dir, name, "stream", s["p0"], b)
        d16 = h16_decode(data_dir, name, "stream", s["p0"], b)
        g32, g16 = LF.fer(d32, uu), LF.fer(d16, uu)
        diff = int((d32["ret"] != d16["ret"]).sum())
        print(f"{name}@{b}: f32 {g32:.4f} binary16 {g16:.4f} ret differs on {diff} max|T| {d16['stats']['max_abs_T']}")
        assert g16 <= g32 + 2.0 / 128.0
        assert (round(g32, 4), round(g16, 4)) == (e32, e16)
        assert diff <= 3
        top = max(top, d16["stats"]["max_abs_T"])
    assert top == TOP_T[name]


@pytest.mark.parametrize("name", list(CODES))
def test_stream_has_both_outcomes(data_dir, name):
    oc, g = LF.code(data_dir, name)
    s = LF.stream(data_dir, name)
    max_iter = CODES[name][2]
    d = h16_decode(data_dir, name, "stream", s["p0"], max_iter)
    conv = d["stats"]["converged"]
    print(f"{name}: converged {conv.mean():.3f}")
    assert conv.mean() >= MIN_SHARE and 1.0 - conv.mean() >= MIN_SHARE
    assert all(oc.parity_count(c) == 0 for c in d["cc_hat"][conv])
    assert d["stats"]["finite"]


# ---- the roundings ----------------------------------------------------------

def _h16_of_llr(g, vals):
    x = np.zeros((1, g.cc_len), np.float32)
    x[0, :len(vals)] = np.array(vals, np.float32)
    return h16_llr_priors(g, x)[0, g.punct:g.punct + len(vals)]


def test_prior_rounding(data_dir):
    _, g = LF.code(data_dir, "bg2")
    bits = lambda a: np.asarray(a, np.float16).view(np.uint16).tolist()
    # ties to even: 1 + 2^-11 is halfway between 1 (0x3C00, even) and 1 + 2^-10; 1 + 3 * 2^-11 goes up to 0x3C02
    assert bits(_h16_of_llr(g, [1.0 + 2.0 ** -11, 1.0 + 3.0 * 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -20])) == \
        [0x3C00, 0x3C02, 0x3C01]
    # half denormals are kept: 2^-24 is the smallest (0x0001), 2^-25 ties to even 0, 1.5 * 2^-25 rounds up,
    # 3 * 2^-24 is 0x0003, and a float denormal rounds to a zero of its sign
    assert bits(_h16_of_llr(g, [2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, 3.0 * 2.0 ** -24, -2.0 ** -24, -1e-40])) == \
        [0x0001, 0x0000, 0x0001, 0x0003, 0x8001, 0x8000]
    # the clamp comes first, in float: +-256 exactly, whatever lay beyond; 255.95 rounds up to it (the halves
    # below 256 are 0.125 apart), 255.9 does not
    assert bits(_h16_of_llr(g, [256.0, -256.0, 256.5, -1e30, np.inf, -np.inf, 255.95, 255.9])) == \
        [0x5C00, 0xDC00, 0x5C00, 0xDC00, 0x5C00, 0xDC00, 0x5C00, 0x5BFF]
    # +-0 keep their sign; a punctured column is +0
    assert bits(_h16_of_llr(g, [0.0, -0.0])) == [0x0000, 0x8000]
    assert g.punct > 0 and not h16_llr_priors(g, np.full((1, g.cc_len), -3.0, np.float32))[0, :g.punct].view(np.uint16).any()
    # alpha: to float first, then to half; 0.75, 0.8125 and 1 are exact
    assert [float(alpha16(a)) for a in (0.75, 0.8125, 1.0)] == [0.75, 0.8125, 1.0]
    assert alpha16(0.8) == np.float16(np.float32(0.8)) and float(alpha16(1e-9)) == 0.0


def test_values_stay_finite_and_bounded(data_dir):
    """|T| <= 512: T = m + c2v with |m| <= 256 and |c2v| <= a16 * 256 <= 256."""
    for key, p0 in (("saturated", F.saturated_p0(data_dir)), ("random", F.random_p0(data_dir))):
        for alpha in (0.75, 1.0):
            d = h16_decode(data_dir, "bg2", key, p0, 50, alpha)
            assert d["stats"]["finite"] and d["stats"]["max_abs_T"] <= 512.0
    sat = h16_decode(data_dir, "bg2", "saturated", F.saturated_p0(data_dir), 50)
    assert sat["stats"]["max_abs_m"] == float(CLAMP16)


@pytest.mark.parametrize("name", list(CODES))
def test_llr_model_on_the_p0_priors_is_the_p0_model(data_dir, name):
    _, g = LF.code(data_dir, name)
    p0 = LF.stream(data_dir, name)["p0"][:16]
    max_iter = CODES[name][2]
    L = priors(g, p0)  # float32, |L| < 28: the LLR clamp changes nothing
    a = lnms_h16_model(g, p0, 8, max_iter)
    b = lnms_h16_llr_model(g, L[:, g.punct:], 8, max_iter)
    for x, y, what in zip(a, b[:3], ("ret", "uu_hat", "cc_hat")):
        assert np.array_equal(x, y), what
    assert np.array_equal(h16_priors(g, p0).view(np.uint16), h16_llr_priors(g, L[:, g.punct:]).view(np.uint16))
    T = b[3]
    assert T.dtype == np.float32 and np.array_equal(T.astype(np.float16).astype(np.float32), T)
    assert np.array_equal(np.where(T > 0, 0, 1).astype(np.uint8), b[2])


def test_ret_semantics(data_dir):
    _, g = LF.code(data_dir, "bg2")
    s = LF.stream(data_dir, "bg2")
    p0 = s["p0"][:16]
    full = h16_decode(data_dir, "bg2", "stream", s["p0"], 50)
    assert np.any(full["ret"][:16] == 50) and np.any(full["ret"][:16] < 50)
    ret, uh, cch = lnms_h16_model(g, p0, 0, 50)  # no sweep: it = 0, outputs as passed (zeros here)
    assert np.all(ret == 1) and not uh.any() and not cch.any()
    ret, uh, cch = lnms_h16_model(g, p0, 1, 50)
    assert np.all(ret == 2) and cch.any()
    ret, _, _ = lnms_h16_model(g, p0, 50, 50)    # it = max_iter is not incremented
    assert np.array_equal(ret, full["ret"][:16])
    ret5, _, _ = lnms_h16_model(g, p0, 5, 50)
    assert np.array_equal(ret5, np.minimum(full["stats"]["iters"][:16], 5) + 1)
