"""The offset-correction contract (tests/bp_oms_model.py): CPU checks of the model
itself on 5G BG2 K960, syn_irr1200 and syn_qc_l200 (the three codes of
tests/test_gpu_oms.py, which holds the GPU kernels to the model bit for bit).

The streams are test_bp_lnms_model.py's seed-17 streams (BG2 7 dB, syn_irr1200
14 dB, syn_qc_l200 3 dB); the model's decodes are made once per session and
shared with the GPU tests (read-only).
"""
from types import SimpleNamespace

import numpy as np
import pytest

import test_bp_lnms_model as L
import test_bp_nms_model as F
from bp_h16_model import lnms_h16_llr_model, lnms_h16_model
from bp_llr_model import llr_decode_model
from bp_lnms_model import lnms_model
from bp_nms_model import CLAMP, nms_model
from bp_oms_model import (beta16, oms_cn_phase, oms_decode, oms_h16_model, oms_llr_model, oms_lnms_model,
                          oms_lnms_rowwise, oms_mag, oms_mag16, oms_nms_model)

CODES = L.CODES
PAIRS = ((0.75, 0.0), (1.0, 0.5), (1.0, 0.0))
_cache = {}


def oms_decoded(data_dir, name, p0_key, p0, iter_count, alpha, beta, schedule="layered", messages="f32"):
    """The model's decode of a named input at a budget (read-only, made once)."""
    key = (data_dir, name, p0_key, iter_count, float(np.float32(alpha)), float(np.float32(beta)), schedule, messages)
    if key not in _cache:
        _, g = L.code(data_dir, name)
        stats = {}
        ret, uh, cch = oms_decode(g, p0, iter_count, CODES[name][2], alpha, beta, schedule, messages, stats=stats)
        for a in (ret, uh, cch):
            a.setflags(write=False)
        _cache[key] = dict(ret=ret, uu_hat=uh, cc_hat=cch, stats=stats)
    return _cache[key]


def failed(d, uu):
    return int((d["uu_hat"] != uu.astype(np.uint8)).any(axis=1).sum())


# ---- beta = 0 is the shipped contract ----------------------------------------

@pytest.mark.parametrize("alpha", [0.75, 1.0])
@pytest.mark.parametrize("name", list(CODES))
def test_beta_zero_equals_the_shipped_models(data_dir, name, alpha):
    """4 stream codewords, 8 sweeps or iterations: bit for bit, all three contracts and the LLR front end."""
    _, g = L.code(data_dir, name)
    p0 = L.stream(data_dir, name)["p0"][:4]
    mx = CODES[name][2]
    pairs = [(oms_nms_model(g, p0, 8, mx, alpha, 0.0), nms_model(g, p0, 8, mx, alpha)),
             (oms_lnms_model(g, p0, 8, mx, alpha, 0.0), lnms_model(g, p0, 8, mx, alpha)),
             (oms_h16_model(g, p0, 8, mx, alpha, 0.0), lnms_h16_model(g, p0, 8, mx, alpha))]
    llr = np.random.default_rng(3).normal(0.0, 6.0, (4, g.cc_len)).astype(np.float32)
    for sched in ("flooding", "layered"):
        pairs.append((oms_llr_model(g, llr, 8, mx, alpha, 0.0, sched), llr_decode_model(g, llr, 8, mx, alpha, sched)))
    pairs.append((oms_llr_model(g, llr, 8, mx, alpha, 0.0, "layered", "f16"), lnms_h16_llr_model(g, llr, 8, mx, alpha)))
    for k, (a, b) in enumerate(pairs):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)), k  # (T: -0 and +0 differ)


@pytest.mark.parametrize("name", list(CODES))
def test_vectorised_model_equals_the_row_by_row_loop(data_dir, name):
    _, g = L.code(data_dir, name)
    p0 = L.stream(data_dir, name)["p0"][:4]
    mx = CODES[name][2]
    a = oms_lnms_model(g, p0, 8, mx, 1.0, 0.5)
    b = oms_lnms_rowwise(g, p0, 8, mx, 1.0, 0.5)
    for x, y, what in zip(a, b, ("ret", "uu_hat", "cc_hat")):
        assert np.array_equal(x, y), what


# ---- the rule itself, on hand-made rows ---------------------------------------

def _row(d):
    return SimpleNamespace(cn_groups=[(d, np.arange(d)[None, :])])


def test_small_products_give_a_zero_magnitude_with_the_xors_sign():
    v2c = np.array([[0.25, -3.0, 0.5, -7.0]], np.float32)
    c = oms_cn_phase(_row(4), v2c, 1.0, 0.5)
    # a = (0.5, 0.25, 0.25, 0.25): every alpha * a <= beta, every magnitude is zero ...
    assert np.array_equal(c.view(np.uint32) & np.uint32(0x7FFFFFFF), np.zeros((1, 4), np.uint32))
    # ... edge 0: 0.5 - 0.5 = +0 exactly; its sign is the XOR of the others' (two negatives: clear)
    # the others see one or two negatives among the rest
    assert np.array_equal(np.signbit(c), np.array([[False, True, False, True]]))
    assert c.view(np.uint32)[0, 1] == 0x80000000  # -0: a legal message
    c = oms_cn_phase(_row(4), v2c, 0.75, 0.125)  # 0.75 * 0.5 - 0.125 = 0.25; 0.75 * 0.25 - 0.125 = 0.0625
    assert np.array_equal(c, np.array([[0.25, -0.0625, 0.0625, -0.0625]], np.float32))


def test_equality_gives_plus_zero():
    assert oms_mag(np.float32(0.5), 1.0, 0.5).view(np.uint32) == 0           # x - x = +0, never -0
    assert oms_mag(np.float32(0.4), 1.0, 0.5).view(np.uint32) == 0           # negative: +0
    assert oms_mag16(np.float16(0.5), 1.0, 0.5).view(np.uint16) == 0
    assert oms_mag16(np.float16(0.25), 1.0, 0.5).view(np.uint16) == 0
    assert oms_mag(np.float32(0.0), 0.75, 0.5).view(np.uint32) == 0          # a = +0
    # one rounding each: RN(alpha * a), then RN(c - b)
    a, al, be = np.float32(1.0000001), np.float32(0.8125), np.float32(0.3)
    want = np.float32(np.float32(al * a) - be)
    assert oms_mag(a, 0.8125, 0.3) == want and oms_mag(a, 0.8125, 0.3).dtype == np.float32
    # a denormal result is kept
    assert oms_mag(np.float32(3.0 * 2.0 ** -140), 1.0, 2.0 ** -140) == np.float32(2.0 ** -139)


def test_binary16_rounding_of_beta():
    assert beta16(0.3).view(np.uint16) == 0x34CD
    assert beta16(0.5).view(np.uint16) == 0x3800 and beta16(0.375).view(np.uint16) == 0x3600
    assert float(np.float32(0.3)) != 0.3 and float(beta16(0.3)) != float(np.float32(0.3))  # inexact in both formats
    # the subtraction is binary16's: 1.0 - RN16(0.3) = 0.7001953125 rounds to a half
    got = oms_mag16(np.float16(1.0), 1.0, 0.3)
    assert got.dtype == np.float16 and got == np.float16(np.float32(1.0) - np.float32(beta16(0.3)))
    assert beta16(2.0 ** -25).view(np.uint16) == 0 and beta16(2.0 ** -24).view(np.uint16) == 1


@pytest.mark.parametrize("schedule,messages", [("flooding", "f32"), ("layered", "f32"), ("layered", "f16")])
def test_values_stay_finite_and_clamped(data_dir, schedule, messages):
    """The saturated and the random priors of test_bp_nms_model.py: |m| <= 256 and reached on the saturated
    ones, every value finite, |T| <= 256 + alpha * 256 (layered), 16 codewords each."""
    for key, p0 in (("saturated", F.saturated_p0(data_dir)), ("random", F.random_p0(data_dir))):
        for alpha, beta in ((1.0, 0.5), (0.8125, 0.375)):
            d = oms_decoded(data_dir, "bg2", key, p0, 50, alpha, beta, schedule, messages)
            st = d["stats"]
            assert st["finite"], (key, alpha)
            assert st["max_abs_m"] <= float(CLAMP)
            if key == "saturated":
                assert st["max_abs_m"] == float(CLAMP)
            if schedule == "layered":
                assert st["max_abs_T"] <= 256.0 + 256.0 * alpha
            else:  # a column of degree <= 9 sums its prior and nine messages
                assert st["max_abs_T"] <= 256.0 + 9 * 256.0 * alpha


# ---- failed codewords of 128 --------------------------------------------------

BUDGETS = {"bg2": (50, 25, 5), "syn_irr1200": (20, 10, 5), "syn_qc_l200": (20, 10, 5)}
# schedule, messages -> code -> one row per budget: failed codewords at (0.75, 0), (1, 0.5), (1, 0)
TABLE = {
    ("layered", "f32"): {"bg2": ((79, 78, 87), (79, 78, 87), (94, 93, 99)),
                         "syn_irr1200": ((61, 59, 64), (63, 60, 67), (76, 72, 77)),
                         "syn_qc_l200": ((69, 69, 70), (72, 72, 72), (75, 76, 76))},
    ("flooding", "f32"): {"bg2": ((79, 78, 87), (83, 81, 87), (112, 113, 112)),
                          "syn_irr1200": ((63, 60, 66), (74, 72, 78), (98, 94, 97)),
                          "syn_qc_l200": ((72, 71, 72), (76, 76, 78), (96, 95, 93))},
    ("layered", "f16"): {"bg2": ((78, 78, 87), (79, 78, 88), (94, 93, 99)),
                         "syn_irr1200": ((61, 59, 64), (63, 60, 67), (76, 72, 77)),
                         "syn_qc_l200": ((69, 69, 70), (72, 72, 72), (75, 76, 76))},
}


@pytest.mark.parametrize("name", list(BUDGETS))
@pytest.mark.parametrize("schedule,messages", list(TABLE))
def test_failed_codewords_table(data_dir, schedule, messages, name):
    """Deterministic CPU results: other values mean the contract was built differently.  The condition on every
    row: the offset at (1, 0.5) fails at most one codeword more than alpha = 0.75 alone."""
    s = L.stream(data_dir, name)
    got = []
    for b in BUDGETS[name]:
        got.append(tuple(failed(oms_decoded(data_dir, name, "stream", s["p0"], b, al, be, schedule, messages), s["uu"])
                         for al, be in PAIRS))
    print(f"{schedule} {messages} {name}: {got}")
    for row in got:
        assert row[1] <= row[0] + 1, row
    assert tuple(got) == TABLE[(schedule, messages)][name]


def test_total_sweeps_at_bg2_budget_25(data_dir):
    s = L.stream(data_dir, "bg2")
    sweeps = [int(oms_decoded(data_dir, "bg2", "stream", s["p0"], 25, al, be)["stats"]["iters"].sum())
              for al, be in PAIRS[:2]]
    assert sweeps == [2244, 2213]  # (0.75, 0) against (1, 0.5)
