"""GPU tests of the offset correction of the min-sum decoders (kml_set_nms_offset;
the offset instances of bp_irregular_nms.hip, bp_irregular_lnms.hip and
bp_irregular_lnms_h16.hip).  Every comparison is equality of bit patterns against
the numpy model of tests/bp_oms_model.py; there is no tolerance anywhere.  With
the offset back at 0 every path is what it was.

Codes, streams and inputs come from test_bp_lnms_model.py, test_bp_llr_model.py
and test_bp_nms_model.py, made once per session; at most 64 stream codewords per
comparison keep the numpy model cheap.
"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from bp_oms_model import oms_blind_metric, oms_decode, oms_llr_model
from conftest import REPO, TESTS, load_case
from test_bp_llr_model import clamp_inputs, llr_stream, points
from test_bp_lnms_model import CODES, QC, code, stream
from test_bp_nms_model import random_p0, saturated_p0
from test_gpu_device_ptrs import DeviceBufs, filled
from test_gpu_llr import assert_equals_llr_model, ctx_for, u32
from test_gpu_nms import assert_equals_model, check_golden_f64

import kmldpc_amd as K

pytestmark = pytest.mark.gpu

# mode -> (schedule, messages, kernel family: the offset only picks the instance)
MODES = {"flooding": ("flooding", "f32", "bp_irregular_nms_kernel"),
         "layered": ("layered", "f32", "bp_irregular_lnms_kernel"),
         "f16": ("layered", "f16", "bp_irregular_lnms_h16_kernel")}
SPA_KERNEL = "bp_irregular_kernel"
PAIRS = [(1.0, 0.5), (0.8125, 0.375), (1.0, 0.3)]  # the last: beta inexact in binary32 and in binary16
N = 64  # stream codewords per comparison
UNSUP = r"\(code -4\)"
ARG = r"\(code -1\)"
KEYS = ("uu_hat", "ret", "cc_hat", "llr_out")


def oms_ctx(data_dir, name, mode, alpha, beta, demapper="exact", **kw):
    sched, msg, _ = MODES[mode]
    ctx = ctx_for(data_dir, name, **kw)
    ctx.set_algorithm("nms", alpha)
    ctx.set_schedule(sched)
    ctx.set_demapper(demapper)
    ctx.set_messages(msg)
    ctx.set_offset(beta)
    assert (ctx.schedule, ctx.demapper, ctx.messages, ctx.offset) == (sched, demapper, msg, float(np.float32(beta)))
    return ctx


def reset(ctx):
    ctx.set_algorithm("spa")
    assert (ctx.schedule, ctx.demapper, ctx.messages, ctx.offset) == ("flooding", "exact", "f32", 0.0)


def p0_model(data_dir, name, p0, budget, mode, alpha, beta):
    _, g = code(data_dir, name)
    sched, msg, _ = MODES[mode]
    return dict(zip(("ret", "uu_hat", "cc_hat"), oms_decode(g, p0, budget, CODES[name][2], alpha, beta, sched, msg)))


def llr_model(data_dir, name, llr, budget, mode, alpha, beta):
    _, g = code(data_dir, name)
    sched, msg, _ = MODES[mode]
    return dict(zip(("ret", "uu_hat", "cc_hat", "llr_out"),
                    oms_llr_model(g, llr, budget, CODES[name][2], alpha, beta, sched, msg)))


def same(a, b, what=""):
    for key in KEYS:
        if key in a and key in b:
            x, y = (u32(a[key]), u32(b[key])) if key == "llr_out" else (np.asarray(a[key]), np.asarray(b[key]))
            assert np.array_equal(x, y), f"{what}: {key}"


def take(r, idx):
    return {k: np.asarray(v)[idx] for k, v in r.items() if k in KEYS}


# BG2: the register path; syn_irr1200: the table path, 91 layers of 1 to 17 rows; syn_qc_l200: layers of 200
# rows, two full passes and a partial one
CASES = [("bg2", 50), ("bg2", 5), ("bg2", 1), ("bg2", 0), ("syn_irr1200", 20), (QC, 20)]


# ---- kernel = model --------------------------------------------------------

@pytest.mark.parametrize("alpha,beta", PAIRS)
@pytest.mark.parametrize("name,budget", CASES)
@pytest.mark.parametrize("mode", list(MODES))
def test_bp_decode_equals_model(data_dir, mode, name, budget, alpha, beta):
    """The P0 instances."""
    ctx = oms_ctx(data_dir, name, mode, alpha, beta)
    p0 = stream(data_dir, name)["p0"][:N]
    m = p0_model(data_dir, name, p0, budget, mode, alpha, beta)
    r = ctx.bp_decode(p0, budget, cc_hat=True)
    assert ctx.bp_kernel() == MODES[mode][2]
    assert_equals_model(r, m, f"{mode} {name} budget {budget} ({alpha}, {beta})")
    max_iter = CODES[name][2]
    if budget == max_iter:  # both outcomes are in the comparison
        assert np.any(m["ret"] == max_iter) and np.any(m["ret"] < max_iter)
    reset(ctx)


@pytest.mark.parametrize("alpha,beta", PAIRS)
@pytest.mark.parametrize("name,budget", CASES)
@pytest.mark.parametrize("mode", list(MODES))
def test_llr_decode_equals_model(data_dir, mode, name, budget, alpha, beta):
    """The LLR instances with the posteriors out; without llr_out (another instance) the same bits."""
    ctx = oms_ctx(data_dir, name, mode, alpha, beta)
    llr = llr_stream(data_dir, name)[:N]
    m = llr_model(data_dir, name, llr, budget, mode, alpha, beta)
    r = ctx.llr_decode(llr, budget, cc_hat=True, llr_out=True)
    assert ctx.bp_kernel() == MODES[mode][2]
    assert_equals_llr_model(r, m, f"{mode} {name} budget {budget} ({alpha}, {beta})")
    plain = ctx.llr_decode(llr, budget, cc_hat=True)
    assert_equals_model(plain, m, f"{mode} {name} budget {budget} ({alpha}, {beta}), no llr_out")
    reset(ctx)


@pytest.mark.parametrize("mode", list(MODES))
def test_the_offset_changes_the_decode(data_dir, mode):
    """(1, 0.5) and (1, 0) differ on the stream, so the comparisons above see the two extra operations."""
    p0 = stream(data_dir, "bg2")["p0"][:N]
    a = p0_model(data_dir, "bg2", p0, 50, mode, 1.0, 0.5)
    b = p0_model(data_dir, "bg2", p0, 50, mode, 1.0, 0.0)
    assert (a["cc_hat"] != b["cc_hat"]).any()
    ctx = oms_ctx(data_dir, "bg2", mode, 1.0, 0.5)
    ra = ctx.bp_decode(p0, 50, cc_hat=True)
    ctx.set_offset(0)
    rb = ctx.bp_decode(p0, 50, cc_hat=True)
    assert_equals_model(ra, a, "beta 0.5")
    assert_equals_model(rb, b, "beta 0")
    reset(ctx)


@pytest.mark.parametrize("mode", list(MODES))
def test_saturated_random_and_clamp_inputs(data_dir, mode):
    """P0 of exactly 0, 1, 0.5 and 1e-300 (messages in the clamp, zero magnitudes, ties), uniform-random P0 that
    never converges, and LLRs of +-inf, +-1e30, +-256, just past 256, +-0 and denormals; beta inexact."""
    alpha, beta = PAIRS[2]
    ctx = oms_ctx(data_dir, "bg2", mode, alpha, beta)
    for key, p0 in (("saturated", saturated_p0(data_dir)), ("random", random_p0(data_dir))):
        m = p0_model(data_dir, "bg2", p0, 50, mode, alpha, beta)
        assert_equals_model(ctx.bp_decode(p0, 50, cc_hat=True), m, key)
    _, g = code(data_dir, "bg2")
    x = clamp_inputs(g, llr_stream(data_dir, "bg2")[0].copy())
    m = llr_model(data_dir, "bg2", x, 50, mode, alpha, beta)
    assert_equals_llr_model(ctx.llr_decode(x, 50, cc_hat=True, llr_out=True), m, "clamp inputs")
    reset(ctx)


def test_zero_iterations_leave_the_outputs(data_dir):
    ctx = oms_ctx(data_dir, "bg2", "layered", 1.0, 0.5)
    B = 5
    llr = np.ascontiguousarray(llr_stream(data_dir, "bg2")[:B])
    uh, cch = np.full((B, ctx.K), 7, np.uint8), np.full((B, ctx.Ncol), 9, np.uint8)
    ret, post = np.full(B, -5, np.int32), np.full((B, ctx.Ncol), -3.5, np.float32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert K.lib().kml_llr_decode(ctx._h, ptr(llr), B, 0, ptr(uh), ptr(ret), ptr(cch), ptr(post), 0) == 0
    assert np.all(uh == 7) and np.all(cch == 9) and np.all(post == np.float32(-3.5)) and np.all(ret == 1)
    reset(ctx)


# ---- the binary16 pair logic -------------------------------------------------

def test_f16_batch_sizes(data_dir):
    """B = 1 (a lone half), 2, 3 (a pair and a lone half) and 63 (an odd batch): a codeword's result is the
    model's whatever the batch."""
    ctx = oms_ctx(data_dir, "bg2", "f16", 1.0, 0.3)
    llr = llr_stream(data_dir, "bg2")[:N]
    m = llr_model(data_dir, "bg2", llr, 50, "f16", 1.0, 0.3)
    for B in (1, 2, 3, 63):
        r = ctx.llr_decode(llr[:B], 50, cc_hat=True, llr_out=True)
        assert ctx.bp_kernel() == MODES["f16"][2]
        same(r, take(m, slice(0, B)), f"B = {B}")
    r = ctx.llr_decode(llr[::-1], 50, cc_hat=True, llr_out=True)  # every codeword in the other half
    same(r, take(m, np.arange(N)[::-1]), "reversed")
    reset(ctx)


@pytest.mark.parametrize("name", ["syn_irr1200", QC])
def test_f16_partners_that_stop_at_different_sweeps(data_dir, name):
    """Noiseless codewords (converged before any sweep: ret = 1) interleaved with priors that never converge (the
    full budget), in both half orders, an odd batch: the early half is recorded at sweep 0 and nothing of it
    changes while its partner runs on with the offset."""
    oc, g = code(data_dir, name)
    rng = np.random.default_rng(31)
    uu = rng.integers(0, 2, (8, oc.K)).astype(np.int32)
    cc = np.stack([oc.encode(u) for u in uu])
    clean = np.where(cc == 0, 6.5, -6.5).astype(np.float32)
    noise = rng.normal(0.0, 3.0, (8, g.cc_len)).astype(np.float32)
    ctx = oms_ctx(data_dir, name, "f16", 1.0, 0.5)
    for first, second in ((clean, noise), (noise, clean)):
        x = np.empty((15, g.cc_len), np.float32)
        x[0::2], x[1::2] = first, second[:7]
        m = llr_model(data_dir, name, x, 20, "f16", 1.0, 0.5)
        early = np.all(x == np.where(x > 0, np.float32(6.5), np.float32(-6.5)), axis=1)
        assert np.all(m["ret"][early] == 1) and np.all(m["ret"][~early] == 20) and 7 <= early.sum() <= 8
        r = ctx.llr_decode(x, 20, cc_hat=True, llr_out=True)
        same(r, m, f"{name}, clean first: {first is clean}")
    reset(ctx)


# ---- the default behaviour is unchanged ------------------------------------

@pytest.mark.parametrize("mode", list(MODES))
def test_offset_zero_after_an_offset_is_the_shipped_decoder(data_dir, mode):
    """One context: the golden fp64 vectors, the beta-0 model, the offset model, the beta-0 model again, the
    golden vectors again."""
    hdr, z = load_case("bg2_16qam_known")
    p0 = z["v_p0"]
    base = p0_model(data_dir, "bg2", p0, 50, mode, 0.75, 0.0)
    off = p0_model(data_dir, "bg2", p0, 50, mode, 0.75, 0.5)
    ctx = ctx_for(data_dir, "bg2")
    reset(ctx)
    check_golden_f64(ctx, z)
    assert ctx.bp_kernel() == SPA_KERNEL
    ctx = oms_ctx(data_dir, "bg2", mode, None, 0.0)
    assert_equals_model(ctx.bp_decode(p0, cc_hat=True), base, "before")
    ctx.set_offset(0.5)
    assert_equals_model(ctx.bp_decode(p0, cc_hat=True), off, "offset 0.5")
    assert ctx.bp_kernel() == MODES[mode][2]
    ctx.set_offset(0)
    assert ctx.offset == 0.0
    assert_equals_model(ctx.bp_decode(p0, cc_hat=True), base, "after")
    assert ctx.bp_kernel() == MODES[mode][2]
    reset(ctx)
    check_golden_f64(ctx, z)
    assert ctx.bp_kernel() == SPA_KERNEL


# ---- the receive paths -----------------------------------------------------

@pytest.mark.parametrize("mode", list(MODES))
def test_known_channel(data_dir, mode):
    """Exact demapper: the P0 model on the oracle's P0; max-log: the LLR model on the model's LLRs."""
    s = stream(data_dir, "bg2")
    y, th, snr = s["y"][:N], s["th"][:N], s["snr"]
    ctx = oms_ctx(data_dir, "bg2", mode, 1.0, 0.5)
    r = ctx.decode_frames(y, snr, th)
    assert ctx.bp_kernel() == MODES[mode][2]
    m = p0_model(data_dir, "bg2", s["p0"][:N], 50, mode, 1.0, 0.5)
    assert np.array_equal(r["uu_hat"], m["uu_hat"]) and np.array_equal(r["ret"], m["ret"])
    ctx.set_demapper("maxlog")
    assert ctx.offset == 0.5
    r = ctx.decode_frames(y, snr, th)
    m = llr_model(data_dir, "bg2", llr_stream(data_dir, "bg2")[:N], 50, mode, 1.0, 0.5)
    assert np.array_equal(r["uu_hat"], m["uu_hat"]) and np.array_equal(r["ret"], m["ret"])
    reset(ctx)


@pytest.mark.parametrize("mode", ["flooding", "layered"])
def test_blind_bg2_exact_demapper(data_dir, mode):
    """The exact front end's candidate metrics stay fp64 sum-product: chosen, metrics and h_hat are bit-identical
    to beta 0 (and to the SPA context's); the final decode is the offset model's on the chosen candidate's P0."""
    n = 32
    s = stream(data_dir, "bg2")
    y, snr = s["y"][:n], s["snr"]
    ctx = ctx_for(data_dir, "bg2")
    reset(ctx)
    spa = ctx.decode_frames(y, snr)
    _, h4 = ctx.kmeans(y)
    ctx = oms_ctx(data_dir, "bg2", mode, 1.0, 0.0)
    ref = ctx.decode_frames(y, snr)
    ctx.set_offset(0.5)
    out = ctx.decode_frames(y, snr)
    assert ctx.bp_kernel() == MODES[mode][2]
    for key in ("chosen", "metrics", "h_hat"):
        assert np.array_equal(out[key], ref[key]) and np.array_equal(out[key], spa[key]), key
    p0 = ctx.demap(y, h4[np.arange(n), out["chosen"]], 10.0 ** (-0.1 * snr))
    m = p0_model(data_dir, "bg2", p0, 50, mode, 1.0, 0.5)
    assert np.array_equal(out["uu_hat"], m["uu_hat"]) and np.array_equal(out["ret"], m["ret"])
    reset(ctx)


@pytest.mark.parametrize("mode", list(MODES))
def test_blind_bg2_maxlog(data_dir, mode):
    """Under max-log the 4 x n metric decodes follow the offset: chosen, metrics, uu_hat and ret are the offset
    model's on ctx.kmeans's candidates; decode_candidates with the caller's two candidates likewise."""
    n = 32
    s = stream(data_dir, "bg2")
    y, snr = s["y"][:n], s["snr"]
    var = 10.0 ** (-0.1 * snr)
    _, g = code(data_dir, "bg2")
    pts, bits = points(data_dir, "bg2")
    sched, msg, kernel = MODES[mode]
    ctx = ctx_for(data_dir, "bg2")
    reset(ctx)
    _, h4 = ctx.kmeans(y)
    ctx = oms_ctx(data_dir, "bg2", mode, 1.0, 0.5, demapper="maxlog")
    out = ctx.decode_frames(y, snr)
    assert ctx.bp_kernel() == kernel
    met, chosen, llrs = oms_blind_metric(g, pts, bits, y, h4, var, 5, 50, 1.0, 0.5, sched, msg)
    met0, _, _ = oms_blind_metric(g, pts, bits, y, h4, var, 5, 50, 1.0, 0.0, sched, msg)
    assert (met != met0).any()  # the offset shows in the metrics of these frames
    assert np.array_equal(out["chosen"], chosen) and np.array_equal(out["metrics"], met)
    m = llr_model(data_dir, "bg2", llrs[np.arange(n), chosen], 50, mode, 1.0, 0.5)
    assert np.array_equal(out["uu_hat"], m["uu_hat"]) and np.array_equal(out["ret"], m["ret"])
    met2, chosen2, llrs2 = oms_blind_metric(g, pts, bits, y, h4[:, :2], var, 5, 50, 1.0, 0.5, sched, msg)
    out2 = ctx.decode_candidates(y, h4[:, :2], snr)
    m2 = llr_model(data_dir, "bg2", llrs2[np.arange(n), chosen2], 50, mode, 1.0, 0.5)
    assert np.array_equal(out2["chosen"], chosen2) and np.array_equal(out2["metrics"], met2)
    assert np.array_equal(out2["uu_hat"], m2["uu_hat"]) and np.array_equal(out2["ret"], m2["ret"])
    reset(ctx)


@pytest.mark.parametrize("mode,n", [("flooding", N), ("layered", N), ("f16", N - 1)])
def test_simulator_path_and_counters(data_dir, mode, n):
    """sim_decode_ex: cw_err and all eight counters (an odd batch in the binary16 format)."""
    s = stream(data_dir, "bg2")
    _, g = code(data_dir, "bg2")
    sched, msg, kernel = MODES[mode]
    st = {}
    ret, uh, _ = oms_decode(g, s["p0"][:n], 50, 50, 1.0, 0.5, sched, msg, stats=st)
    uu = s["uu"][:n].astype(np.uint8)
    want = (uh != uu).sum(axis=1).astype(np.int32)
    it, conv = st["iters"], st["converged"]
    ctx = oms_ctx(data_dir, "bg2", mode, 1.0, 0.5)
    ctx.sim_load(s["snr"], uu, s["y"][:n], s["th"][:n])
    err, _, cnt = ctx.sim_decode_ex(s["snr"])
    assert ctx.bp_kernel() == kernel
    assert np.array_equal(err, want)
    assert (cnt["err_bit"], cnt["err_blk"]) == (int(want.sum()), int(np.sum(want > 0)))
    assert (cnt["tot_bit"], cnt["tot_blk"]) == (n * g.K, n)
    assert cnt["redone"] == 0 and 0 < cnt["err_blk"] < n
    assert cnt["cn_phases"] == int(it.sum()) and cnt["vn_phases"] == int(it.sum() + conv.sum())
    assert cnt["converged"] == int(conv.sum())
    reset(ctx)


def test_device_pointers(data_dir):
    ctx = oms_ctx(data_dir, "bg2", "layered", 1.0, 0.5)
    B = 3
    llr = np.ascontiguousarray(llr_stream(data_dir, "bg2")[:B])
    m = llr_model(data_dir, "bg2", llr, 50, "layered", 1.0, 0.5)
    uh, ret = filled((B, ctx.K), np.uint8), filled(B, np.int32)
    cch, post = filled((B, ctx.Ncol), np.uint8), filled((B, ctx.Ncol), np.float32)
    with DeviceBufs() as d:
        d_l, d_uh, d_ret, d_cch, d_po = d.put(llr), d.put(uh), d.put(ret), d.put(cch), d.put(post)
        assert K.lib().kml_llr_decode(ctx._h, d_l, B, 50, d_uh, d_ret, d_cch, d_po, K.KML_DEVICE_PTRS) == 0
        got = dict(uu_hat=d.get(d_uh, uh), ret=d.get(d_ret, ret), cc_hat=d.get(d_cch, cch), llr_out=d.get(d_po, post))
        same(got, m, "KML_DEVICE_PTRS")
    reset(ctx)


# ---- the cascade and the refusals ------------------------------------------

def test_cascade(data_dir):
    hdr, z = load_case("bg2_16qam_known")
    ctx = oms_ctx(data_dir, "bg2", "flooding", None, 0.5)
    ctx.set_algorithm("nms", 0.8125)  # a new alpha keeps the offset
    assert ctx.offset == 0.5 and ctx.algorithm == ("nms", 0.8125)
    ctx.set_schedule("layered")       # and so do the schedule, the demapper and the format, both ways
    assert ctx.offset == 0.5
    ctx.set_demapper("maxlog")
    ctx.set_messages("f16")
    assert ctx.offset == 0.5
    ctx.set_messages("f32")
    ctx.set_demapper("exact")
    ctx.set_schedule("flooding")
    assert ctx.offset == 0.5
    ctx.set_offset(0.3)               # held as a float
    assert ctx.offset == float(np.float32(0.3))
    ctx.set_algorithm("spa")          # leaves the min-sum mode and its offset
    assert (ctx.offset, ctx.messages, ctx.schedule, ctx.demapper) == (0.0, "f32", "flooding", "exact")
    ctx.set_algorithm("nms")          # coming back does not bring the offset back
    assert ctx.offset == 0.0
    reset(ctx)
    check_golden_f64(ctx, z)
    assert ctx.bp_kernel() == SPA_KERNEL


def test_the_offset_needs_the_min_sum_mode(data_dir):
    hdr, z = load_case("bg2_16qam_known")
    ctx = ctx_for(data_dir, "bg2")
    reset(ctx)
    with pytest.raises(K.KmlError, match=UNSUP):  # SPA mode
        ctx.set_offset(0.5)
    assert "min-sum mode" in K.lib().kml_last_error(ctx._h).decode()
    assert ctx.offset == 0.0 and ctx.algorithm[0] == "spa"
    check_golden_f64(ctx, z)
    ctx.set_offset(0)  # always accepted
    ctx.set_algorithm("nms")
    ctx.set_offset(0.5)
    for bad in (-0.5, float("nan"), float("inf"), 257.0, 1e-50):
        with pytest.raises(K.KmlError, match=ARG):
            ctx.set_offset(bad)
        assert ctx.offset == 0.5  # the context keeps its value
    reset(ctx)
    check_golden_f64(ctx, z)
    assert ctx.bp_kernel() == SPA_KERNEL


def test_an_offset_that_rounds_to_zero_in_binary16(data_dir):
    hdr, z = load_case("bg2_16qam_known")
    ctx = oms_ctx(data_dir, "bg2", "f16", None, 0.5)
    for tiny in (1e-9, 2.0 ** -25):  # RN16 gives +0 (2^-25 is the tie, to even)
        with pytest.raises(K.KmlError, match=ARG):
            ctx.set_offset(tiny)
        assert "binary16" in K.lib().kml_last_error(ctx._h).decode()
        assert ctx.messages == "f16" and ctx.offset == 0.5
    ctx.set_offset(2.0 ** -24)  # the smallest half
    ctx.set_messages("f32")
    ctx.set_offset(1e-9)        # fine in f32 ...
    with pytest.raises(K.KmlError, match=ARG):  # ... and then the format is refused
        ctx.set_messages("f16")
    assert "offset" in K.lib().kml_last_error(ctx._h).decode()
    assert ctx.messages == "f32" and ctx.offset == float(np.float32(1e-9))
    reset(ctx)
    check_golden_f64(ctx, z)


def test_min_sum_refusals_hold(data_dir):
    """syn, the iteration profile and the soft-syndrome metric are refused as without the offset."""
    hdr, z = load_case("bg2_16qam_known")
    s = stream(data_dir, "bg2")
    ctx = oms_ctx(data_dir, "bg2", "layered", None, 0.5)
    B = z["v_p0"].shape[0]
    with pytest.raises(K.KmlError, match=UNSUP):
        ctx.bp_decode(z["v_p0"], syn=np.full((B, ctx.M), -1.0))
    assert "syn" in K.lib().kml_last_error(ctx._h).decode()
    ctx.sim_load(s["snr"], s["uu"][:8].astype(np.uint8), s["y"][:8], s["th"][:8])
    with pytest.raises(K.KmlError, match=UNSUP):
        ctx.sim_decode_profile(s["snr"])
    assert ctx.offset == 0.5 and ctx.algorithm[0] == "nms"
    reset(ctx)
    check_golden_f64(ctx, z)
    soft = oms_ctx(data_dir, "bg2", "layered", None, 0.5, metric_soft=True)
    with pytest.raises(K.KmlError, match=UNSUP):
        soft.decode_frames(s["y"][:4], s["snr"])
    assert "soft-syndrome" in K.lib().kml_last_error(soft._h).decode()
    assert soft.offset == 0.5
    reset(soft)
    check_golden_f64(soft, z)


def test_other_codes_refuse_the_offset(data_dir):
    hdr, z = load_case("peg2304_qpsk_known")
    ctx = K.Context(matrix_file=os.path.join(data_dir, hdr["matrix"]), modem_file=os.path.join(data_dir, hdr["modem"]),
                    is5g=bool(hdr["is5g"]), max_iter=hdr["max_iter"], device=0)
    with pytest.raises(K.KmlError, match=UNSUP):  # the algorithm's refusal comes first
        ctx.set_algorithm("nms")
    with pytest.raises(K.KmlError, match=UNSUP):
        ctx.set_offset(0.5)
    assert ctx.offset == 0.0 and ctx.algorithm[0] == "spa"
    check_golden_f64(ctx, z)
    ctx.close()


def test_generic_kernel_refuses_the_offset(data_dir):
    """KML_BP_KERNEL is read once per process: a child started with KML_BP_KERNEL=generic."""
    env = dict(os.environ, PYTHONPATH=REPO, KML_BP_KERNEL="generic")
    p = subprocess.run([sys.executable, os.path.join(TESTS, "oms_generic_child.py"), data_dir], env=env,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "refused" in p.stdout


def test_drivers_take_the_offset(data_dir, tmp_path):
    """kmldpc_sim and python -m kmldpc_amd.simulate: --offset / KML_OFFSET, stated in the line after the message
    format's; the same frames give the same lines in both drivers, and their counts are those of the Python
    face on the same generated frames.  The default output has no new line."""
    from test_gpu_driver import _messages
    from conftest import write_config
    from kmldpc_amd.simulate import point_seed
    cfg = tmp_path / "config.toml"
    write_config(str(cfg), data_dir, CODES["bg2"][0], CODES["bg2"][3], is5g=True, known=True, max_iter=50, snr=7.0,
                 max_blocks=256, max_err=1000000)
    env = dict(os.environ, KML_BATCH="256", KML_SEED="4", PYTHONPATH=REPO)
    for k in ("KML_ALGORITHM", "KML_SCHEDULE", "KML_DEMAPPER", "KML_MESSAGES", "KML_OFFSET"):
        env.pop(k, None)
    exe = os.path.join(REPO, "kmldpc_amd", "bin", "kmldpc_sim")
    py = [sys.executable, "-m", "kmldpc_amd.simulate"]
    run = lambda cmd, e=env: subprocess.run(cmd, cwd=tmp_path, env=e, capture_output=True, text=True, timeout=120)
    r1 = run([exe, "--algorithm", "nms:1", "--schedule", "layered", "--offset", "0.5", str(cfg)])
    r2 = run(py + [str(cfg)], dict(env, KML_ALGORITHM="nms:1", KML_SCHEDULE="layered", KML_OFFSET="0.5"))
    off0 = run([exe, "--algorithm", "nms:1", "--schedule", "layered", "--offset=0", str(cfg)])
    plain = run([exe, "--algorithm", "nms:1", "--schedule", "layered", str(cfg)])
    for r in (r1, r2, off0, plain):
        assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-1000:]
    m1, m2, m0, mp = (_messages(r.stdout) for r in (r1, r2, off0, plain))
    assert m1[1] == "BP decode schedule: layered" and m1[2] == "BP min-sum offset: 0.5"
    assert m1[3] == "Start simulation"
    assert m1[:-1] == m2[:-1]
    assert m0[:-1] == mp[:-1] and not any("offset" in x for x in mp)  # no added line by default
    assert m1[:-1] != [x for x in mp[:-1]]
    res = [x for x in m1 if x.startswith("SNR = ")]
    got = re.search(r"Total blk = (\d+) Error blk = (\d+) Error bit = (\d+)", res[-1])  # the point's last line
    ctx = oms_ctx(data_dir, "bg2", "layered", 1.0, 0.5)
    ctx.sim_generate(7.0, 256, seed=point_seed(4, 0))  # the drivers' one round of 256 frames
    c = ctx.sim_decode(7.0)
    assert tuple(int(x) for x in got.groups()) == (c["tot_blk"], c["err_blk"], c["err_bit"])
    assert c["tot_blk"] == 256 and 0 < c["err_blk"] < 256
    reset(ctx)
    assert run([exe, "--algorithm", "nms", "--offset", "half", str(cfg)]).returncode == 2
    assert run(py + ["--algorithm", "nms", "--offset", "half", str(cfg)]).returncode == 2
