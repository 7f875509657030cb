"""GPU tests of the binary16 message format of the layered min-sum decoder
(kml_set_messages, KML_MSG_F16; kmldpc_amd/csrc/bp_irregular_lnms_h16.hip).
Every comparison is equality of bit patterns against the numpy model of
tests/bp_h16_model.py; there is no tolerance anywhere.

The kernel decodes two codewords in the two halves of every word, so beside the
arithmetic the tests pin the pair logic: lone halves, odd batches, second pairs
of a workgroup, every codeword in both halves and beside different partners, and
partners that stop at different times.  Nothing of the format leaks into the f32
min-sum or the fp64 paths.

Codes, streams and the models' decodes come from test_bp_h16_model.py,
test_bp_llr_model.py and test_bp_lnms_model.py, made once per session.
"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from bp_h16_model import blind_metric_h16, lnms_h16_llr_model, lnms_h16_model
from bp_lnms_model import lnms_model
from bp_nms_model import nms_model
from conftest import REPO, TESTS, load_case
from test_bp_h16_model import h16_decode, h16_llr_decoded
from test_bp_llr_model import clamp_inputs, llr_stream, points
from test_bp_lnms_model import CODES, QC, code, stream
from test_bp_nms_model import random_p0, saturated_p0
from test_gpu_device_ptrs import DeviceBufs, filled
from test_gpu_llr import assert_equals_llr_model, ctx_for, u32
from test_gpu_nms import assert_equals_model, check_golden_f64

import kmldpc_amd as K

pytestmark = pytest.mark.gpu

H16_KERNEL = "bp_irregular_lnms_h16_kernel"
F32_KERNEL = "bp_irregular_lnms_kernel"
FLOOD_KERNEL = "bp_irregular_nms_kernel"
SPA_KERNEL = "bp_irregular_kernel"
N = 64  # stream codewords per comparison
UNSUP = r"\(code -4\)"
ARG = r"\(code -1\)"
KEYS = ("uu_hat", "ret", "cc_hat", "llr_out")


def h16_ctx(data_dir, name, alpha=None, demapper="exact", **kw):
    ctx = ctx_for(data_dir, name, **kw)
    ctx.set_algorithm("nms", alpha)
    ctx.set_schedule("layered")
    ctx.set_demapper(demapper)
    ctx.set_messages("f16")
    assert (ctx.schedule, ctx.demapper, ctx.messages) == ("layered", demapper, "f16")
    return ctx


def reset(ctx):
    ctx.set_algorithm("spa")
    assert ctx.schedule == "flooding" and ctx.demapper == "exact" and ctx.messages == "f32"


def same(a, b, what=""):
    for key in KEYS:
        if key in a or key in b:
            x, y = (u32(a[key]), u32(b[key])) if key == "llr_out" else (np.asarray(a[key]), np.asarray(b[key]))
            assert np.array_equal(x, y), f"{what}: {key}"


def take(r, idx):
    return {k: np.asarray(v)[idx] for k, v in r.items() if k in KEYS}


CASES = [("bg2", 50), ("bg2", 5), ("bg2", 1), ("bg2", 0), ("syn_irr1200", 20), (QC, 20)]


# ---- kernel = model --------------------------------------------------------

@pytest.mark.parametrize("name,budget", CASES)
def test_bp_decode_equals_model(data_dir, name, budget):
    """The P0 instances: BG2 (12 passes in registers), syn_irr1200 (91 layers, the table path) and
    syn_qc_l200 (a layer of two passes and a partial one)."""
    ctx = h16_ctx(data_dir, name)
    p0 = stream(data_dir, name)["p0"][:N]
    m = h16_decode(data_dir, name, f"stream{N}", p0, budget)
    r = ctx.bp_decode(p0, budget, cc_hat=True)
    assert ctx.bp_kernel() == H16_KERNEL
    assert_equals_model(r, m, f"{name} budget {budget}")
    max_iter = CODES[name][2]
    if budget == max_iter:  # both outcomes are in the comparison
        assert np.any(m["ret"] == max_iter) and np.any(m["ret"] < max_iter)
    reset(ctx)


@pytest.mark.parametrize("name,budget", CASES)
def test_llr_decode_equals_model(data_dir, name, budget):
    """The LLR instances with the posteriors out; without llr_out (another instance) the same bits."""
    ctx = h16_ctx(data_dir, name)
    llr = llr_stream(data_dir, name)[:N]
    m = h16_llr_decoded(data_dir, name, f"stream{N}", llr, budget)
    r = ctx.llr_decode(llr, budget, cc_hat=True, llr_out=True)
    assert ctx.bp_kernel() == H16_KERNEL
    assert_equals_llr_model(r, m, f"{name} budget {budget}")
    plain = ctx.llr_decode(llr, budget, cc_hat=True)
    assert_equals_model(plain, m, f"{name} budget {budget}, no llr_out")
    if budget > 0:  # the posteriors are halves, and the decisions are theirs
        T = r["llr_out"]
        assert np.array_equal(u32(T.astype(np.float16).astype(np.float32)), u32(T))
        assert np.array_equal(np.where(T > 0, 0, 1).astype(np.uint8), r["cc_hat"])
    reset(ctx)


def test_zero_iterations_leave_the_outputs(data_dir):
    ctx = h16_ctx(data_dir, "bg2")
    B = 5
    llr = np.ascontiguousarray(llr_stream(data_dir, "bg2")[:B])
    uh, cch = np.full((B, ctx.K), 7, np.uint8), np.full((B, ctx.Ncol), 9, np.uint8)
    ret, post = np.full(B, -5, np.int32), np.full((B, ctx.Ncol), -3.5, np.float32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert K.lib().kml_llr_decode(ctx._h, ptr(llr), B, 0, ptr(uh), ptr(ret), ptr(cch), ptr(post), 0) == 0
    assert ctx.bp_kernel() == H16_KERNEL
    assert np.all(uh == 7) and np.all(cch == 9) and np.all(post == np.float32(-3.5))
    assert np.all(ret == 1)
    reset(ctx)


@pytest.mark.parametrize("alpha", [1.0, 0.8125])
def test_alpha(data_dir, alpha):
    ctx = h16_ctx(data_dir, "bg2", alpha)
    llr = llr_stream(data_dir, "bg2")[:N]
    m = h16_llr_decoded(data_dir, "bg2", f"stream{N}", llr, 50, alpha)
    base = h16_llr_decoded(data_dir, "bg2", f"stream{N}", llr, 50)
    assert (m["cc_hat"] != base["cc_hat"]).any()  # the factor matters on these codewords
    r = ctx.llr_decode(llr, 50, cc_hat=True, llr_out=True)
    assert_equals_llr_model(r, m, f"alpha {alpha}")
    reset(ctx)


@pytest.mark.parametrize("key,make", [("saturated", saturated_p0), ("random", random_p0)])
def test_saturated_and_random_priors(data_dir, key, make):
    p0 = make(data_dir)
    m = h16_decode(data_dir, "bg2", key, p0, 50)
    ctx = h16_ctx(data_dir, "bg2")
    assert_equals_model(ctx.bp_decode(p0, 50, cc_hat=True), m, key)
    reset(ctx)


def test_clamp_inputs(data_dir):
    """+-inf, +-1e30, +-256, just past 256, +-0 and denormals: the kernel decodes their clamped values."""
    _, g = code(data_dir, "bg2")
    x = clamp_inputs(g, llr_stream(data_dir, "bg2")[0].copy())
    m = h16_llr_decoded(data_dir, "bg2", "clamp", x, 50)
    ctx = h16_ctx(data_dir, "bg2")
    r = ctx.llr_decode(x, 50, cc_hat=True, llr_out=True)
    assert_equals_llr_model(r, m, "clamp inputs")
    r2 = ctx.llr_decode(np.clip(x, -256.0, 256.0), 50, cc_hat=True, llr_out=True)
    assert_equals_llr_model(r2, m, "clamped inputs")
    reset(ctx)


def test_tie_to_the_p0_entry(data_dir):
    """llr_decode of the P0 contract's float priors equals bp_decode of that P0."""
    from bp_nms_model import priors
    _, g = code(data_dir, "bg2")
    ctx = h16_ctx(data_dir, "bg2")
    for p0 in (stream(data_dir, "bg2")["p0"][:N], saturated_p0(data_dir)):
        old = ctx.bp_decode(p0, 50, cc_hat=True)
        new = ctx.llr_decode(priors(g, p0)[:, g.punct:], 50, cc_hat=True)
        same(old, new, "P0 entry against LLR entry")
    reset(ctx)


# ---- the pair logic --------------------------------------------------------

def test_batch_sizes(data_dir):
    """B = 1 (a lone half), 2, 3 (a pair and a lone half) and 700 (beyond the resident workgroups), each
    twice on one context: a codeword's result is the model's whatever the batch."""
    ctx = h16_ctx(data_dir, "bg2")
    llr = llr_stream(data_dir, "bg2")
    n = llr.shape[0]
    big = np.concatenate([llr] * (700 // n + 1))[:700]
    m = h16_llr_decoded(data_dir, "bg2", f"stream{N}", llr[:N], 50)
    runs = {}
    for tag, B in [("1", 1), ("2", 2), ("3", 3), ("700", 700), ("1 again", 1), ("2 again", 2), ("3 again", 3),
                   ("700 again", 700)]:
        runs[tag] = ctx.llr_decode(big[:B], 50, cc_hat=True, llr_out=True)
        assert ctx.bp_kernel() == H16_KERNEL
    for tag, B in [("1", 1), ("2", 2), ("3", 3)]:
        same(runs[tag], runs[tag + " again"], f"B = {B} twice")
        same(runs[tag], take(m, slice(0, B)), f"B = {B} against the model")
    same(runs["700"], runs["700 again"], "B = 700 twice")
    same(take(runs["700"], slice(0, N)), m, "B = 700 against the model")
    same(take(runs["700"], slice(n, 700)), take(runs["700"], slice(0, 700 - n)), "B = 700, the repeats")
    reset(ctx)


def test_workgroups_take_a_second_pair(data_dir):
    """1100 frames, the 64 tiled, at budget 5: more pairs than resident workgroups (two per CU)."""
    ctx = h16_ctx(data_dir, "bg2")
    p0 = stream(data_dir, "bg2")["p0"][:N]
    m = h16_decode(data_dir, "bg2", f"stream{N}", p0, 5)
    idx = np.arange(1100) % N
    r = ctx.bp_decode(p0[idx], 5, cc_hat=True)
    assert ctx.bp_kernel() == H16_KERNEL
    same(r, take(m, idx), "1100 tiled frames")
    reset(ctx)


@pytest.mark.parametrize("name", ["bg2", "syn_irr1200"])
def test_partners_and_halves(data_dir, name):
    """The same 64 codewords in order, reversed and rolled by one: every codeword sits in both halves and
    beside different partners, and each result equals the model's (and so the other orders')."""
    budget = CODES[name][2]
    ctx = h16_ctx(data_dir, name)
    llr = llr_stream(data_dir, name)[:N]
    m = h16_llr_decoded(data_dir, name, f"stream{N}", llr, budget)
    for what, idx in (("in order", np.arange(N)), ("reversed", np.arange(N)[::-1]), ("rolled", np.roll(np.arange(N), 1))):
        r = ctx.llr_decode(llr[idx], budget, cc_hat=True, llr_out=True)
        same(r, take(m, idx), f"{name} {what}")
    reset(ctx)


@pytest.mark.parametrize("name", ["syn_irr1200", QC])
def test_partners_that_stop_at_different_times(data_dir, name):
    """Noiseless codewords (converged before any sweep: ret = 1) interleaved with priors that never converge
    (the full budget), in both half orders, an odd batch included: the early half is recorded at sweep 0,
    the pair runs on for 20 sweeps, and nothing of the recorded half changes."""
    oc, g = code(data_dir, name)
    rng = np.random.default_rng(31)
    uu = rng.integers(0, 2, (8, oc.K)).astype(np.int32)
    cc = np.stack([oc.encode(u) for u in uu])
    clean = np.where(cc == 0, 6.5, -6.5).astype(np.float32)
    noise = rng.normal(0.0, 3.0, (8, g.cc_len)).astype(np.float32)
    ctx = h16_ctx(data_dir, name)
    for first, second in ((clean, noise), (noise, clean)):
        x = np.empty((15, g.cc_len), np.float32)
        x[0::2], x[1::2] = first, second[:7]
        ret, uh, cch, T = lnms_h16_llr_model(g, x, 20, 20)
        early = np.all(x == np.where(x > 0, np.float32(6.5), np.float32(-6.5)), axis=1)
        assert np.all(ret[early] == 1) and np.all(ret[~early] == 20) and 7 <= early.sum() <= 8
        r = ctx.llr_decode(x, 20, cc_hat=True, llr_out=True)
        same(r, dict(ret=ret, uu_hat=uh, cc_hat=cch, llr_out=T), f"{name}, clean first: {first is clean}")
        assert np.array_equal(r["uu_hat"][early], uu[:early.sum()].astype(np.uint8))
    reset(ctx)


# ---- the receive paths -----------------------------------------------------

def test_known_channel(data_dir):
    """Exact demapper: the P0 model on the oracle's P0; max-log: the LLR model on the model's LLRs."""
    s = stream(data_dir, "bg2")
    y, th, snr = s["y"][:N], s["th"][:N], s["snr"]
    ctx = h16_ctx(data_dir, "bg2")
    r = ctx.decode_frames(y, snr, th)
    assert ctx.bp_kernel() == H16_KERNEL
    m = h16_decode(data_dir, "bg2", f"stream{N}", s["p0"][:N], 50)
    assert np.array_equal(r["uu_hat"], m["uu_hat"]) and np.array_equal(r["ret"], m["ret"])
    ctx.set_demapper("maxlog")
    assert ctx.messages == "f16"
    r = ctx.decode_frames(y, snr, th)
    assert ctx.bp_kernel() == H16_KERNEL
    m = h16_llr_decoded(data_dir, "bg2", f"stream{N}", llr_stream(data_dir, "bg2")[:N], 50)
    assert np.array_equal(r["uu_hat"], m["uu_hat"]) and np.array_equal(r["ret"], m["ret"])
    reset(ctx)


def test_blind_bg2_exact_demapper(data_dir):
    """The exact front end's candidate metrics stay fp64 sum-product: chosen, metrics and h_hat are the SPA
    context's; the final decode is the binary16 model's on the chosen candidate's P0."""
    n = 32
    s = stream(data_dir, "bg2")
    y, snr = s["y"][:n], s["snr"]
    _, g = code(data_dir, "bg2")
    ctx = ctx_for(data_dir, "bg2")
    reset(ctx)
    ref = ctx.decode_frames(y, snr)
    _, h4 = ctx.kmeans(y)
    ctx = h16_ctx(data_dir, "bg2")
    out = ctx.decode_frames(y, snr)
    assert ctx.bp_kernel() == H16_KERNEL
    for key in ("chosen", "metrics", "h_hat"):
        assert np.array_equal(out[key], ref[key]), key
    p0 = ctx.demap(y, h4[np.arange(n), out["chosen"]], 10.0 ** (-0.1 * snr))
    ret, uh, _ = lnms_h16_model(g, p0, 50, 50)
    assert np.array_equal(out["uu_hat"], uh) and np.array_equal(out["ret"], ret)
    reset(ctx)


def test_blind_bg2_maxlog(data_dir):
    """chosen, metrics, uu_hat and ret are the model's on ctx.kmeans's candidates: the 4 x n metric decodes
    and the final decode (its p0_sel addressing applied per half) all run the binary16 kernel."""
    n = 32
    s = stream(data_dir, "bg2")
    y, snr = s["y"][:n], s["snr"]
    var = 10.0 ** (-0.1 * snr)
    _, g = code(data_dir, "bg2")
    pts, bits = points(data_dir, "bg2")
    ctx = ctx_for(data_dir, "bg2")
    reset(ctx)
    ref = ctx.decode_frames(y, snr)
    _, h4 = ctx.kmeans(y)
    ctx = h16_ctx(data_dir, "bg2", demapper="maxlog")
    out = ctx.decode_frames(y, snr)
    assert ctx.bp_kernel() == H16_KERNEL
    met, chosen, llrs = blind_metric_h16(g, pts, bits, y, h4, var, 5, 50)
    assert np.array_equal(out["chosen"], chosen)
    assert np.array_equal(out["metrics"], met)
    assert np.array_equal(out["h_hat"], ref["h_hat"])  # k-means is untouched
    assert len(set(chosen.tolist())) > 1               # more than one rotation is chosen
    ret, uh, _, _ = lnms_h16_llr_model(g, llrs[np.arange(n), chosen], 50, 50)
    assert np.array_equal(out["uu_hat"], uh) and np.array_equal(out["ret"], ret)
    # the caller's candidates: two of them
    met2, chosen2, llrs2 = blind_metric_h16(g, pts, bits, y, h4[:, :2], var, 5, 50)
    out2 = ctx.decode_candidates(y, h4[:, :2], snr)
    ret2, uh2, _, _ = lnms_h16_llr_model(g, llrs2[np.arange(n), chosen2], 50, 50)
    assert np.array_equal(out2["chosen"], chosen2) and np.array_equal(out2["metrics"], met2)
    assert np.array_equal(out2["uu_hat"], uh2) and np.array_equal(out2["ret"], ret2)
    # histogram mode: the metrics only; uu_hat is what the last candidate's metric decode left
    hist = ctx.decode_frames(y, snr, histogram=True)
    assert np.array_equal(hist["chosen"], chosen) and np.array_equal(hist["metrics"], met)
    assert np.array_equal(hist["uu_hat"], lnms_h16_llr_model(g, llrs[:, 3], 5, 50)[1])
    reset(ctx)


def test_blind_syn_irr1200(data_dir):
    """A non-5G code keeps the hard metric: chosen and metrics are the f32 format's bit for bit, the final
    decode is the binary16 model's."""
    from bp_llr_model import maxlog_llr
    n = 32
    name = "syn_irr1200"
    s = stream(data_dir, name)
    y, snr = s["y"][:n], s["snr"]
    _, g = code(data_dir, name)
    pts, bits = points(data_dir, name)
    ctx = h16_ctx(data_dir, name, demapper="maxlog")
    ctx.set_messages("f32")
    ref = ctx.decode_frames(y, snr)
    assert ctx.bp_kernel() == F32_KERNEL
    _, h4 = ctx.kmeans(y)
    ctx.set_messages("f16")
    out = ctx.decode_frames(y, snr)
    assert ctx.bp_kernel() == H16_KERNEL
    for key in ("chosen", "metrics", "h_hat"):
        assert np.array_equal(out[key], ref[key]), key
    llr = maxlog_llr(pts, bits, y, h4[np.arange(n), out["chosen"]], 10.0 ** (-0.1 * snr))
    ret, uh, _, _ = lnms_h16_llr_model(g, llr, 20, 20)
    assert np.array_equal(out["uu_hat"], uh) and np.array_equal(out["ret"], ret)
    reset(ctx)


@pytest.mark.parametrize("n", [N, N - 1])
def test_simulator_path_and_counters(data_dir, n):
    """sim_decode_ex: cw_err and all eight counters are each codeword's own, the phase counts from its own
    sweep count and not the pair's (an odd batch included)."""
    s = stream(data_dir, "bg2")
    _, g = code(data_dir, "bg2")
    m = h16_decode(data_dir, "bg2", f"stream{N}", s["p0"][:N], 50)
    uu = s["uu"][:n].astype(np.uint8)
    want = (m["uu_hat"][:n] != uu).sum(axis=1).astype(np.int32)
    it, conv = m["stats"]["iters"][:n], m["stats"]["converged"][:n]
    assert len(set(it.tolist())) > 3  # partners stop at different times
    ctx = h16_ctx(data_dir, "bg2")
    ctx.sim_load(s["snr"], uu, s["y"][:n], s["th"][:n])
    err, _, cnt = ctx.sim_decode_ex(s["snr"])
    assert ctx.bp_kernel() == H16_KERNEL
    assert np.array_equal(err, want)
    assert (cnt["err_bit"], cnt["err_blk"]) == (int(want.sum()), int(np.sum(want > 0)))
    assert (cnt["tot_bit"], cnt["tot_blk"]) == (n * g.K, n)
    assert cnt["redone"] == 0
    assert 0 < cnt["err_blk"] < n
    assert cnt["cn_phases"] == int(it.sum()) and cnt["vn_phases"] == int(it.sum() + conv.sum())
    assert cnt["converged"] == int(conv.sum())
    c = ctx.sim_decode(s["snr"])  # the plain entry point counts the same
    assert (c["err_bit"], c["err_blk"], c["tot_blk"], c["redone"]) == (cnt["err_bit"], cnt["err_blk"], n, 0)
    reset(ctx)


def test_device_pointers(data_dir):
    ctx = h16_ctx(data_dir, "bg2")
    B = 3
    llr = np.ascontiguousarray(llr_stream(data_dir, "bg2")[:B])
    m = h16_llr_decoded(data_dir, "bg2", f"stream{N}", llr_stream(data_dir, "bg2")[:N], 50)
    uh, ret = filled((B, ctx.K), np.uint8), filled(B, np.int32)
    cch, post = filled((B, ctx.Ncol), np.uint8), filled((B, ctx.Ncol), np.float32)
    with DeviceBufs() as d:
        d_l, d_uh, d_ret, d_cch, d_po = d.put(llr), d.put(uh), d.put(ret), d.put(cch), d.put(post)
        assert K.lib().kml_llr_decode(ctx._h, d_l, B, 50, d_uh, d_ret, d_cch, d_po, K.KML_DEVICE_PTRS) == 0
        assert ctx.bp_kernel() == H16_KERNEL
        got = dict(uu_hat=d.get(d_uh, uh), ret=d.get(d_ret, ret), cc_hat=d.get(d_cch, cch), llr_out=d.get(d_po, post))
        same(got, take(m, slice(0, B)), "KML_DEVICE_PTRS")
    reset(ctx)


# ---- nothing leaks into the other paths ------------------------------------

def test_no_leakage(data_dir):
    """The fp64 golden vectors (syn included), an f32 flooding and an f32 layered min-sum decode match their
    models before a binary16 decode and again after it, on one context."""
    hdr, z = load_case("bg2_16qam_known")
    assert (hdr["matrix"], hdr["modem"], hdr["max_iter"]) == (CODES["bg2"][0], CODES["bg2"][3], CODES["bg2"][2])
    _, g = code(data_dir, "bg2")
    p0 = z["v_p0"]
    flood = dict(zip(("ret", "uu_hat", "cc_hat"), nms_model(g, p0, 50, 50)))
    lay = dict(zip(("ret", "uu_hat", "cc_hat"), lnms_model(g, p0, 50, 50)))
    half = dict(zip(("ret", "uu_hat", "cc_hat"), lnms_h16_model(g, p0, 50, 50)))
    ctx = ctx_for(data_dir, "bg2")
    reset(ctx)

    def f32_paths():
        check_golden_f64(ctx, z)
        assert ctx.bp_kernel() == SPA_KERNEL
        ctx.set_algorithm("nms")
        assert ctx.messages == "f32"
        assert_equals_model(ctx.bp_decode(p0, cc_hat=True), flood, "flooding, f32")
        assert ctx.bp_kernel() == FLOOD_KERNEL
        ctx.set_schedule("layered")
        assert ctx.messages == "f32"
        assert_equals_model(ctx.bp_decode(p0, cc_hat=True), lay, "layered, f32")
        assert ctx.bp_kernel() == F32_KERNEL

    f32_paths()
    ctx.set_messages("f16")
    assert_equals_model(ctx.bp_decode(p0, cc_hat=True), half, "layered, binary16")
    assert ctx.bp_kernel() == H16_KERNEL
    ctx.set_messages("f32")  # back within the layered mode
    assert_equals_model(ctx.bp_decode(p0, cc_hat=True), lay, "layered, f32 after binary16")
    assert ctx.bp_kernel() == F32_KERNEL
    ctx.set_messages("f16")
    ctx.bp_decode(p0, cc_hat=True)
    ctx.set_algorithm("spa")  # leaves the min-sum mode, its schedule, its front end and its format
    assert (ctx.messages, ctx.demapper, ctx.schedule) == ("f32", "exact", "flooding")
    f32_paths()
    reset(ctx)
    check_golden_f64(ctx, z)


# ---- the cascade and the refusals ------------------------------------------

def test_cascade(data_dir):
    hdr, z = load_case("bg2_16qam_known")
    ctx = h16_ctx(data_dir, "bg2")
    ctx.set_algorithm("nms", 0.8125)  # a new alpha keeps the format
    assert ctx.messages == "f16" and ctx.algorithm == ("nms", 0.8125)
    ctx.set_schedule("layered")       # and so do the layered schedule again and the demapper
    ctx.set_demapper("maxlog")
    assert ctx.messages == "f16"
    ctx.set_demapper("exact")
    assert ctx.messages == "f16"
    ctx.set_schedule("flooding")      # the flooding schedule has no binary16 kernel
    assert ctx.messages == "f32" and ctx.algorithm == ("nms", 0.8125)
    ctx.set_schedule("layered")       # coming back does not bring the format back
    assert ctx.messages == "f32"
    ctx.set_messages("f16")
    ctx.set_algorithm("spa")
    assert (ctx.messages, ctx.schedule, ctx.demapper) == ("f32", "flooding", "exact")
    check_golden_f64(ctx, z)
    assert ctx.bp_kernel() == SPA_KERNEL


def test_f16_needs_the_layered_min_sum_mode(data_dir):
    hdr, z = load_case("bg2_16qam_known")
    ctx = ctx_for(data_dir, "bg2")
    reset(ctx)
    with pytest.raises(K.KmlError, match=UNSUP):  # SPA mode
        ctx.set_messages("f16")
    assert "layered min-sum" in K.lib().kml_last_error(ctx._h).decode()
    assert ctx.messages == "f32" and ctx.algorithm[0] == "spa"
    check_golden_f64(ctx, z)
    ctx.set_algorithm("nms")
    with pytest.raises(K.KmlError, match=UNSUP):  # min-sum, flooding
        ctx.set_messages("f16")
    assert "flooding schedule has no binary16 kernel" in K.lib().kml_last_error(ctx._h).decode()
    assert ctx.messages == "f32" and ctx.schedule == "flooding"
    with pytest.raises(K.KmlError, match=ARG):
        ctx.set_messages("bf16")
    assert ctx.messages == "f32"
    reset(ctx)
    check_golden_f64(ctx, z)
    assert ctx.bp_kernel() == SPA_KERNEL


def test_alpha_that_rounds_to_zero(data_dir):
    hdr, z = load_case("bg2_16qam_known")
    ctx = h16_ctx(data_dir, "bg2")
    for tiny in (1e-9, 2.0 ** -25):  # RN16 gives +0 (2^-25 is the tie, to even)
        with pytest.raises(K.KmlError, match=ARG):
            ctx.set_algorithm("nms", tiny)
        assert "binary16" in K.lib().kml_last_error(ctx._h).decode()
        assert ctx.messages == "f16" and ctx.algorithm == ("nms", 0.75) and ctx.schedule == "layered"
    ctx.set_algorithm("nms", 2.0 ** -24)  # the smallest half
    assert ctx.messages == "f16"
    ctx.set_messages("f32")
    ctx.set_algorithm("nms", 1e-9)        # fine in f32 ...
    with pytest.raises(K.KmlError, match=ARG):  # ... and then the format is refused
        ctx.set_messages("f16")
    assert ctx.messages == "f32" and ctx.algorithm == ("nms", float(np.float32(1e-9)))
    reset(ctx)
    check_golden_f64(ctx, z)


def test_min_sum_refusals_hold(data_dir):
    """syn, the iteration profile and the soft-syndrome metric are refused as in the f32 format."""
    hdr, z = load_case("bg2_16qam_known")
    s = stream(data_dir, "bg2")
    ctx = h16_ctx(data_dir, "bg2")
    B = z["v_p0"].shape[0]
    with pytest.raises(K.KmlError, match=UNSUP):
        ctx.bp_decode(z["v_p0"], syn=np.full((B, ctx.M), -1.0))
    assert "syn" in K.lib().kml_last_error(ctx._h).decode()
    ctx.sim_load(s["snr"], s["uu"][:8].astype(np.uint8), s["y"][:8], s["th"][:8])
    with pytest.raises(K.KmlError, match=UNSUP):
        ctx.sim_decode_profile(s["snr"])
    assert ctx.messages == "f16" and ctx.algorithm[0] == "nms"
    reset(ctx)
    check_golden_f64(ctx, z)
    soft = h16_ctx(data_dir, "bg2", metric_soft=True)
    with pytest.raises(K.KmlError, match=UNSUP):
        soft.decode_frames(s["y"][:4], s["snr"])
    assert "soft-syndrome" in K.lib().kml_last_error(soft._h).decode()
    assert soft.messages == "f16"
    reset(soft)
    check_golden_f64(soft, z)


@pytest.mark.parametrize("case", ["peg2304_qpsk_known", "peg8064_qpsk_known"])
def test_other_codes_refuse_the_format(data_dir, case):
    hdr, z = load_case(case)
    ctx = K.Context(matrix_file=os.path.join(data_dir, hdr["matrix"]), modem_file=os.path.join(data_dir, hdr["modem"]),
                    is5g=bool(hdr["is5g"]), max_iter=hdr["max_iter"], device=0)
    with pytest.raises(K.KmlError, match=UNSUP):  # the algorithm's refusal comes first
        ctx.set_algorithm("nms")
    with pytest.raises(K.KmlError, match=UNSUP):
        ctx.set_messages("f16")
    assert ctx.messages == "f32" and ctx.algorithm[0] == "spa"
    check_golden_f64(ctx, z)
    ctx.close()


def test_generic_kernel_refuses_f16(data_dir):
    """KML_BP_KERNEL is read once per process: a child started with KML_BP_KERNEL=generic."""
    env = dict(os.environ, PYTHONPATH=REPO, KML_BP_KERNEL="generic")
    p = subprocess.run([sys.executable, os.path.join(TESTS, "h16_generic_child.py"), data_dir], env=env,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "refused" in p.stdout


def test_drivers_take_the_format(data_dir, tmp_path):
    """kmldpc_sim and python -m kmldpc_amd.simulate: --messages / KML_MESSAGES, stated in the line after the
    schedule's; the same frames give the same lines in both drivers, and their counts are those of the
    Python face on the same generated frames."""
    from test_gpu_driver import _messages
    from conftest import write_config
    from kmldpc_amd.simulate import point_seed
    cfg = tmp_path / "config.toml"
    write_config(str(cfg), data_dir, CODES["bg2"][0], CODES["bg2"][3], is5g=True, known=True, max_iter=50, snr=7.0,
                 max_blocks=256, max_err=1000000)
    env = dict(os.environ, KML_BATCH="256", KML_SEED="4", PYTHONPATH=REPO)
    for k in ("KML_ALGORITHM", "KML_SCHEDULE", "KML_DEMAPPER", "KML_MESSAGES"):
        env.pop(k, None)
    exe = os.path.join(REPO, "kmldpc_amd", "bin", "kmldpc_sim")
    py = [sys.executable, "-m", "kmldpc_amd.simulate"]
    run = lambda cmd, e=env: subprocess.run(cmd, cwd=tmp_path, env=e, capture_output=True, text=True, timeout=120)
    r1 = run([exe, "--algorithm", "nms", "--schedule", "layered", "--messages", "f16", str(cfg)])
    r2 = run(py + [str(cfg)], dict(env, KML_ALGORITHM="nms", KML_SCHEDULE="layered", KML_MESSAGES="f16"))
    f32 = run([exe, "--algorithm", "nms", "--schedule", "layered", "--messages=f32", str(cfg)])
    for r in (r1, r2, f32):
        assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-1000:]
    m1, m2, mf = (_messages(r.stdout) for r in (r1, r2, f32))
    assert m1[1] == "BP decode schedule: layered" and m1[2].startswith("BP message format: f16")
    assert m1[3] == "Start simulation"
    assert m1[:-1] == m2[:-1]
    assert mf[2] == "Start simulation" and not any("message format" in x for x in mf)  # no added line by default
    res = [x for x in m1 if x.startswith("SNR = ")]
    got = re.search(r"Total blk = (\d+) Error blk = (\d+) Error bit = (\d+)", res[-1])  # the point's last line
    ctx = h16_ctx(data_dir, "bg2")
    ctx.sim_generate(7.0, 256, seed=point_seed(4, 0))  # the drivers' one round of 256 frames
    c = ctx.sim_decode(7.0)
    assert ctx.bp_kernel() == H16_KERNEL
    assert tuple(int(x) for x in got.groups()) == (c["tot_blk"], c["err_blk"], c["err_bit"])
    assert c["tot_blk"] == 256 and 0 < c["err_blk"] < 256
    reset(ctx)
    bad = run([exe, "--algorithm", "nms", "--messages", "f16", str(cfg)])  # without layered
    assert bad.returncode == 255 and "--messages" in bad.stdout
    assert run(py + ["--algorithm", "nms", "--messages", "f16", str(cfg)]).returncode == 2  # argparse's usage error
