"""GPU tests of the LLR front end of the min-sum mode: the max-log demapper
(kml_demap_llr, kmldpc_amd/csrc/demap_llr.hip), the LLR instances of the two
min-sum kernels (kml_llr_decode) and the per-context switch that puts both on the
receive path (kml_set_demapper, KML_DEMAP_MAXLOG).  Every comparison is equality
of bit patterns against the numpy models of tests/bp_llr_model.py; there is no
tolerance anywhere.  Nothing of it leaks into the exact front end or the fp64
paths.

Codes, streams and the models' decodes come from test_bp_llr_model.py and
test_bp_lnms_model.py, made once per session.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from bp_llr_model import blind_metric, llr_decode_model, maxlog_llr
from bp_lnms_model import lnms_model
from bp_nms_model import nms_model, priors
from conftest import REPO, TESTS, load_case
from test_bp_llr_model import SCHEDULES, clamp_inputs, llr_decoded, llr_stream, points
from test_bp_lnms_model import CODES, QC, code, stream
from test_bp_nms_model import saturated_p0
from test_gpu_device_ptrs import DeviceBufs, filled
from test_gpu_nms import assert_equals_model, check_golden_f64

import kmldpc_amd as K

pytestmark = pytest.mark.gpu

KERNEL = {"flooding": "bp_irregular_nms_kernel", "layered": "bp_irregular_lnms_kernel"}
SPA_KERNEL = "bp_irregular_kernel"
N = 64  # stream codewords per comparison
UNSUP = r"\(code -4\)"

_ctx = {}


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def ctx_for(data_dir, name, **kw):
    """One context per code (and option set); every test leaves it in SPA mode: flooding, exact demapper."""
    key = (name,) + tuple(sorted(kw.items()))
    if key not in _ctx:
        matrix, is5g, max_iter, modem, _ = CODES[name]
        _ctx[key] = K.Context(matrix_file=os.path.join(data_dir, matrix), modem_file=os.path.join(data_dir, modem),
                              is5g=is5g, max_iter=max_iter, device=0, **kw)
    return _ctx[key]


def nms_ctx(data_dir, name, schedule, alpha=None, demapper="exact", **kw):
    ctx = ctx_for(data_dir, name, **kw)
    ctx.set_algorithm("nms", alpha)
    ctx.set_schedule(schedule)
    ctx.set_demapper(demapper)
    assert (ctx.schedule, ctx.demapper) == (schedule, demapper)
    return ctx


def reset(ctx):
    ctx.set_algorithm("spa")
    assert ctx.schedule == "flooding" and ctx.demapper == "exact"


def assert_equals_llr_model(r, m, what):
    assert_equals_model(r, m, what)
    if "llr_out" in r:
        bad = np.nonzero((u32(r["llr_out"]) != u32(m["llr_out"])).any(axis=1))[0]
        assert bad.size == 0, f"{what}: llr_out differs from the model on codewords {bad[:8]} ({bad.size} in all)"


# ---- demap_llr = model -----------------------------------------------------

@pytest.mark.parametrize("name", list(CODES))
def test_demap_llr_equals_model(data_dir, name):
    """16QAM, 64QAM and QPSK on the streams (the model's LLRs are test_bp_llr_model's, shared)."""
    s = stream(data_dir, name)
    ctx = ctx_for(data_dir, name)
    got = ctx.demap_llr(s["y"][:N], s["th"][:N], 10.0 ** (-0.1 * s["snr"]))
    want = llr_stream(data_dir, name)[:N]
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(u32(got), u32(want))
    assert ctx.demapper == "exact" and ctx.algorithm[0] == "spa"  # a pure demapper, in any mode


@pytest.mark.parametrize("modem,matrix", [("syn_1bit_BPSK.txt", "syn_reg36_192.txt"),
                                          ("syn_3bits_8PSK_Gray.txt", "syn_reg36_192.txt"),
                                          ("syn_3bits_star8.txt", "PEG2304regular0.5.txt")])
def test_demap_llr_synthetic_constellations(data_dir, modem, matrix):
    """1 and 3 bits per symbol, on codes the min-sum mode does not take."""
    ctx = K.Context(matrix_file=os.path.join(data_dir, matrix), modem_file=os.path.join(data_dir, modem), device=0)
    rng = np.random.default_rng(len(modem) + ctx.S)
    B = 5
    pts = ctx.constellation()
    hc = rng.uniform(0.8, 1.5, B) * np.exp(2j * np.pi * rng.random(B))
    h = np.stack([hc.real, hc.imag], axis=-1)
    lab = rng.integers(0, ctx.Kc, (B, ctx.S))
    tx = (pts[lab][..., 0] + 1j * pts[lab][..., 1]) * hc[:, None]
    y = np.stack([tx.real, tx.imag], axis=-1) + 0.1 * rng.normal(size=(B, ctx.S, 2))
    got = ctx.demap_llr(y, h, 0.18)
    want = maxlog_llr(pts, ctx.bits, y, h, 0.18)
    assert np.array_equal(u32(got), u32(want))
    k = np.arange(ctx.bits)
    sent = ((lab[:, :, None] >> (ctx.bits - 1 - k)[None, None, :]) & 1).reshape(B, -1)
    assert np.mean((got > 0) == (sent == 0)) > 0.8  # and they are LLRs of the bits that were sent
    ctx.close()


def test_demap_llr_special_inputs(data_dir):
    """y exactly on a point (d = 0), y = 0, h = 0 (every L is +0), -0 inputs and values whose distances are
    float32 denormals, in one call of 7 codewords, at two noise variances."""
    ctx = ctx_for(data_dir, "bg2")
    pts, bits = points(data_dir, "bg2")
    S = ctx.S
    rng = np.random.default_rng(12)
    p32 = pts.astype(np.float32).astype(np.float64)
    y = rng.normal(size=(7, S, 2))
    h = rng.normal(size=(7, 2))
    y[0], h[0] = p32[rng.integers(0, 16, S)], [1.0, 0.0]
    y[1] = 0.0
    h[2] = 0.0
    y[3], h[3] = 1e-21 * rng.normal(size=(S, 2)), [1e-21, -2e-21]
    y[4], h[4] = 0.0, 0.0
    y[5], h[5] = p32[rng.integers(0, 16, S)] * [1.0, -1.0], [0.0, 0.0]
    y[5, ::2] = -0.0
    for var in (0.2, 1e-3):
        got = ctx.demap_llr(y, h, var)
        want = maxlog_llr(pts, bits, y, h, var)
        assert np.array_equal(u32(got), u32(want)), var
    assert not got[2].any() and not np.signbit(got[2]).any() and not u32(got[4]).any()
    d = (np.float32(1e-21) * np.float32(0.7)) ** 2
    assert 0 < d < np.finfo(np.float32).tiny  # (codeword 3's distances are denormal)
    assert np.isfinite(got[3]).all() and got[3].any()


@pytest.mark.parametrize("name", ["bg2", QC])
def test_demap_llr_batches_and_device_pointers(data_dir, name):
    """B = 1, 3 and 700, and one KML_DEVICE_PTRS call.  700 BG2 codewords are 336,000 symbols: 1312 tiles of
    256 and a partial one; 700 syn_qc_l200 codewords are 560,000: 2187 tiles and a partial one, more than
    the grid's 8 workgroups per CU, so workgroups stride to a second tile."""
    s = stream(data_dir, name)
    ctx = ctx_for(data_dir, name)
    assert 700 * ctx.S == {"bg2": 336000, QC: 560000}[name] and (700 * ctx.S) % 256 != 0
    var = 10.0 ** (-0.1 * s["snr"])
    n = s["y"].shape[0]
    y = np.concatenate([s["y"]] * (700 // n + 1))[:700]
    h = np.concatenate([s["th"]] * (700 // n + 1))[:700]
    want = llr_stream(data_dir, name)
    big = ctx.demap_llr(y, h, var)
    assert np.array_equal(u32(big[:n]), u32(want))
    assert np.array_equal(u32(big[n:700]), u32(big[:700 - n]))
    for B in (1, 3):
        assert np.array_equal(u32(ctx.demap_llr(y[:B], h[:B], var)), u32(want[:B])), B
    B = 3
    out = filled((B, ctx.cc_len), np.float32)
    with DeviceBufs() as d:
        d_y, d_h, d_o = d.put(np.ascontiguousarray(y[:B])), d.put(np.ascontiguousarray(h[:B])), d.put(out)
        assert K.lib().kml_demap_llr(ctx._h, d_y, d_h, var, B, d_o, K.KML_DEVICE_PTRS) == 0
        assert np.array_equal(u32(d.get(d_o, out)), u32(want[:B]))


# ---- llr_decode = model ----------------------------------------------------

@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("name,budget", [("bg2", 50), ("bg2", 5), ("bg2", 1), ("bg2", 0), ("syn_irr1200", 20),
                                         (QC, 20)])
def test_llr_decode_equals_model(data_dir, name, budget, schedule):
    ctx = nms_ctx(data_dir, name, schedule)
    llr = llr_stream(data_dir, name)[:N]
    m = llr_decoded(data_dir, name, f"stream{N}", llr, budget, schedule=schedule)
    r = ctx.llr_decode(llr, budget, cc_hat=True, llr_out=True)
    assert ctx.bp_kernel() == KERNEL[schedule]
    assert_equals_llr_model(r, m, f"{name} {schedule} budget {budget}")
    max_iter = CODES[name][2]
    if budget == max_iter:  # both outcomes are in the comparison
        assert np.any(m["ret"] == max_iter) and np.any(m["ret"] < max_iter)
    reset(ctx)


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_zero_iterations_leave_the_outputs(data_dir, schedule):
    ctx = nms_ctx(data_dir, "bg2", schedule)
    B = 5
    llr = np.ascontiguousarray(llr_stream(data_dir, "bg2")[:B])
    uh, cch = np.full((B, ctx.K), 7, np.uint8), np.full((B, ctx.Ncol), 9, np.uint8)
    ret, post = np.full(B, -5, np.int32), np.full((B, ctx.Ncol), -3.5, np.float32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert K.lib().kml_llr_decode(ctx._h, ptr(llr), B, 0, ptr(uh), ptr(ret), ptr(cch), ptr(post), 0) == 0
    assert np.all(uh == 7) and np.all(cch == 9) and np.all(post == np.float32(-3.5))
    assert np.all(ret == 1)
    reset(ctx)


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("alpha", [1.0, 0.8125])
def test_alpha(data_dir, alpha, schedule):
    ctx = nms_ctx(data_dir, "bg2", schedule, alpha)
    llr = llr_stream(data_dir, "bg2")[:N]
    m = llr_decoded(data_dir, "bg2", f"stream{N}", llr, 50, alpha, schedule)
    base = llr_decoded(data_dir, "bg2", f"stream{N}", llr, 50, schedule=schedule)
    assert (m["cc_hat"] != base["cc_hat"]).any()  # the factor matters on these codewords
    r = ctx.llr_decode(llr, 50, cc_hat=True, llr_out=True)
    assert_equals_llr_model(r, m, f"{schedule} alpha {alpha}")
    reset(ctx)


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_clamp_inputs(data_dir, schedule):
    """+-inf, +-1e30, +-256, just past 256, +-0 and denormals: the kernel decodes their clamped values."""
    _, g = code(data_dir, "bg2")
    x = clamp_inputs(g, llr_stream(data_dir, "bg2")[0].copy())
    m = llr_decoded(data_dir, "bg2", "clamp", x, 50, schedule=schedule)
    ctx = nms_ctx(data_dir, "bg2", schedule)
    r = ctx.llr_decode(x, 50, cc_hat=True, llr_out=True)
    assert_equals_llr_model(r, m, f"clamp inputs, {schedule}")
    r2 = ctx.llr_decode(np.clip(x, -256.0, 256.0), 50, cc_hat=True, llr_out=True)
    assert_equals_llr_model(r2, m, f"clamped inputs, {schedule}")
    reset(ctx)


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_batch_and_queue_independence(data_dir, schedule):
    """B = 1, 3 and 700 (beyond the resident workgroups), each twice; with and without llr_out the same bits."""
    ctx = nms_ctx(data_dir, "bg2", schedule)
    llr = llr_stream(data_dir, "bg2")
    n = llr.shape[0]
    big = np.concatenate([llr] * (700 // n + 1))[:700]
    runs = {}
    for tag, B in [("1", 1), ("3", 3), ("700", 700), ("1 again", 1), ("3 again", 3), ("700 again", 700)]:
        runs[tag] = ctx.llr_decode(big[:B], 50, cc_hat=True, llr_out=True)
        assert ctx.bp_kernel() == KERNEL[schedule]
    for key in ("uu_hat", "ret", "cc_hat", "llr_out"):
        bits = (lambda a: u32(a)) if key == "llr_out" else (lambda a: a)
        for tag in ("1", "3", "700"):
            assert np.array_equal(bits(runs[tag][key]), bits(runs[tag + " again"][key])), (tag, key)
        assert np.array_equal(bits(runs["1"][key]), bits(runs["700"][key][:1])), key
        assert np.array_equal(bits(runs["3"][key]), bits(runs["700"][key][:3])), key
        assert np.array_equal(bits(runs["700"][key][n:700]), bits(runs["700"][key][:700 - n])), key
    m = llr_decoded(data_dir, "bg2", f"stream{N}", llr[:N], 50, schedule=schedule)
    assert_equals_llr_model({k: v[:N] for k, v in runs["700"].items()}, m, "B = 700")
    plain = ctx.llr_decode(big, 50, cc_hat=True)  # the instance without the posterior output
    for key in ("uu_hat", "ret", "cc_hat"):
        assert np.array_equal(plain[key], runs["700"][key]), key
    reset(ctx)


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_tie_to_the_old_entry(data_dir, schedule):
    """llr_decode(priors(p0)) equals bp_decode(p0): stream and saturated priors (P0 of exactly 0, 1, 0.5)."""
    _, g = code(data_dir, "bg2")
    ctx = nms_ctx(data_dir, "bg2", schedule)
    for p0 in (stream(data_dir, "bg2")["p0"][:N], saturated_p0(data_dir)):
        old = ctx.bp_decode(p0, 50, cc_hat=True)
        new = ctx.llr_decode(priors(g, p0)[:, g.punct:], 50, cc_hat=True)
        for key in ("uu_hat", "ret", "cc_hat"):
            assert np.array_equal(old[key], new[key]), key
    reset(ctx)


def test_device_pointers(data_dir):
    ctx = nms_ctx(data_dir, "bg2", "layered")
    B = 3
    llr = np.ascontiguousarray(llr_stream(data_dir, "bg2")[:B])
    host = ctx.llr_decode(llr, 50, cc_hat=True, llr_out=True)
    uh, ret = filled((B, ctx.K), np.uint8), filled(B, np.int32)
    cch, post = filled((B, ctx.Ncol), np.uint8), filled((B, ctx.Ncol), np.float32)
    with DeviceBufs() as d:
        d_l, d_uh, d_ret, d_cch, d_po = d.put(llr), d.put(uh), d.put(ret), d.put(cch), d.put(post)
        assert K.lib().kml_llr_decode(ctx._h, d_l, B, 50, d_uh, d_ret, d_cch, d_po, K.KML_DEVICE_PTRS) == 0
        assert np.array_equal(d.get(d_uh, uh), host["uu_hat"])
        assert np.array_equal(d.get(d_ret, ret), host["ret"])
        assert np.array_equal(d.get(d_cch, cch), host["cc_hat"])
        assert np.array_equal(u32(d.get(d_po, post)), u32(host["llr_out"]))
    reset(ctx)


# ---- the switch on the receive path ----------------------------------------

@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("name", ["bg2", "syn_irr1200"])
def test_switch_known_channel(data_dir, name, schedule):
    s = stream(data_dir, name)
    max_iter = CODES[name][2]
    m = llr_decoded(data_dir, name, f"stream{N}", llr_stream(data_dir, name)[:N], max_iter, schedule=schedule)
    ctx = nms_ctx(data_dir, name, schedule, demapper="maxlog")
    r = ctx.decode_frames(s["y"][:N], s["snr"], s["th"][:N])
    assert ctx.bp_kernel() == KERNEL[schedule]
    assert np.array_equal(r["uu_hat"], m["uu_hat"]) and np.array_equal(r["ret"], m["ret"])
    ctx.set_demapper("exact")  # and back: the exact front end of the same mode
    e = ctx.decode_frames(s["y"][:N], s["snr"], s["th"][:N])
    model = {"flooding": nms_model, "layered": lnms_model}[schedule]
    ret, uh, _ = model(code(data_dir, name)[1], s["p0"][:N], max_iter, max_iter)
    assert np.array_equal(e["uu_hat"], uh) and np.array_equal(e["ret"], ret)
    reset(ctx)


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_switch_blind_bg2(data_dir, schedule):
    """chosen, metrics, uu_hat and ret are the model's on ctx.kmeans's candidates (the metric decodes read
    demap_llr's reps = 4 addressing, the final decode its h_sel addressing); h_hat is the exact mode's."""
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
    ctx = nms_ctx(data_dir, "bg2", schedule, demapper="maxlog")
    out = ctx.decode_frames(y, snr)
    assert ctx.bp_kernel() == KERNEL[schedule]
    met, chosen, llrs = blind_metric(g, pts, bits, y, h4, var, 5, 50, schedule=schedule)
    assert np.array_equal(out["chosen"], chosen)
    assert np.array_equal(out["metrics"], met)
    assert np.array_equal(out["h_hat"], ref["h_hat"])  # k-means is untouched
    assert len(set(chosen.tolist())) > 1               # more than one rotation is chosen
    assert (out["metrics"] != ref["metrics"]).any()    # a min-sum receiver's metrics, not the reference's
    ret, uh, _, _ = llr_decode_model(g, llrs[np.arange(n), chosen], 50, 50, schedule=schedule)
    assert np.array_equal(out["uu_hat"], uh) and np.array_equal(out["ret"], ret)
    # the caller's candidates: two of them
    met2, chosen2, llrs2 = blind_metric(g, pts, bits, y, h4[:, :2], var, 5, 50, schedule=schedule)
    out2 = ctx.decode_candidates(y, h4[:, :2], snr)
    ret2, uh2, _, _ = llr_decode_model(g, llrs2[np.arange(n), chosen2], 50, 50, schedule=schedule)
    assert np.array_equal(out2["chosen"], chosen2) and np.array_equal(out2["metrics"], met2)
    assert np.array_equal(out2["uu_hat"], uh2) and np.array_equal(out2["ret"], ret2)
    # histogram mode: the metrics only; uu_hat is what the last candidate's metric decode left
    hist = ctx.decode_frames(y, snr, histogram=True)
    assert np.array_equal(hist["chosen"], chosen) and np.array_equal(hist["metrics"], met)
    assert np.array_equal(hist["uu_hat"], llr_decode_model(g, llrs[:, 3], 5, 50, schedule=schedule)[1])
    hist2 = ctx.decode_candidates(y, h4[:, :2], snr, histogram=True)
    assert np.array_equal(hist2["chosen"], chosen2) and np.array_equal(hist2["metrics"], met2)
    reset(ctx)


def test_switch_blind_syn_irr1200(data_dir):
    """A non-5G code keeps the hard metric on the exact demapper's output: chosen and metrics are the exact
    mode's bit for bit, only the final decode's priors change."""
    n = 32
    name = "syn_irr1200"
    s = stream(data_dir, name)
    y, snr = s["y"][:n], s["snr"]
    _, g = code(data_dir, name)
    pts, bits = points(data_dir, name)
    ctx = nms_ctx(data_dir, name, "layered")
    ref = ctx.decode_frames(y, snr)
    _, h4 = ctx.kmeans(y)
    ctx.set_demapper("maxlog")
    out = ctx.decode_frames(y, snr)
    assert ctx.bp_kernel() == KERNEL["layered"]
    for key in ("chosen", "metrics", "h_hat"):
        assert np.array_equal(out[key], ref[key]), key
    llr = maxlog_llr(pts, bits, y, h4[np.arange(n), out["chosen"]], 10.0 ** (-0.1 * snr))
    ret, uh, _, _ = llr_decode_model(g, llr, 20, 20, schedule="layered")
    assert np.array_equal(out["uu_hat"], uh) and np.array_equal(out["ret"], ret)
    assert (out["uu_hat"] != ref["uu_hat"]).any()  # other priors, another decode
    reset(ctx)


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_simulator_path(data_dir, schedule):
    n = 128
    s = stream(data_dir, "bg2", n)
    _, g = code(data_dir, "bg2")
    m = llr_decoded(data_dir, "bg2", f"stream{n}", llr_stream(data_dir, "bg2", n), 50, schedule=schedule)
    uu = s["uu"].astype(np.uint8)
    want = (m["uu_hat"] != uu).sum(axis=1).astype(np.int32)
    it, conv = m["stats"]["iters"], m["stats"]["converged"]
    ctx = nms_ctx(data_dir, "bg2", schedule, demapper="maxlog")
    ctx.sim_load(s["snr"], uu, s["y"], s["th"])
    err, _, cnt = ctx.sim_decode_ex(s["snr"])
    assert ctx.bp_kernel() == KERNEL[schedule]
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


# ---- nothing leaks into the other paths ------------------------------------

def test_no_leakage(data_dir):
    """The fp64 golden vectors (syn included) and the exact-front-end min-sum decodes match their models
    before a max-log decode and again after it, on one context."""
    hdr, z = load_case("bg2_16qam_known")
    assert (hdr["matrix"], hdr["modem"], hdr["max_iter"]) == (CODES["bg2"][0], CODES["bg2"][3], CODES["bg2"][2])
    _, g = code(data_dir, "bg2")
    s = stream(data_dir, "bg2")
    p0 = z["v_p0"]
    flood = dict(zip(("ret", "uu_hat", "cc_hat"), nms_model(g, p0, 50, 50)))
    lay = dict(zip(("ret", "uu_hat", "cc_hat"), lnms_model(g, p0, 50, 50)))
    y, th, snr = s["y"][:8], s["th"][:8], s["snr"]
    exact_known = lnms_model(g, s["p0"][:8], 50, 50)
    ctx = ctx_for(data_dir, "bg2")
    reset(ctx)

    def exact_paths():
        check_golden_f64(ctx, z)
        assert ctx.bp_kernel() == SPA_KERNEL
        ctx.set_algorithm("nms")
        assert ctx.demapper == "exact"
        assert_equals_model(ctx.bp_decode(p0, cc_hat=True), flood, "flooding, exact front end")
        ctx.set_schedule("layered")
        assert_equals_model(ctx.bp_decode(p0, cc_hat=True), lay, "layered, exact front end")
        r = ctx.decode_frames(y, snr, th)
        assert np.array_equal(r["uu_hat"], exact_known[1]) and np.array_equal(r["ret"], exact_known[0])

    exact_paths()
    ctx.set_demapper("maxlog")
    ctx.set_schedule("flooding")    # keeps the demapper
    assert ctx.demapper == "maxlog"
    ctx.set_algorithm("nms", 0.8125)  # and so does a new alpha
    assert ctx.demapper == "maxlog" and ctx.algorithm == ("nms", 0.8125)
    ctx.set_algorithm("nms")
    m = llr_decoded(data_dir, "bg2", f"stream{N}", llr_stream(data_dir, "bg2")[:N], 50, schedule="flooding")
    r = ctx.decode_frames(y, snr, th)
    assert np.array_equal(r["uu_hat"], m["uu_hat"][:8])
    ctx.decode_frames(y, snr)       # a blind max-log receive, metric decodes included
    assert_equals_model(ctx.bp_decode(p0, cc_hat=True), flood, "kml_bp_decode does not read the switch")
    assert np.array_equal(ctx.demap(y, th, 10.0 ** (-0.1 * snr)), s["p0"][:8])  # nor does kml_demap
    ctx.set_algorithm("spa")        # leaves the min-sum mode, its schedule and its front end
    assert ctx.demapper == "exact" and ctx.schedule == "flooding"
    exact_paths()
    reset(ctx)
    check_golden_f64(ctx, z)


# ---- refusals: KML_E_UNSUP, the demapper kept, the fp64 decode intact --------

def test_maxlog_needs_the_min_sum_mode(data_dir):
    hdr, z = load_case("bg2_16qam_known")
    ctx = ctx_for(data_dir, "bg2")
    reset(ctx)
    with pytest.raises(K.KmlError, match=UNSUP):
        ctx.set_demapper("maxlog")
    assert "min-sum" in K.lib().kml_last_error(ctx._h).decode()
    with pytest.raises(K.KmlError, match=UNSUP):
        ctx.llr_decode(llr_stream(data_dir, "bg2")[:2])
    assert "min-sum" in K.lib().kml_last_error(ctx._h).decode()
    with pytest.raises(K.KmlError, match=r"\(code -1\)"):
        ctx.set_demapper("approx")
    assert ctx.demapper == "exact" and ctx.algorithm[0] == "spa"
    check_golden_f64(ctx, z)
    assert ctx.bp_kernel() == SPA_KERNEL


@pytest.mark.parametrize("case", ["peg2304_qpsk_known", "peg8064_qpsk_known"])
def test_other_codes_refuse_the_front_end(data_dir, case):
    hdr, z = load_case(case)
    ctx = K.Context(matrix_file=os.path.join(data_dir, hdr["matrix"]), modem_file=os.path.join(data_dir, hdr["modem"]),
                    is5g=bool(hdr["is5g"]), max_iter=hdr["max_iter"], device=0)
    with pytest.raises(K.KmlError, match=UNSUP):  # the algorithm's refusal comes first
        ctx.set_algorithm("nms")
    with pytest.raises(K.KmlError, match=UNSUP):
        ctx.set_demapper("maxlog")
    with pytest.raises(K.KmlError, match=UNSUP):
        ctx.llr_decode(np.zeros((2, ctx.cc_len), np.float32), llr_out=True)
    assert ctx.demapper == "exact" and ctx.algorithm[0] == "spa"
    rng = np.random.default_rng(4)  # the pure demapper works on any code
    y, h = rng.normal(size=(2, ctx.S, 2)), rng.normal(size=(2, 2))
    assert np.array_equal(u32(ctx.demap_llr(y, h, 0.5)), u32(maxlog_llr(ctx.constellation(), ctx.bits, y, h, 0.5)))
    check_golden_f64(ctx, z)
    ctx.close()


def test_soft_metric_is_refused(data_dir):
    hdr, z = load_case("bg2_16qam_known")
    ctx = nms_ctx(data_dir, "bg2", "layered", demapper="maxlog", metric_soft=True)
    s = stream(data_dir, "bg2")
    with pytest.raises(K.KmlError, match=UNSUP):
        ctx.decode_frames(s["y"][:4], s["snr"])
    assert "soft-syndrome" in K.lib().kml_last_error(ctx._h).decode()
    assert ctx.demapper == "maxlog"
    r = ctx.decode_frames(s["y"][:4], s["snr"], s["th"][:4])  # the known channel has no metric: it decodes
    m = llr_decoded(data_dir, "bg2", f"stream{N}", llr_stream(data_dir, "bg2")[:N], 50, schedule="layered")
    assert np.array_equal(r["uu_hat"], m["uu_hat"][:4])
    reset(ctx)
    check_golden_f64(ctx, z)


def test_syn_and_the_iteration_profile_are_refused(data_dir):
    hdr, z = load_case("bg2_16qam_known")
    s = stream(data_dir, "bg2")
    ctx = nms_ctx(data_dir, "bg2", "flooding", demapper="maxlog")
    B = z["v_p0"].shape[0]
    with pytest.raises(K.KmlError, match=UNSUP):
        ctx.bp_decode(z["v_p0"], syn=np.full((B, ctx.M), -1.0))
    assert "syn" in K.lib().kml_last_error(ctx._h).decode()
    ctx.sim_load(s["snr"], s["uu"][:8].astype(np.uint8), s["y"][:8], s["th"][:8])
    with pytest.raises(K.KmlError, match=UNSUP):
        ctx.sim_decode_profile(s["snr"])
    assert "min-sum" in K.lib().kml_last_error(ctx._h).decode()
    assert ctx.demapper == "maxlog" and ctx.algorithm[0] == "nms"
    reset(ctx)
    ctx.sim_decode_profile(s["snr"])  # and it is back in SPA mode
    check_golden_f64(ctx, z)


def test_generic_kernel_refuses_maxlog(data_dir):
    """KML_BP_KERNEL is read once per process: a child started with KML_BP_KERNEL=generic."""
    env = dict(os.environ, PYTHONPATH=REPO, KML_BP_KERNEL="generic")
    p = subprocess.run([sys.executable, os.path.join(TESTS, "llr_generic_child.py"), data_dir], env=env,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "refused" in p.stdout


def test_drivers_take_the_demapper(data_dir, tmp_path):
    """kmldpc_sim and python -m kmldpc_amd.simulate: --demapper / KML_DEMAPPER, stated in the line after
    the schedule's; the same frames give the same lines in both drivers, other lines than the exact front
    end's, and a default run prints no added line."""
    from test_gpu_driver import _messages
    from conftest import write_config
    cfg = tmp_path / "config.toml"
    write_config(str(cfg), data_dir, CODES["bg2"][0], CODES["bg2"][3], is5g=True, known=True, max_iter=50, snr=7.0,
                 max_blocks=256, max_err=1000000)
    env = dict(os.environ, KML_BATCH="256", KML_SEED="4", PYTHONPATH=REPO)
    for k in ("KML_ALGORITHM", "KML_SCHEDULE", "KML_DEMAPPER"):
        env.pop(k, None)
    exe = os.path.join(REPO, "kmldpc_amd", "bin", "kmldpc_sim")
    py = [sys.executable, "-m", "kmldpc_amd.simulate"]
    run = lambda cmd, e=env: subprocess.run(cmd, cwd=tmp_path, env=e, capture_output=True, text=True, timeout=120)
    r1 = run([exe, "--algorithm", "nms", "--schedule", "layered", "--demapper", "maxlog", str(cfg)])
    r2 = run(py + [str(cfg)], dict(env, KML_ALGORITHM="nms", KML_SCHEDULE="layered", KML_DEMAPPER="maxlog"))
    exact = run([exe, "--algorithm", "nms", "--schedule", "layered", "--demapper=exact", str(cfg)])
    plain = run([exe, str(cfg)])
    for r in (r1, r2, exact, plain):
        assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-1000:]
    m1, m2, me, mp = (_messages(r.stdout) for r in (r1, r2, exact, plain))
    assert m1[1] == "BP decode schedule: layered" and m1[2].startswith("Demapper: maxlog")
    assert m1[3] == "Start simulation"
    assert m1[:-1] == m2[:-1]
    assert me[2] == "Start simulation" and mp[0] == "Start simulation"  # no added line by default
    assert not any("Demapper" in x for x in me + mp)
    res = lambda m: [x for x in m if x.startswith("SNR = ")]
    assert res(m1) and res(m1) != res(me)  # another front end on the same frames
    bad = run([exe, "--demapper", "maxlog", str(cfg)])  # without nms
    assert bad.returncode == 255 and "--demapper" in bad.stdout
    assert run([exe, "--algorithm", "nms", "--demapper", "approx", str(cfg)]).returncode == 255
    assert run(py + ["--demapper", "maxlog", str(cfg)]).returncode == 2  # argparse's usage error
    assert run(py + [str(cfg)], dict(env, KML_DEMAPPER="maxlog")).returncode == 2
