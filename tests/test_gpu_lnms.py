"""GPU tests of the layered schedule of the min-sum mode (kml_set_schedule,
KML_SCHED_LAYERED; kmldpc_amd/csrc/bp_irregular_lnms.hip).  The kernel equals the
numpy model (tests/bp_lnms_model.py) bit for bit on uu_hat, ret and cc_hat, its
results do not depend on the batch, and nothing of it leaks into the flooding
min-sum decoder or the fp64 paths.

The codes are 5G BG2 K960 with 16QAM (a layer is exactly one pass of the kernel),
syn_irr1200 with 64QAM (91 layers of 1 to 17 rows: mostly idle passes) and
syn_qc_l200 with QPSK (4 layers of 200 rows: two full passes and a partial one,
no barrier between them).  Streams, special inputs and the models' decodes come
from test_bp_lnms_model.py and test_bp_nms_model.py, made once per session.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from bp_lnms_model import lnms_model
from bp_nms_model import nms_model
from conftest import REPO, TESTS, load_case
from test_bp_lnms_model import CODES, QC, code, layered_decode, stream
from test_bp_nms_model import random_p0, saturated_p0
from test_gpu_device_ptrs import DeviceBufs, filled
from test_gpu_nms import assert_equals_model, check_golden_f64

import kmldpc_amd as K

pytestmark = pytest.mark.gpu

LNMS_KERNEL = "bp_irregular_lnms_kernel"
NMS_KERNEL = "bp_irregular_nms_kernel"
SPA_KERNEL = "bp_irregular_kernel"
N = 64  # stream codewords per comparison
UNSUP = r"\(code -4\)"

_ctx = {}


def ctx_for(data_dir, name, **kw):
    """One context per code (and option set); every test leaves it in SPA mode, flooding."""
    key = (name,) + tuple(sorted(kw.items()))
    if key not in _ctx:
        matrix, is5g, max_iter, modem, _ = CODES[name]
        _ctx[key] = K.Context(matrix_file=os.path.join(data_dir, matrix), modem_file=os.path.join(data_dir, modem),
                              is5g=is5g, max_iter=max_iter, device=0, **kw)
    return _ctx[key]


def layered_ctx(data_dir, name, alpha=None, **kw):
    ctx = ctx_for(data_dir, name, **kw)
    ctx.set_algorithm("nms", alpha)
    ctx.set_schedule("layered")
    assert ctx.schedule == "layered"
    assert ctx.algorithm == ("nms", float(np.float32(0.75 if alpha is None else alpha)))
    return ctx


def reset(ctx):
    ctx.set_algorithm("spa")
    assert ctx.schedule == "flooding"


# ---- kernel = model --------------------------------------------------------

@pytest.mark.parametrize("name,budget", [("bg2", 50), ("bg2", 5), ("bg2", 1), ("syn_irr1200", 20), (QC, 20)])
def test_kernel_equals_model(data_dir, name, budget):
    ctx = layered_ctx(data_dir, name)
    p0 = stream(data_dir, name)["p0"][:N]
    m = layered_decode(data_dir, name, f"stream{N}", p0, budget)
    r = ctx.bp_decode(p0, budget, cc_hat=True)
    assert ctx.bp_kernel() == LNMS_KERNEL
    assert_equals_model(r, m, f"{name} budget {budget}")
    max_iter = CODES[name][2]
    if budget == max_iter:  # both outcomes are in the comparison
        assert np.any(m["ret"] == max_iter) and np.any(m["ret"] < max_iter)
    reset(ctx)


def test_zero_iterations_leave_the_outputs(data_dir):
    ctx = layered_ctx(data_dir, "bg2")
    B = 5
    p0 = np.ascontiguousarray(stream(data_dir, "bg2")["p0"][:B])
    uh = np.full((B, ctx.K), 7, np.uint8)
    cch = np.full((B, ctx.Ncol), 9, np.uint8)
    ret = np.full(B, -5, np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert K.lib().kml_bp_decode(ctx._h, ptr(p0), B, 0, ptr(uh), ptr(ret), ptr(cch), None, 0) == 0
    assert ctx.bp_kernel() == LNMS_KERNEL
    assert np.all(uh == 7) and np.all(cch == 9)
    assert np.all(ret == 1)  # it = 0 < max_iter
    reset(ctx)


@pytest.mark.parametrize("alpha", [1.0, 0.8125])
def test_alpha(data_dir, alpha):
    ctx = layered_ctx(data_dir, "bg2", alpha)
    p0 = stream(data_dir, "bg2")["p0"][:N]
    m = layered_decode(data_dir, "bg2", f"stream{N}", p0, 50, alpha)
    base = layered_decode(data_dir, "bg2", f"stream{N}", p0, 50)
    assert (m["cc_hat"] != base["cc_hat"]).any()  # the factor matters on these codewords
    r = ctx.bp_decode(p0, 50, cc_hat=True)
    assert ctx.bp_kernel() == LNMS_KERNEL
    assert_equals_model(r, m, f"alpha {alpha}")
    reset(ctx)


@pytest.mark.parametrize("which", ["saturated", "random"])
def test_saturated_and_random_priors(data_dir, which):
    """P0 of exactly 0, 1, 0.5 and 1e-300, the all-0.5 codeword (messages in the +-256 clamp, zero
    magnitudes, ties), and uniform-random P0."""
    ctx = layered_ctx(data_dir, "bg2")
    p0 = saturated_p0(data_dir) if which == "saturated" else random_p0(data_dir)
    m = layered_decode(data_dir, "bg2", which, p0, 50)
    if which == "saturated":
        assert m["stats"]["max_abs_m"] == 256.0
    r = ctx.bp_decode(p0, 50, cc_hat=True)
    assert ctx.bp_kernel() == LNMS_KERNEL
    assert_equals_model(r, m, which)
    reset(ctx)


def test_batch_and_queue_independence(data_dir):
    """B = 700 exceeds the resident workgroups, so workgroups re-enter the dequeue loop."""
    ctx = layered_ctx(data_dir, "bg2")
    p0 = stream(data_dir, "bg2")["p0"]
    n = p0.shape[0]
    big = np.concatenate([p0] * (700 // n + 1))[:700]
    runs = {}
    for tag, B in [("1", 1), ("3", 3), ("700", 700), ("1 again", 1), ("3 again", 3), ("700 again", 700)]:
        runs[tag] = ctx.bp_decode(big[:B], 50, cc_hat=True)
        assert ctx.bp_kernel() == LNMS_KERNEL
    for key in ("uu_hat", "ret", "cc_hat"):
        for tag in ("1", "3", "700"):  # each batch decoded twice
            assert np.array_equal(runs[tag][key], runs[tag + " again"][key]), (tag, key)
        assert np.array_equal(runs["1"][key], runs["700"][key][:1]), key
        assert np.array_equal(runs["3"][key], runs["700"][key][:3]), key
        # the later copies of the stream sit at other queue positions
        assert np.array_equal(runs["700"][key][n:700], runs["700"][key][:700 - n]), key
    m = layered_decode(data_dir, "bg2", f"stream{N}", p0[:N], 50)
    assert_equals_model({k: v[:N] for k, v in runs["700"].items()}, m, "B = 700")
    reset(ctx)


# ---- nothing leaks into the other decoders ---------------------------------

def test_no_leakage_between_schedules(data_dir):
    hdr, z = load_case("bg2_16qam_known")
    assert (hdr["matrix"], hdr["modem"], hdr["max_iter"]) == (CODES["bg2"][0], CODES["bg2"][3], CODES["bg2"][2])
    _, g = code(data_dir, "bg2")
    p0 = z["v_p0"]
    flood = dict(zip(("ret", "uu_hat", "cc_hat"), nms_model(g, p0, 50, 50)))
    lay = dict(zip(("ret", "uu_hat", "cc_hat"), lnms_model(g, p0, 50, 50)))
    ctx = ctx_for(data_dir, "bg2")
    reset(ctx)
    check_golden_f64(ctx, z)  # syn included
    assert ctx.bp_kernel() == SPA_KERNEL
    ctx.set_algorithm("nms")
    assert_equals_model(ctx.bp_decode(p0, cc_hat=True), flood, "flooding before")
    assert ctx.bp_kernel() == NMS_KERNEL
    ctx.set_schedule("layered")
    assert_equals_model(ctx.bp_decode(p0, cc_hat=True), lay, "layered")
    assert ctx.bp_kernel() == LNMS_KERNEL
    ctx.set_schedule("flooding")
    assert ctx.schedule == "flooding" and ctx.algorithm[0] == "nms"
    assert_equals_model(ctx.bp_decode(p0, cc_hat=True), flood, "flooding after")
    assert ctx.bp_kernel() == NMS_KERNEL
    ctx.set_schedule("layered")
    ctx.set_algorithm("spa")  # leaves the min-sum mode and its schedule
    assert ctx.schedule == "flooding"
    check_golden_f64(ctx, z)
    assert ctx.bp_kernel() == SPA_KERNEL


def test_the_algorithm_switch_and_the_schedule(data_dir):
    ctx = layered_ctx(data_dir, "bg2")
    ctx.set_algorithm("nms", 0.8125)  # keeps the schedule
    assert ctx.schedule == "layered" and ctx.algorithm == ("nms", 0.8125)
    ctx.set_algorithm("spa")          # returns it to flooding
    assert ctx.schedule == "flooding"
    ctx.set_algorithm("nms")
    assert ctx.schedule == "flooding"  # and it stays there until asked again
    p0 = stream(data_dir, "bg2")["p0"][:3]
    ctx.bp_decode(p0, 5)
    assert ctx.bp_kernel() == NMS_KERNEL
    with pytest.raises(K.KmlError, match=r"\(code -1\)"):
        ctx.set_schedule("zigzag")
    reset(ctx)


def test_blind_path_front_end_untouched(data_dir):
    """k-means, the demapper and BG2's metric_iter decodes stay fp64 sum-product: chosen, metrics and
    h_hat are those of SPA mode, and uu_hat is the model's decode of demap(y, h_chosen)."""
    n = 32
    s = stream(data_dir, "bg2")
    y, snr = s["y"][:n], s["snr"]
    ctx = ctx_for(data_dir, "bg2")
    reset(ctx)
    ref = ctx.decode_frames(y, snr)
    assert ctx.bp_kernel() == SPA_KERNEL
    _, h4 = ctx.kmeans(y)
    ctx = layered_ctx(data_dir, "bg2")
    out = ctx.decode_frames(y, snr)
    assert ctx.bp_kernel() == LNMS_KERNEL
    for key in ("chosen", "metrics", "h_hat"):
        assert np.array_equal(out[key], ref[key]), key
    assert len(set(out["chosen"].tolist())) > 1  # more than one rotation is chosen
    p0 = ctx.demap(y, h4[np.arange(n), out["chosen"]], 10.0 ** (-0.1 * snr))
    _, g = code(data_dir, "bg2")
    ret, uh, _ = lnms_model(g, p0, 50, 50)
    assert np.array_equal(out["uu_hat"], uh)
    assert np.array_equal(out["ret"], ret)
    reset(ctx)


def test_simulator_path(data_dir):
    n = 256
    s = stream(data_dir, "bg2", n)
    _, g = code(data_dir, "bg2")
    m = layered_decode(data_dir, "bg2", f"stream{n}", s["p0"], 50)
    uu = s["uu"].astype(np.uint8)
    want = (m["uu_hat"] != uu).sum(axis=1).astype(np.int32)
    it, conv = m["stats"]["iters"], m["stats"]["converged"]
    ctx = layered_ctx(data_dir, "bg2")
    ctx.sim_load(s["snr"], uu, s["y"], s["th"])
    err, _, cnt = ctx.sim_decode_ex(s["snr"])
    assert ctx.bp_kernel() == LNMS_KERNEL
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
    ctx = layered_ctx(data_dir, "bg2")
    B = 3
    p0 = np.ascontiguousarray(stream(data_dir, "bg2")["p0"][:B])
    host = ctx.bp_decode(p0, 50, cc_hat=True)
    uh, ret, cch = filled((B, ctx.K), np.uint8), filled(B, np.int32), filled((B, ctx.Ncol), np.uint8)
    with DeviceBufs() as d:
        d_p0, d_uh, d_ret, d_cch = d.put(p0), d.put(uh), d.put(ret), d.put(cch)
        assert K.lib().kml_bp_decode(ctx._h, d_p0, B, 50, d_uh, d_ret, d_cch, None, K.KML_DEVICE_PTRS) == 0
        assert ctx.bp_kernel() == LNMS_KERNEL
        assert np.array_equal(d.get(d_uh, uh), host["uu_hat"])
        assert np.array_equal(d.get(d_ret, ret), host["ret"])
        assert np.array_equal(d.get(d_cch, cch), host["cc_hat"])
    m = layered_decode(data_dir, "bg2", f"stream{N}", stream(data_dir, "bg2")["p0"][:N], 50)
    assert np.array_equal(host["uu_hat"], m["uu_hat"][:B])
    reset(ctx)


def test_layers_on_a_gpu_context(data_dir):
    for name, want in (("bg2", 12), ("syn_irr1200", 91), (QC, 4)):
        assert len(ctx_for(data_dir, name).layers()) - 1 == want


# ---- refusals: KML_E_UNSUP, the schedule kept, the fp64 decode intact --------

def test_layered_needs_the_min_sum_mode(data_dir):
    hdr, z = load_case("bg2_16qam_known")
    ctx = ctx_for(data_dir, "bg2")
    reset(ctx)
    with pytest.raises(K.KmlError, match=UNSUP):
        ctx.set_schedule("layered")
    assert "min-sum" in K.lib().kml_last_error(ctx._h).decode()
    assert ctx.schedule == "flooding" and ctx.algorithm[0] == "spa"
    check_golden_f64(ctx, z)
    assert ctx.bp_kernel() == SPA_KERNEL


@pytest.mark.parametrize("case", ["peg2304_qpsk_known", "peg8064_qpsk_known"])
def test_other_codes_refuse_layered(data_dir, case):
    hdr, z = load_case(case)
    ctx = K.Context(matrix_file=os.path.join(data_dir, hdr["matrix"]), modem_file=os.path.join(data_dir, hdr["modem"]),
                    is5g=bool(hdr["is5g"]), max_iter=hdr["max_iter"], device=0)
    with pytest.raises(K.KmlError, match=UNSUP):  # the algorithm's refusal comes first
        ctx.set_algorithm("nms")
    with pytest.raises(K.KmlError, match=UNSUP):
        ctx.set_schedule("layered")
    assert ctx.schedule == "flooding" and ctx.algorithm[0] == "spa"
    assert K.lib().kml_code_layers(ctx._h, None, 0) == -4
    check_golden_f64(ctx, z)
    assert ctx.bp_kernel() not in (LNMS_KERNEL, NMS_KERNEL, SPA_KERNEL)
    ctx.close()


def test_syn_is_refused(data_dir):
    hdr, z = load_case("bg2_16qam_known")
    ctx = layered_ctx(data_dir, "bg2")
    B = z["v_p0"].shape[0]
    with pytest.raises(K.KmlError, match=UNSUP):
        ctx.bp_decode(z["v_p0"], syn=np.full((B, ctx.M), -1.0))
    assert "syn" in K.lib().kml_last_error(ctx._h).decode()
    assert ctx.schedule == "layered" and ctx.algorithm[0] == "nms"
    reset(ctx)
    check_golden_f64(ctx, z)


def test_soft_metric_is_refused(data_dir):
    hdr, z = load_case("bg2_16qam_known")
    ctx = layered_ctx(data_dir, "bg2", metric_soft=True)
    s = stream(data_dir, "bg2")
    with pytest.raises(K.KmlError, match=UNSUP):
        ctx.decode_frames(s["y"][:4], s["snr"])
    assert "soft-syndrome" in K.lib().kml_last_error(ctx._h).decode()
    r = ctx.decode_frames(s["y"][:4], s["snr"], s["th"][:4])  # the known channel has no metric: it decodes
    assert ctx.bp_kernel() == LNMS_KERNEL
    m = layered_decode(data_dir, "bg2", f"stream{N}", s["p0"][:N], 50)
    assert np.array_equal(r["uu_hat"], m["uu_hat"][:4])
    reset(ctx)
    check_golden_f64(ctx, z)


def test_iteration_profile_is_refused(data_dir):
    hdr, z = load_case("bg2_16qam_known")
    s = stream(data_dir, "bg2")
    ctx = layered_ctx(data_dir, "bg2")
    ctx.sim_load(s["snr"], s["uu"][:8].astype(np.uint8), s["y"][:8], s["th"][:8])
    with pytest.raises(K.KmlError, match=UNSUP):
        ctx.sim_decode_profile(s["snr"])
    assert "min-sum" in K.lib().kml_last_error(ctx._h).decode()
    assert ctx.schedule == "layered"
    reset(ctx)
    ctx.sim_decode_profile(s["snr"])  # and it is back in SPA mode
    check_golden_f64(ctx, z)


def test_drivers_take_the_schedule(data_dir, tmp_path):
    """kmldpc_sim and python -m kmldpc_amd.simulate: --schedule / KML_SCHEDULE, stated in the line after
    the algorithm's; the same frames give the same lines in both drivers, and other lines than a
    flooding min-sum run's."""
    from test_gpu_driver import _messages
    from conftest import write_config
    cfg = tmp_path / "config.toml"
    write_config(str(cfg), data_dir, CODES["bg2"][0], CODES["bg2"][3], is5g=True, known=True, max_iter=50, snr=7.0,
                 max_blocks=256, max_err=1000000)
    env = dict(os.environ, KML_BATCH="256", KML_SEED="4", PYTHONPATH=REPO)
    env.pop("KML_ALGORITHM", None)
    env.pop("KML_SCHEDULE", None)
    exe = os.path.join(REPO, "kmldpc_amd", "bin", "kmldpc_sim")
    py = [sys.executable, "-m", "kmldpc_amd.simulate"]
    run = lambda cmd, e=env: subprocess.run(cmd, cwd=tmp_path, env=e, capture_output=True, text=True, timeout=120)
    r1 = run([exe, "--algorithm", "nms", "--schedule", "layered", str(cfg)])
    r2 = run(py + [str(cfg)], dict(env, KML_ALGORITHM="nms", KML_SCHEDULE="layered"))
    flood = run([exe, "--algorithm", "nms", "--schedule=flooding", str(cfg)])
    for r in (r1, r2, flood):
        assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-1000:]
    m1, m2, mf = (_messages(r.stdout) for r in (r1, r2, flood))
    assert m1[0].startswith("BP decode algorithm: nms") and m1[1] == "BP decode schedule: layered"
    assert m1[2] == "Start simulation"
    assert m1[:-1] == m2[:-1]
    assert mf[1] == "Start simulation"
    res = lambda m: [x for x in m if x.startswith("SNR = ")]
    assert res(m1) and res(m1) != res(mf)  # another schedule on the same frames
    bad = run([exe, "--schedule", "layered", str(cfg)])  # without nms
    assert bad.returncode == 255 and "--schedule" in bad.stdout
    assert run([exe, "--algorithm", "nms", "--schedule", "zigzag", str(cfg)]).returncode == 255
    assert run(py + ["--schedule", "layered", str(cfg)]).returncode == 2  # argparse's usage error
    assert run(py + [str(cfg)], dict(env, KML_SCHEDULE="layered")).returncode == 2


def test_generic_kernel_refuses_layered(data_dir):
    """KML_BP_KERNEL is read once per process: a child started with KML_BP_KERNEL=generic."""
    env = dict(os.environ, PYTHONPATH=REPO, KML_BP_KERNEL="generic")
    p = subprocess.run([sys.executable, os.path.join(TESTS, "lnms_generic_child.py"), data_dir], env=env,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "refused" in p.stdout
