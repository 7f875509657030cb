"""GPU tests of the opt-in normalized min-sum mode (kml_set_algorithm, KML_ALG_NMS;
kmldpc_amd/csrc/bp_irregular_nms.hip).  The mode is a different decoder from the
reference's, so it is held to its own contract instead: the kernel equals the
numpy model (tests/bp_nms_model.py) bit for bit on uu_hat, ret and cc_hat, its
results do not depend on the batch, and nothing of it leaks into the fp64 paths.

The codes are 5G BG2 K960 with 16QAM and syn_irr1200 with 64QAM (every degree
instance of the kernel, idle and partial waves, the non-5G epilogue, K = 600 off
the 64-bit grid).  Streams, special inputs and the model's decodes come from
test_bp_nms_model.py, made once per session.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from bp_nms_model import nms_model
from conftest import REPO, TESTS, load_case
from oracle import oracle as O
from test_bp_nms_model import CODES, code, model_decode, random_p0, saturated_p0, stream
from test_gpu_device_ptrs import DeviceBufs, filled

import kmldpc_amd as K

pytestmark = pytest.mark.gpu

NMS_KERNEL = "bp_irregular_nms_kernel"
SPA_KERNEL = "bp_irregular_kernel"
N = 64  # stream codewords per comparison

_ctx = {}


def ctx_for(data_dir, name, **kw):
    """One context per code (and option set); the tests set the algorithm they need."""
    key = (name,) + tuple(sorted(kw.items()))
    if key not in _ctx:
        matrix, is5g, max_iter, modem, _ = CODES[name]
        _ctx[key] = K.Context(matrix_file=os.path.join(data_dir, matrix), modem_file=os.path.join(data_dir, modem),
                              is5g=is5g, max_iter=max_iter, device=0, **kw)
    return _ctx[key]


def nms_ctx(data_dir, name, alpha=None):
    ctx = ctx_for(data_dir, name)
    ctx.set_algorithm("nms", alpha)
    assert ctx.algorithm == ("nms", float(np.float32(0.75 if alpha is None else alpha)))
    return ctx


def assert_equals_model(r, m, what):
    for key in ("ret", "uu_hat", "cc_hat"):
        bad = np.nonzero((np.asarray(r[key]) != m[key]).reshape(len(m[key]), -1).any(axis=1))[0]
        assert bad.size == 0, f"{what}: {key} differs from the model on codewords {bad[:8]} ({bad.size} in all)"


def check_golden_f64(ctx, z):
    p0 = z["v_p0"]
    B = p0.shape[0]
    r = ctx.bp_decode(p0, cc_hat=True, syn=np.full((B, ctx.M), -1.0))
    assert np.array_equal(r["ret"], z["s_ret"][:B])
    assert np.array_equal(r["uu_hat"], z["v_uu_hat"])
    assert np.array_equal(r["cc_hat"], z["v_cc_hat"])
    for i in range(B):
        if r["ret"][i] > 1:
            assert np.array_equal(r["syn"][i], z["v_syn"][i]), f"syndrom_soft cw {i}"


# ---- kernel = model --------------------------------------------------------

@pytest.mark.parametrize("name,budget", [("bg2", 50), ("bg2", 5), ("bg2", 1), ("syn_irr1200", 20)])
def test_kernel_equals_model(data_dir, name, budget):
    ctx = nms_ctx(data_dir, name)
    p0 = stream(data_dir, name)["p0"][:N]
    m = model_decode(data_dir, name, f"stream{N}", p0, budget)
    r = ctx.bp_decode(p0, budget, cc_hat=True)
    assert ctx.bp_kernel() == NMS_KERNEL
    assert_equals_model(r, m, f"{name} budget {budget}")
    max_iter = CODES[name][2]
    if budget == max_iter:  # both outcomes are in the comparison
        assert np.any(m["ret"] == max_iter) and np.any(m["ret"] < max_iter)
    ctx.set_algorithm("spa")


def test_zero_iterations_leave_the_outputs(data_dir):
    ctx = nms_ctx(data_dir, "bg2")
    B = 5
    p0 = np.ascontiguousarray(stream(data_dir, "bg2")["p0"][:B])
    uh = np.full((B, ctx.K), 7, np.uint8)
    cch = np.full((B, ctx.Ncol), 9, np.uint8)
    ret = np.full(B, -5, np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert K.lib().kml_bp_decode(ctx._h, ptr(p0), B, 0, ptr(uh), ptr(ret), ptr(cch), None, 0) == 0
    assert ctx.bp_kernel() == NMS_KERNEL
    assert np.all(uh == 7) and np.all(cch == 9)
    assert np.all(ret == 1)  # iter = 0 < max_iter
    ctx.set_algorithm("spa")


@pytest.mark.parametrize("alpha", [1.0, 0.8125])
def test_alpha(data_dir, alpha):
    ctx = nms_ctx(data_dir, "bg2", alpha)
    p0 = stream(data_dir, "bg2")["p0"][:N]
    m = model_decode(data_dir, "bg2", f"stream{N}", p0, 50, alpha)
    base = model_decode(data_dir, "bg2", f"stream{N}", p0, 50)
    assert (m["cc_hat"] != base["cc_hat"]).any()  # the factor matters on these codewords
    r = ctx.bp_decode(p0, 50, cc_hat=True)
    assert ctx.bp_kernel() == NMS_KERNEL
    assert_equals_model(r, m, f"alpha {alpha}")
    ctx.set_algorithm("spa")


@pytest.mark.parametrize("which", ["saturated", "random"])
def test_saturated_and_random_priors(data_dir, which):
    """P0 of exactly 0, 1, 0.5 and 1e-300, the all-0.5 codeword (messages in the +-256 clamp, zero
    magnitudes, ties), and uniform-random P0 that never converges."""
    ctx = nms_ctx(data_dir, "bg2")
    p0 = saturated_p0(data_dir) if which == "saturated" else random_p0(data_dir)
    m = model_decode(data_dir, "bg2", which, p0, 50)
    if which == "saturated":
        assert m["stats"]["max_abs_v2c"] == 256.0
    else:
        assert np.all(m["ret"] == 50)
    r = ctx.bp_decode(p0, 50, cc_hat=True)
    assert ctx.bp_kernel() == NMS_KERNEL
    assert_equals_model(r, m, which)
    ctx.set_algorithm("spa")


def test_batch_and_queue_independence(data_dir):
    """B = 700 exceeds the resident workgroups (one per CU), so workgroups re-enter the dequeue loop."""
    ctx = nms_ctx(data_dir, "bg2")
    p0 = stream(data_dir, "bg2")["p0"]
    n = p0.shape[0]
    big = np.concatenate([p0] * (700 // n + 1))[:700]
    runs = {}
    for tag, B in [("1", 1), ("3", 3), ("700", 700), ("1 again", 1), ("3 again", 3), ("700 again", 700)]:
        runs[tag] = ctx.bp_decode(big[:B], 50, cc_hat=True)
        assert ctx.bp_kernel() == NMS_KERNEL
    for key in ("uu_hat", "ret", "cc_hat"):
        for tag in ("1", "3", "700"):  # each batch decoded twice
            assert np.array_equal(runs[tag][key], runs[tag + " again"][key]), (tag, key)
        assert np.array_equal(runs["1"][key], runs["700"][key][:1]), key
        assert np.array_equal(runs["3"][key], runs["700"][key][:3]), key
        # the later copies of the stream sit at other queue positions
        assert np.array_equal(runs["700"][key][n:700], runs["700"][key][:700 - n]), key
    m = model_decode(data_dir, "bg2", f"stream{N}", p0[:N], 50)
    assert_equals_model({k: v[:N] for k, v in runs["700"].items()}, m, "B = 700")
    ctx.set_algorithm("spa")


# ---- nothing leaks into the fp64 paths -------------------------------------

def test_no_leakage_between_algorithms(data_dir):
    hdr, z = load_case("bg2_16qam_known")
    assert (hdr["matrix"], hdr["modem"], hdr["max_iter"]) == (CODES["bg2"][0], CODES["bg2"][3], CODES["bg2"][2])
    ctx = ctx_for(data_dir, "bg2")
    ctx.set_algorithm("spa")
    check_golden_f64(ctx, z)
    assert ctx.bp_kernel() == SPA_KERNEL
    ctx.set_algorithm("nms")
    r = ctx.bp_decode(z["v_p0"], cc_hat=True)
    assert ctx.bp_kernel() == NMS_KERNEL
    _, g = code(data_dir, "bg2")
    ret, uh, cch = nms_model(g, z["v_p0"], 50, 50)
    assert_equals_model(r, dict(ret=ret, uu_hat=uh, cc_hat=cch), "golden P0")
    ctx.set_algorithm("spa")
    assert ctx.algorithm[0] == "spa"
    check_golden_f64(ctx, z)
    assert ctx.bp_kernel() == SPA_KERNEL


def test_blind_path_front_end_untouched(data_dir):
    """k-means, the demapper and BG2's metric_iter decodes stay fp64 sum-product: chosen, metrics and
    h_hat are those of SPA mode, and uu_hat is the model's decode of demap(y, h_chosen)."""
    n = 32
    s = stream(data_dir, "bg2")
    y, snr = s["y"][:n], s["snr"]
    ctx = ctx_for(data_dir, "bg2")
    ctx.set_algorithm("spa")
    ref = ctx.decode_frames(y, snr)
    assert ctx.bp_kernel() == SPA_KERNEL
    _, h4 = ctx.kmeans(y)
    ctx.set_algorithm("nms")
    out = ctx.decode_frames(y, snr)
    assert ctx.bp_kernel() == NMS_KERNEL
    for key in ("chosen", "metrics", "h_hat"):
        assert np.array_equal(out[key], ref[key]), key
    assert len(set(out["chosen"].tolist())) > 1  # more than one rotation is chosen
    p0 = ctx.demap(y, h4[np.arange(n), out["chosen"]], 10.0 ** (-0.1 * snr))
    _, g = code(data_dir, "bg2")
    ret, uh, _ = nms_model(g, p0, 50, 50)
    assert np.array_equal(out["uu_hat"], uh)
    assert np.array_equal(out["ret"], ret)
    ctx.set_algorithm("spa")


def test_simulator_path(data_dir):
    n = 256
    s = stream(data_dir, "bg2", n)
    _, g = code(data_dir, "bg2")
    m = model_decode(data_dir, "bg2", f"stream{n}", s["p0"], 50)
    uu = s["uu"].astype(np.uint8)
    want = (m["uu_hat"] != uu).sum(axis=1).astype(np.int32)
    ctx = nms_ctx(data_dir, "bg2")
    ctx.sim_load(s["snr"], uu, s["y"], s["th"])
    err, _, cnt = ctx.sim_decode_ex(s["snr"])
    assert ctx.bp_kernel() == NMS_KERNEL
    assert np.array_equal(err, want)
    assert (cnt["err_bit"], cnt["err_blk"]) == (int(want.sum()), int(np.sum(want > 0)))
    assert (cnt["tot_bit"], cnt["tot_blk"]) == (n * g.K, n)
    assert cnt["redone"] == 0
    assert 0 < cnt["err_blk"] < n
    c = ctx.sim_decode(s["snr"])  # the plain entry point counts the same
    assert (c["err_bit"], c["err_blk"], c["tot_blk"], c["redone"]) == (cnt["err_bit"], cnt["err_blk"], n, 0)
    ctx.set_algorithm("spa")


def test_device_pointers(data_dir):
    ctx = nms_ctx(data_dir, "bg2")
    B = 3
    p0 = np.ascontiguousarray(stream(data_dir, "bg2")["p0"][:B])
    host = ctx.bp_decode(p0, 50, cc_hat=True)
    uh, ret, cch = filled((B, ctx.K), np.uint8), filled(B, np.int32), filled((B, ctx.Ncol), np.uint8)
    with DeviceBufs() as d:
        d_p0, d_uh, d_ret, d_cch = d.put(p0), d.put(uh), d.put(ret), d.put(cch)
        assert K.lib().kml_bp_decode(ctx._h, d_p0, B, 50, d_uh, d_ret, d_cch, None, K.KML_DEVICE_PTRS) == 0
        assert ctx.bp_kernel() == NMS_KERNEL
        assert np.array_equal(d.get(d_uh, uh), host["uu_hat"])
        assert np.array_equal(d.get(d_ret, ret), host["ret"])
        assert np.array_equal(d.get(d_cch, cch), host["cc_hat"])
    ctx.set_algorithm("spa")


# ---- refusals: KML_E_UNSUP, the algorithm kept, the fp64 decode intact -------

UNSUP = r"\(code -4\)"


@pytest.mark.parametrize("case", ["peg2304_qpsk_known", "peg8064_qpsk_known", "syn_reg36_192_qpsk_blind"])
def test_other_codes_refuse_nms(data_dir, case):
    hdr, z = load_case(case)
    ctx = K.Context(matrix_file=os.path.join(data_dir, hdr["matrix"]), modem_file=os.path.join(data_dir, hdr["modem"]),
                    is5g=bool(hdr["is5g"]), max_iter=hdr["max_iter"], device=0)
    with pytest.raises(K.KmlError, match=UNSUP):
        ctx.set_algorithm("nms")
    assert ctx.algorithm[0] == "spa"
    check_golden_f64(ctx, z)
    assert ctx.bp_kernel() not in (NMS_KERNEL, SPA_KERNEL)
    ctx.close()


def test_syn_is_refused(data_dir):
    hdr, z = load_case("bg2_16qam_known")
    ctx = nms_ctx(data_dir, "bg2")
    B = z["v_p0"].shape[0]
    with pytest.raises(K.KmlError, match=UNSUP):
        ctx.bp_decode(z["v_p0"], syn=np.full((B, ctx.M), -1.0))
    assert "syn" in K.lib().kml_last_error(ctx._h).decode()
    assert ctx.algorithm[0] == "nms"
    ctx.set_algorithm("spa")
    check_golden_f64(ctx, z)


def test_soft_metric_is_refused(data_dir):
    hdr, z = load_case("bg2_16qam_known")
    ctx = ctx_for(data_dir, "bg2", metric_soft=True)
    ctx.set_algorithm("nms")
    s = stream(data_dir, "bg2")
    with pytest.raises(K.KmlError, match=UNSUP):
        ctx.decode_frames(s["y"][:4], s["snr"])
    assert "soft-syndrome" in K.lib().kml_last_error(ctx._h).decode()
    r = ctx.decode_frames(s["y"][:4], s["snr"], s["th"][:4])  # the known channel has no metric: it decodes
    assert ctx.bp_kernel() == NMS_KERNEL
    m = model_decode(data_dir, "bg2", f"stream{N}", s["p0"][:N], 50)
    assert np.array_equal(r["uu_hat"], m["uu_hat"][:4])
    ctx.set_algorithm("spa")
    check_golden_f64(ctx, z)


def test_iteration_profile_is_refused(data_dir):
    hdr, z = load_case("bg2_16qam_known")
    s = stream(data_dir, "bg2")
    ctx = nms_ctx(data_dir, "bg2")
    ctx.sim_load(s["snr"], s["uu"][:8].astype(np.uint8), s["y"][:8], s["th"][:8])
    with pytest.raises(K.KmlError, match=UNSUP):
        ctx.sim_decode_profile(s["snr"])
    assert "min-sum" in K.lib().kml_last_error(ctx._h).decode()
    ctx.set_algorithm("spa")
    ctx.sim_decode_profile(s["snr"])  # and it is back in SPA mode
    check_golden_f64(ctx, z)


def test_f32_and_nms_exclude_each_other(data_dir):
    hdr, z = load_case("peg2304_qpsk_known")
    peg = K.Context(matrix_file=os.path.join(data_dir, hdr["matrix"]), modem_file=os.path.join(data_dir, hdr["modem"]),
                    max_iter=hdr["max_iter"], device=0)
    peg.set_precision("f32")
    with pytest.raises(K.KmlError, match=UNSUP):
        peg.set_algorithm("nms")
    assert "f32" in K.lib().kml_last_error(peg._h).decode()
    assert peg.algorithm[0] == "spa" and peg.precision == "f32"
    peg.set_precision("f64")
    check_golden_f64(peg, z)
    peg.close()
    hdr, z = load_case("bg2_16qam_known")
    ctx = nms_ctx(data_dir, "bg2")
    with pytest.raises(K.KmlError, match=UNSUP):
        ctx.set_precision("f32")
    assert ctx.algorithm[0] == "nms" and ctx.precision == "f64"
    ctx.set_algorithm("spa")
    check_golden_f64(ctx, z)


def test_drivers_take_the_algorithm(data_dir, tmp_path):
    """kmldpc_sim and python -m kmldpc_amd.simulate: --algorithm / KML_ALGORITHM, stated in the first
    line; the same frames give the same lines in both drivers, and other lines than a SPA run's."""
    from test_gpu_driver import _messages
    from conftest import write_config
    cfg = tmp_path / "config.toml"
    write_config(str(cfg), data_dir, CODES["bg2"][0], CODES["bg2"][3], is5g=True, known=True, max_iter=50, snr=7.0,
                 max_blocks=256, max_err=1000000)
    env = dict(os.environ, KML_BATCH="256", KML_SEED="4", PYTHONPATH=REPO)
    env.pop("KML_ALGORITHM", None)
    exe = os.path.join(REPO, "kmldpc_amd", "bin", "kmldpc_sim")
    py = [sys.executable, "-m", "kmldpc_amd.simulate"]
    run = lambda cmd, e=env: subprocess.run(cmd, cwd=tmp_path, env=e, capture_output=True, text=True, timeout=120)
    r1 = run([exe, "--algorithm", "nms:0.8125", str(cfg)])
    r2 = run(py + [str(cfg)], dict(env, KML_ALGORITHM="nms:0.8125"))
    spa = run([exe, str(cfg)])
    for r in (r1, r2, spa):
        assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-1000:]
    m1, m2, ms = (_messages(r.stdout) for r in (r1, r2, spa))
    assert m1[0].startswith("BP decode algorithm: nms (normalized min-sum, alpha = 0.8125") and m1[1] == "Start simulation"
    assert m1[:-1] == m2[:-1]
    assert ms[0] == "Start simulation"
    res = lambda m: [x for x in m if x.startswith("SNR = ")]
    assert res(m1) and res(m1) != res(ms)  # a different decoder on the same frames
    bad = run([exe, "--algorithm", "nms:1.5", str(cfg)])
    assert bad.returncode == 255 and "--algorithm" in bad.stdout
    assert run(py + ["--algorithm", "oms", str(cfg)]).returncode == 2  # argparse's usage error


def test_generic_kernel_refuses_nms(data_dir):
    """KML_BP_KERNEL is read once per process: a child started with KML_BP_KERNEL=generic."""
    env = dict(os.environ, PYTHONPATH=REPO, KML_BP_KERNEL="generic")
    p = subprocess.run([sys.executable, os.path.join(TESTS, "nms_generic_child.py"), data_dir], env=env,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "refused" in p.stdout
