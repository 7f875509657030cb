"""GPU tests of the layered min-sum decoders on codes past bp_irregular_kernel's
round plan (the lifted BG2 codes of tests/golden/make_codes_lifted.py) and of
the kernels' global-table instances.  Every comparison is equality of bit
patterns against the numpy models (tests/bp_oms_model.py, which equals
bp_lnms_model / bp_h16_model / bp_llr_model at offset 0); no tolerance anywhere.

How a test knows which instance ran: kml_bp_kernel names the global-table
instances "bp_irregular_lnms_gt_kernel" / "bp_irregular_lnms_h16_gt_kernel" and
the LDS-table instances as before.

The stream, the codes and the checks shared with the child process are in
tests/lifted_codes.py.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import lifted_codes as LC
from bp_oms_model import oms_blind_metric
from conftest import REPO, TESTS

import kmldpc_amd as K

pytestmark = pytest.mark.gpu

UNSUP = r"\(code -4\)"
LDS, GLOBAL = LC.FAMILIES[False], LC.FAMILIES[True]
_ctx = {}


@pytest.fixture(scope="module")
def big_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("lifted")


def ctx_for(data_dir, Z, tmp_dir=None, **kw):
    """One context per code (and option set); every test leaves it in SPA mode."""
    key = (Z,) + tuple(sorted(kw.items()))
    if key not in _ctx:
        _ctx[key] = K.Context(device=0, **LC.ctx_args(data_dir, Z, tmp_dir, **kw))
    return _ctx[key]


def last_error(ctx):
    return K.lib().kml_last_error(ctx._h).decode()


# ---- Z = 128: a layered-only code whose tables fit in LDS -------------------

@pytest.mark.parametrize("beta", [0.0, 0.5])
@pytest.mark.parametrize("alpha", [0.75, 1.0])
@pytest.mark.parametrize("messages", ["f32", "f16"])
def test_z128_llr_decode_equals_model(data_dir, messages, alpha, beta):
    """Budgets 25, 5, 1 and 0, with and without llr_out; 24 passes: the LDS-table instances, two workgroups a CU."""
    _, g = LC.graph(data_dir, 128)
    LC.check_llr_decodes(ctx_for(data_dir, 128), g, LDS, messages, alpha, beta)


@pytest.mark.parametrize("messages", ["f32", "f16"])
def test_z128_batches_and_p0(data_dir, messages):
    _, g = LC.graph(data_dir, 128)
    ctx = ctx_for(data_dir, 128)
    LC.check_batches(ctx, g, LDS, messages)
    LC.check_p0_decode(ctx, g, LDS, messages)


def child(data_dir, what, **env):
    p = subprocess.run([sys.executable, os.path.join(TESTS, "lifted_global_child.py"), data_dir, what],
                       env=dict(os.environ, PYTHONPATH=REPO + os.pathsep + TESTS, **env), capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    return p.stdout


def test_global_table_instances_on_codes_that_fit(data_dir):
    """KML_LNMS_TABLES is read once per process: a child runs the Z = 128 shapes above, BG2 K960 (the register
    path) and syn_qc_l200 (multi-pass layers) on the global-table instances."""
    assert "equal the models" in child(data_dir, "tables", KML_LNMS_TABLES="global")


# ---- Z = 288 and 384: the tables do not fit ---------------------------------

@pytest.mark.parametrize("messages", ["f32", "f16"])
@pytest.mark.parametrize("Z", [288, 384])
def test_large_codes_take_the_global_table_instances(data_dir, big_dir, Z, messages):
    """No variable set: the LDS-table footprint (171,810 B at Z = 288) is past one CU, the launch takes the
    global-table instance, one workgroup a CU; 36 and 48 passes.  B = 5: an unpaired half in binary16."""
    _, g = LC.graph(data_dir, Z, big_dir)
    assert 4 * g.N + 4 * g.E + 2 * g.E + 2 * (g.M + 1) + g.N > 160 * 1024 > 4 * g.N + 4 * g.E + g.N + 48 * 4 + 32
    ctx = ctx_for(data_dir, Z, big_dir)
    assert ctx.layers().tolist() == list(range(0, 12 * Z + 1, Z))
    LC.check_llr_decodes(ctx, g, GLOBAL, messages, 0.75, 0.0, budgets=(25, 1), B=5)


def test_a_code_past_one_cu_is_still_refused(data_dir, big_dir):
    ctx = ctx_for(data_dir, 416, big_dir)
    with pytest.raises(K.KmlError, match=UNSUP):
        ctx.set_algorithm("nms")
    assert "the context keeps its algorithm" in last_error(ctx) and ctx.algorithm[0] == "spa"
    assert K.lib().kml_code_layers(ctx._h, None, 0) == -4


# ---- the schedule rule ------------------------------------------------------

def test_schedule_rule(data_dir):
    """In the min-sum mode under the flooding schedule every decode entry answers KML_E_UNSUP, names the schedule
    setter and launches nothing; after set_schedule("layered") they decode; set_algorithm("spa") goes back to the
    generic fp64 kernel."""
    _, g = LC.graph(data_dir, 128)
    ctx = ctx_for(data_dir, 128)
    ctx.set_algorithm("spa")
    B = 4
    easy = LC.p0_stream(g.cc_len, B, snr=3.0)
    r = ctx.bp_decode(easy, 5)
    assert ctx.bp_kernel() == "bp_kernel" and not r["uu_hat"].any()
    ctx.set_algorithm("nms")  # accepted; the schedule starts as flooding
    assert ctx.algorithm == ("nms", 0.75) and ctx.schedule == "flooding"
    ctx.sim_generate(7.0, B, seed=3)
    uu, y, h = ctx.sim_frames(B)
    llr = np.ascontiguousarray(LC.llr_stream(g.cc_len, B))
    p0 = np.ascontiguousarray(LC.p0_stream(g.cc_len, B))
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    L = K.lib()

    def refused(call, *names):
        before = ctx.bp_kernel()
        with pytest.raises(K.KmlError, match=UNSUP):
            call()
        msg = last_error(ctx)
        assert "kml_set_schedule(KML_SCHED_LAYERED)" in msg and any(n in msg for n in names), msg
        assert ctx.bp_kernel() == before  # nothing was launched
        assert ctx.algorithm == ("nms", 0.75) and ctx.schedule == "flooding"  # the context keeps its state

    for entry, first in (("kml_llr_decode", llr), ("kml_bp_decode", p0)):
        uh, cch = np.full((B, ctx.K), 7, np.uint8), np.full((B, ctx.Ncol), 9, np.uint8)
        ret, post = np.full(B, -5, np.int32), np.full((B, ctx.Ncol), -3.5, np.float32)
        last = ptr(post) if entry == "kml_llr_decode" else None
        assert getattr(L, entry)(ctx._h, ptr(first), B, 25, ptr(uh), ptr(ret), ptr(cch), last, 0) == -4
        assert entry in last_error(ctx) and "kml_set_schedule(KML_SCHED_LAYERED)" in last_error(ctx)
        assert np.all(uh == 7) and np.all(cch == 9) and np.all(ret == -5) and np.all(post == np.float32(-3.5))
        assert ctx.bp_kernel() == "bp_kernel"
    refused(lambda: ctx.llr_decode(llr, 25, llr_out=True), "kml_llr_decode")
    refused(lambda: ctx.bp_decode(p0, 25), "kml_bp_decode")
    refused(lambda: ctx.decode_frames(y, 7.0, h), "kml_decode_frames")
    refused(lambda: ctx.decode_frames(y, 7.0), "kml_decode_frames")
    refused(lambda: ctx.decode_candidates(y, np.tile(h[:, None, :], (1, 2, 1)), 7.0), "kml_decode_candidates")
    refused(lambda: ctx.decode_candidates(y, h[:, None, :], 7.0), "kml_decode_frames")  # one candidate: that path
    refused(lambda: ctx.sim_decode(7.0), "kml_sim_decode")
    refused(lambda: ctx.sim_decode(7.0, sync=False), "kml_sim_decode")
    refused(lambda: ctx.sim_decode_ex(7.0), "kml_sim_decode_ex")
    refused(lambda: ctx.sim_decode_ex(7.0, blind=True), "kml_sim_decode_ex")
    refused(lambda: ctx.sim_point(7.0, 1, batch=8, max_blocks=8, max_err=100), "kml_sim_point")
    with pytest.raises(K.KmlError, match=UNSUP):  # no binary16 format without the layered schedule, as everywhere
        ctx.set_messages("f16")
    ctx.set_demapper("maxlog")  # the front end and the offset belong to the mode, not to the schedule
    ctx.set_offset(0.5)
    refused(lambda: ctx.decode_frames(y, 7.0, h), "kml_decode_frames")
    ctx.set_demapper("exact")
    ctx.set_offset(0)
    # ... and then they decode
    ctx.set_schedule("layered")
    m = LC.llr_model(g, llr, 25, LC.MAX_ITER, 0.75, 0.0, "f32")
    LC.same(ctx.llr_decode(llr, 25, cc_hat=True, llr_out=True), m, "after set_schedule")
    assert ctx.bp_kernel() == LDS["f32"]
    LC.same(ctx.bp_decode(p0, 25, cc_hat=True), LC.p0_model(g, p0, 25, LC.MAX_ITER, 0.75, 0.0, "f32"), "P0")
    for out in (ctx.decode_frames(y, 7.0, h), ctx.decode_candidates(y, np.tile(h[:, None, :], (1, 2, 1)), 7.0)):
        assert out["ret"].min() >= 1 and ctx.bp_kernel() == LDS["f32"]
    c = ctx.sim_decode(7.0)
    assert c["tot_blk"] == B and ctx.sim_decode_ex(7.0)[2]["tot_blk"] == B
    assert ctx.sim_point(7.0, 1, batch=8, max_blocks=8, max_err=100)["tot_blk"] == 8
    ctx.set_schedule("flooding")  # back under the rule
    refused(lambda: ctx.llr_decode(llr, 25), "kml_llr_decode")
    ctx.set_algorithm("spa")
    r = ctx.bp_decode(easy, 5)
    assert ctx.bp_kernel() == "bp_kernel" and not r["uu_hat"].any()


# ---- the receive path -------------------------------------------------------

def test_receive_path_known_channel_maxlog(data_dir):
    """Z = 128 + 16QAM: sim_decode's counters are those of llr_decode(demap_llr(frames)), and that decode is
    the model's."""
    _, g = LC.graph(data_dir, 128)
    ctx = ctx_for(data_dir, 128)
    B, snr = 64, 7.0
    for messages in ("f32", "f16"):
        LC.layered_mode(ctx, 0.75, 0.0, messages)
        ctx.set_demapper("maxlog")
        ctx.sim_generate(snr, B, seed=11)
        uu, y, h = ctx.sim_frames(B)
        err, _, cnt = ctx.sim_decode_ex(snr)
        assert ctx.bp_kernel() == LDS[messages]
        llr = ctx.demap_llr(y, h, 10.0 ** (-0.1 * snr))
        r = ctx.llr_decode(llr, LC.MAX_ITER, cc_hat=True, llr_out=True)
        want = (r["uu_hat"] != uu).sum(axis=1).astype(np.int32)
        print(f"{messages}: {int((want > 0).sum())} of {B} blocks in error")
        assert np.array_equal(err, want)
        assert (cnt["err_bit"], cnt["err_blk"], cnt["tot_blk"]) == (int(want.sum()), int((want > 0).sum()), B)
        assert cnt == ctx.sim_decode(snr)
        out = ctx.decode_frames(y, snr, h)
        assert np.array_equal(out["uu_hat"], r["uu_hat"]) and np.array_equal(out["ret"], r["ret"])
        if messages == "f32":
            LC.same(r, LC.llr_model(g, llr, LC.MAX_ITER, LC.MAX_ITER, 0.75, 0.0, messages), "receive path")
        ctx.set_algorithm("spa")


def test_receive_path_blind(data_dir):
    """Blind, max-log (B = 8): the four candidates' metric decodes run the layered decoder, chosen and metrics are
    the model's.  Blind, exact demapper (B = 4): the metric decodes stay fp64 sum-product, here on the generic
    bp_kernel: chosen and metrics are the SPA context's, the final decode is the layered model's."""
    _, g = LC.graph(data_dir, 128)
    ctx = ctx_for(data_dir, 128)
    snr = 9.0
    var = 10.0 ** (-0.1 * snr)
    ctx.set_algorithm("spa")
    ctx.sim_generate(snr, 8, seed=5)
    uu, y, h = ctx.sim_frames(8)
    _, h4 = ctx.kmeans(y)
    spa = ctx.decode_frames(y[:4], snr)
    assert ctx.bp_kernel() == "bp_kernel"
    LC.layered_mode(ctx, 0.75, 0.0, "f32")
    ctx.set_demapper("maxlog")
    out = ctx.decode_frames(y, snr)
    assert ctx.bp_kernel() == LDS["f32"]
    met, chosen, llrs = oms_blind_metric(g, ctx.constellation(), ctx.bits, y, h4, var, 5, LC.MAX_ITER, 0.75, 0.0,
                                         "layered", "f32")
    assert np.array_equal(out["chosen"], chosen) and np.array_equal(out["metrics"], met)
    m = LC.llr_model(g, llrs[np.arange(8), chosen], LC.MAX_ITER, LC.MAX_ITER, 0.75, 0.0, "f32")
    assert np.array_equal(out["uu_hat"], m["uu_hat"]) and np.array_equal(out["ret"], m["ret"])
    ctx.set_demapper("exact")
    out = ctx.decode_frames(y[:4], snr)
    assert ctx.bp_kernel() == LDS["f32"]
    for key in ("chosen", "metrics", "h_hat"):
        assert np.array_equal(out[key], spa[key]), key
    p0 = ctx.demap(y[:4], h4[np.arange(4), out["chosen"]], var)
    m = LC.p0_model(g, p0, LC.MAX_ITER, LC.MAX_ITER, 0.75, 0.0, "f32")
    assert np.array_equal(out["uu_hat"], m["uu_hat"]) and np.array_equal(out["ret"], m["ret"])
    ctx.set_algorithm("spa")


# ---- the refusals that stay -------------------------------------------------

def test_min_sum_refusals_hold(data_dir):
    """syn, the iteration profile and the soft-syndrome metric, in the layered schedule."""
    _, g = LC.graph(data_dir, 128)
    ctx = ctx_for(data_dir, 128)
    LC.layered_mode(ctx, 0.75, 0.0, "f32")
    p0 = LC.p0_stream(g.cc_len, 2)
    with pytest.raises(K.KmlError, match=UNSUP):
        ctx.bp_decode(p0, syn=np.full((2, ctx.M), -1.0))
    assert "syn" in last_error(ctx)
    ctx.sim_generate(7.0, 4, seed=3)
    with pytest.raises(K.KmlError, match=UNSUP):
        ctx.sim_decode_profile(7.0)
    assert "profile" in last_error(ctx)
    assert ctx.algorithm[0] == "nms" and ctx.schedule == "layered"
    ctx.set_algorithm("spa")
    soft = ctx_for(data_dir, 128, metric_soft=True)
    LC.layered_mode(soft, 0.75, 0.0, "f32")
    uu, y, h = ctx.sim_frames(4)
    with pytest.raises(K.KmlError, match=UNSUP):
        soft.decode_frames(y, 7.0)
    assert "soft-syndrome" in last_error(soft)
    soft.set_algorithm("spa")


def test_generic_kernel_refuses_the_min_sum_mode(data_dir):
    assert "refused" in child(data_dir, "generic", KML_BP_KERNEL="generic")
