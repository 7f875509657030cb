"""GPU tests of the opt-in single-precision BP mode (kml_set_precision, KML_PREC_F32;
kmldpc_amd/csrc/bp_regular_f32.hip).  The mode is not bit-exact with the
reference: what it promises is agreement within a cap, independence of the
batch, determinism, and that nothing of it leaks into the fp64 paths.

The code is PEG2304 (the kernel's only shape is its class: (3,6)-regular,
2304 x 1152), and in one row or run of the decision, batch and demap tests the
rank-1147 code of that class (K = 1157, 19 words of decoded bits, chk = 1147:
tests/golden/make_codes.py).  The streams, the oracle's decodes of them and
the float32 model come from test_bp_f32_model.py.
"""
import os

import numpy as np
import pytest

from conftest import load_case
from oracle import oracle as O
from test_bp_f32_model import (CAP, MATRIX, R1147, STREAM_MATRIX, STREAMS, SYN_FILL, assert_both_outcomes, differing,
                               oracle_decode, stream)

import kmldpc_amd as K

pytestmark = pytest.mark.gpu

F32_KERNEL = "bp_regular_f32_kernel"
F64_KERNEL = "bp_regular_kernel"
N = 384  # codewords per stream
N_R1147 = 96  # of the rank-1147 code's stream

_ctx = {}


def ctx_for(data_dir, modem, matrix=MATRIX, is5g=False, max_iter=20):
    """One context per (code, modem); the tests set the precision they need."""
    key = (matrix, modem, is5g, max_iter)
    if key not in _ctx:
        _ctx[key] = K.Context(matrix_file=os.path.join(data_dir, matrix), modem_file=os.path.join(data_dir, modem),
                              is5g=is5g, max_iter=max_iter, device=0)
    return _ctx[key]


def f32_ctx(data_dir, name="qpsk"):
    ctx = ctx_for(data_dir, STREAMS[name][0], STREAM_MATRIX.get(name, MATRIX))
    ctx.set_precision("f32")
    assert ctx.precision == "f32"
    return ctx


# max |syn - oracle syn| over the codewords whose ret agrees: 4 x the float32
# ("ieee") model's own distance from the oracle on the same 384 codewords
# (test_bp_f32_model.model_syn_delta; the margin is for the kernel's different
# rounding: reciprocal-multiply instead of division).  The model's values:
#   qpsk  budget 1: 1.281e-07   budget 5: 1.423e-04   budget 20: 5.409e-04
#   16qam budget 20: 1.014e-03  64qam budget 20: 9.540e-04
# (the reciprocal-multiply model with +-1 ulp reciprocals stays inside the
# bounds too: 2.3e-07, 4.6e-04, 1.26e-03, 2.62e-03, 1.03e-03)
# On the rank-1147 code's stream (96 codewords, QPSK at 4 dB) the budget-20
# bound does not carry over: over 192 codewords the model itself sits 0.30 from
# the oracle on one codeword whose ret agrees (a decode that diverges late),
# against 1.2e-04 over the first 96, so the distance there measures the stream,
# not the arithmetic.  Its syndromes are held at budget 1 (one CN phase, nothing
# to diverge), where the model's value is
#   r1147_qpsk budget 1: 1.238e-07
SYN_BOUND = {
    ("r1147_qpsk", 1): 4 * 1.238e-07,
    ("qpsk", 1): 4 * 1.281e-07,
    ("qpsk", 5): 4 * 1.423e-04,
    ("qpsk", 20): 4 * 5.409e-04,
    ("16qam", 20): 4 * 1.014e-03,
    ("64qam", 20): 4 * 9.540e-04,
}


NO_SYN_BOUND = {("r1147_qpsk", 20)}  # every other row asserts its SYN_BOUND


@pytest.mark.parametrize("matrix,name,budget,N", [
    pytest.param(MATRIX, "qpsk", 20, N, id="qpsk-20"), pytest.param(MATRIX, "16qam", 20, N, id="16qam-20"),
    pytest.param(MATRIX, "64qam", 20, N, id="64qam-20"), pytest.param(MATRIX, "qpsk", 1, N, id="qpsk-1"),
    pytest.param(MATRIX, "qpsk", 5, N, id="qpsk-5"),
    pytest.param(R1147, "r1147_qpsk", 20, N_R1147, id="r1147_qpsk-20"),
    pytest.param(R1147, "r1147_qpsk", 1, N_R1147, id="r1147_qpsk-1"),
])
def test_decisions_against_the_oracle(data_dir, matrix, name, budget, N):
    assert STREAM_MATRIX.get(name, MATRIX) == matrix
    ctx = f32_ctx(data_dir, name)
    p0 = stream(data_dir, name, N)["p0"]
    ref = oracle_decode(data_dir, name, N, budget)
    if budget == 20:
        assert_both_outcomes(ref["ret"])
    r = ctx.bp_decode(p0, budget, cc_hat=True, syn=np.full((N, ctx.M), SYN_FILL))
    assert ctx.bp_kernel() == F32_KERNEL
    d_uu = differing(r["uu_hat"], ref["uu_hat"])
    d_ret = r["ret"] != ref["ret"]
    d_cc = differing(r["cc_hat"], ref["cc_hat"])
    same = ~d_ret
    d_syn = float(np.max(np.abs(r["syn"][same] - ref["syn"][same])))
    bound = None if (name, budget) in NO_SYN_BOUND else SYN_BOUND[(name, budget)]
    print(f"{name} budget {budget}: codewords differing in uu_hat {int(d_uu.sum())}, ret {int(d_ret.sum())}, "
          f"cc_hat {int(d_cc.sum())} of {N}; max |syn - oracle| {d_syn:.3e} (bound {bound})")
    assert (ctx.K, ctx.chk) == ((1157, 1147) if matrix == R1147 else (1152, 1152))
    assert d_uu.mean() <= CAP
    assert d_ret.mean() <= CAP
    assert d_cc.mean() <= CAP
    if bound is not None:
        assert d_syn <= bound


def test_batch_and_queue_independence(data_dir):
    """B = 700 exceeds the resident workgroups (one per CU), so workgroups re-enter the dequeue loop."""
    ctx = f32_ctx(data_dir)
    p0 = stream(data_dir, "qpsk", N)["p0"]
    big = np.concatenate([p0, p0])[:700]
    runs = {}
    for tag, B in [("1", 1), ("3", 3), ("700", 700), ("700 again", 700)]:
        runs[tag] = ctx.bp_decode(big[:B], 20, cc_hat=True, syn=np.full((B, ctx.M), SYN_FILL))
    for key in ("uu_hat", "ret", "cc_hat", "syn"):
        assert np.array_equal(runs["700"][key], runs["700 again"][key]), key
        assert np.array_equal(runs["1"][key], runs["700"][key][:1]), key
        assert np.array_equal(runs["3"][key], runs["700"][key][:3]), key
        # the second copy of the stream sits at other queue positions
        assert np.array_equal(runs["700"][key][N:700], runs["700"][key][:700 - N]), key
    assert np.any(runs["700"]["ret"] == 20) and np.any(runs["700"]["ret"] < 20)


def test_batch_independence_at_rank_1147(data_dir):
    """The same on the rank-1147 code (uu_hat rows of 1157 bytes): B = 1, 3 and 96, the stream's first 48 twice."""
    ctx = f32_ctx(data_dir, "r1147_qpsk")
    p0 = stream(data_dir, "r1147_qpsk", N_R1147)["p0"][:48]
    big = np.concatenate([p0, p0])
    runs = {}
    for tag, B in [("1", 1), ("3", 3), ("96", 96), ("96 again", 96)]:
        runs[tag] = ctx.bp_decode(big[:B], 20, cc_hat=True, syn=np.full((B, ctx.M), SYN_FILL))
        assert ctx.bp_kernel() == F32_KERNEL
    for key in ("uu_hat", "ret", "cc_hat", "syn"):
        assert np.array_equal(runs["96"][key], runs["96 again"][key]), key
        assert np.array_equal(runs["1"][key], runs["96"][key][:1]), key
        assert np.array_equal(runs["3"][key], runs["96"][key][:3]), key
        assert np.array_equal(runs["96"][key][48:], runs["96"][key][:48]), key
    assert np.any(runs["96"]["ret"] == 20) and np.any(runs["96"]["ret"] < 20)


def _check_golden_f64(ctx, z):
    p0 = z["v_p0"]
    B = p0.shape[0]
    r = ctx.bp_decode(p0, cc_hat=True, syn=np.full((B, ctx.M), -1.0))
    assert np.array_equal(r["ret"], z["s_ret"][:B])
    assert np.array_equal(r["uu_hat"], z["v_uu_hat"])
    assert np.array_equal(r["cc_hat"], z["v_cc_hat"])
    for i in range(B):
        if r["ret"][i] > 1:
            assert np.array_equal(r["syn"][i], z["v_syn"][i]), f"syndrom_soft cw {i}"


def test_no_leakage_between_modes(data_dir):
    hdr, z = load_case("peg2304_qpsk_known")
    ctx = ctx_for(data_dir, hdr["modem"])
    ctx.set_precision("f64")
    _check_golden_f64(ctx, z)
    assert ctx.bp_kernel() == F64_KERNEL
    ctx.set_precision("f32")
    assert ctx.precision == "f32"
    B = z["v_p0"].shape[0]
    r = ctx.bp_decode(z["v_p0"], cc_hat=True, syn=np.full((B, ctx.M), -1.0))
    assert ctx.bp_kernel() == F32_KERNEL
    assert r["ret"].min() >= 1 and r["ret"].max() <= 20
    ctx.set_precision("f64")
    assert ctx.precision == "f64"
    _check_golden_f64(ctx, z)
    assert ctx.bp_kernel() == F64_KERNEL


def test_fused_and_separate_demap_agree(data_dir):
    _fused_and_separate_demap_agree(data_dir, "qpsk", N, 256)


def test_fused_and_separate_demap_agree_at_rank_1147(data_dir):
    _fused_and_separate_demap_agree(data_dir, "r1147_qpsk", N_R1147, N_R1147)


def _fused_and_separate_demap_agree(data_dir, name, N, n):
    ctx = f32_ctx(data_dir, name)
    s = stream(data_dir, name, N)
    y, th = s["y"][:n], s["th"][:n]
    fused = ctx.decode_frames(y, s["snr"], th)
    assert ctx.bp_kernel() == F32_KERNEL
    p0 = ctx.demap(y, th, 10.0 ** (-0.1 * s["snr"]))
    sep = ctx.bp_decode(p0, 20)
    assert ctx.bp_kernel() == F32_KERNEL
    assert np.array_equal(fused["uu_hat"], sep["uu_hat"])
    assert np.array_equal(fused["ret"], sep["ret"])


def test_blind_path_front_end_untouched(data_dir):
    s = stream(data_dir, "qpsk", N)
    n = 256
    y = s["y"][:n]
    ctx = ctx_for(data_dir, STREAMS["qpsk"][0])
    ctx.set_precision("f64")
    ref = ctx.decode_frames(y, s["snr"])
    ctx.set_precision("f32")
    out = ctx.decode_frames(y, s["snr"])
    assert ctx.bp_kernel() == F32_KERNEL
    for key in ("chosen", "metrics", "h_hat"):
        assert np.array_equal(out[key], ref[key]), key
    d = differing(out["uu_hat"], ref["uu_hat"])
    print(f"blind: {int(d.sum())} of {n} codewords differ in uu_hat")
    assert d.mean() <= CAP


def test_simulator_path(data_dir):
    n = 2048
    modem, snr = STREAMS["qpsk"]
    oc = O.Code(os.path.join(data_dir, MATRIX), False, True, False, 20)
    om = O.Modem(os.path.join(data_dir, modem))
    uu, _, th, y = O.gen_frames(oc, om, snr, n)
    ctx = ctx_for(data_dir, modem)
    ctx.sim_load(snr, uu.astype(np.uint8), y, th)
    ctx.set_precision("f64")
    e64, _, c64 = ctx.sim_decode_ex(snr)
    assert ctx.bp_kernel() == F64_KERNEL
    ctx.set_precision("f32")
    e32, _, c32 = ctx.sim_decode_ex(snr)
    assert ctx.bp_kernel() == F32_KERNEL
    ndiff = int(np.sum(e64 != e32))
    print(f"sim: cw_err differs on {ndiff} of {n}; err_blk {c64['err_blk']} / {c32['err_blk']}, "
          f"err_bit {c64['err_bit']} / {c32['err_bit']}")
    assert ndiff <= CAP * n
    assert c32["tot_blk"] == c64["tot_blk"] == n
    assert c32["tot_bit"] == c64["tot_bit"]
    assert c32["redone"] == 0
    assert abs(c32["err_blk"] - c64["err_blk"]) <= ndiff
    assert c32["err_bit"] == int(e32.sum()) and c32["err_blk"] == int(np.sum(e32 > 0))
    # the plain entry point counts the same
    c = ctx.sim_decode(snr)
    assert (c["err_bit"], c["err_blk"], c["tot_blk"]) == (c32["err_bit"], c32["err_blk"], n)
    ctx.set_precision("f64")


@pytest.mark.parametrize("case", ["bg2_qpsk_known", "peg8064_qpsk_known", "syn_reg36_192_qpsk_blind"])
def test_other_codes_refuse_f32(data_dir, case):
    hdr, z = load_case(case)
    assert hdr["active"]
    ctx = ctx_for(data_dir, hdr["modem"], hdr["matrix"], bool(hdr["is5g"]), hdr["max_iter"])
    with pytest.raises(K.KmlError, match=r"\(code -4\)"):  # KML_E_UNSUP
        ctx.set_precision("f32")
    assert ctx.precision == "f64"
    _check_golden_f64(ctx, z)
    assert ctx.bp_kernel() != F32_KERNEL


@pytest.mark.parametrize("case", ["syn_reg36_2304_qpsk_known", "syn_reg36_2304_r1147_16qam_known"])
def test_peg2304_class_codes_accept_f32(data_dir, case):
    """The counter-case: any (3,6)-regular 2304 x 1152 code takes the mode, full rank or not, and leaves it again."""
    hdr, z = load_case(case)
    ctx = ctx_for(data_dir, hdr["modem"], hdr["matrix"], False, hdr["max_iter"])
    ctx.set_precision("f32")
    assert ctx.precision == "f32"
    B = z["v_p0"].shape[0]
    r = ctx.bp_decode(z["v_p0"], cc_hat=True, syn=np.full((B, ctx.M), -1.0))
    assert ctx.bp_kernel() == F32_KERNEL
    assert r["ret"].min() >= 1 and r["ret"].max() <= 20
    ctx.set_precision("f64")
    assert ctx.precision == "f64"
    _check_golden_f64(ctx, z)
    assert ctx.bp_kernel() == F64_KERNEL


def test_unknown_precision_is_an_argument_error(data_dir):
    ctx = ctx_for(data_dir, STREAMS["qpsk"][0])
    ctx.set_precision("f64")
    with pytest.raises(K.KmlError, match=r"\(code -1\)"):  # KML_E_ARG
        ctx.set_precision("f16")
    assert K.lib().kml_set_precision(ctx._h, 2) == -1
    assert ctx.precision == "f64"


def test_zero_iterations_leave_the_outputs(data_dir):
    ctx = f32_ctx(data_dir)
    B = 5
    p0 = np.ascontiguousarray(stream(data_dir, "qpsk", N)["p0"][:B])
    uh = np.full((B, ctx.K), 7, np.uint8)
    cch = np.full((B, ctx.Ncol), 9, np.uint8)
    ret = np.full(B, -5, np.int32)
    ptr = lambda a: a.ctypes.data_as(K.C.c_void_p)
    rc = K.lib().kml_bp_decode(ctx._h, ptr(p0), B, 0, ptr(uh), ptr(ret), ptr(cch), None, 0)
    assert rc == 0
    assert ctx.bp_kernel() == F32_KERNEL
    assert np.all(uh == 7) and np.all(cch == 9)
    assert np.all(ret == 1)  # iter = 0 < max_iter
    ctx.set_precision("f64")
