"""What the tests of the lifted BG2 codes share (tests/test_lifted_host.py,
tests/test_bp_lifted_model.py, tests/test_gpu_lifted.py and its child process):
the code files, the model graphs, the input stream and the models' decodes, each
made once per process and read-only.

The codes come from tests/golden/make_codes_lifted.py: Z = 128 is committed
(syn_bg2_z128), the larger ones are built into a temporary directory.

The stream is the all-zero codeword with BPSK-like LLRs:
    y = 1 + default_rng(7).normal(size=(B, cc_len)) * sqrt(var / 2), var = 10 ** (-snr / 10),
    L = float32(4 * y / var),  P0 = 1 / (1 + exp(-L)),
at snr = -2.0 dB, where the layered model at 25 sweeps, alpha 0.75, leaves both
outcomes (at -3.0 nothing converges, at -1.7 nearly everything does).
"""
import os
import sys

import numpy as np

from bp_nms_model import Graph
from oracle import oracle as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_codes_lifted  # noqa: E402

SNR = -2.0
MAX_ITER = 25
MODEM = "4bit_16QAM_Gray.txt"
_cache = {}


def matrix_path(data_dir, Z, tmp_dir=None):
    """The code's file: the committed one (decompressed into data_dir) for Z = 128, else built into tmp_dir."""
    if Z == make_codes_lifted.COMMITTED_Z:
        return os.path.join(data_dir, make_codes_lifted.NAME + ".txt")
    key = ("file", Z)
    if key not in _cache or not os.path.exists(_cache[key]):
        _cache[key] = make_codes_lifted.write(Z, str(tmp_dir))
    return _cache[key]


def graph(data_dir, Z, tmp_dir=None):
    """(oracle code, model graph)."""
    key = ("graph", Z)
    if key not in _cache:
        oc = O.Code(matrix_path(data_dir, Z, tmp_dir), True, True, False, MAX_ITER)
        _cache[key] = (oc, Graph(oc))
    return _cache[key]


def llr_stream(cc_len, B, snr=SNR):
    """L[B, cc_len] float32 of the stream (read-only)."""
    key = ("llr", cc_len, B, snr)
    if key not in _cache:
        var = 10.0 ** (-snr / 10.0)
        y = 1.0 + np.random.default_rng(7).normal(size=(B, cc_len)) * np.sqrt(var / 2.0)
        L = (4.0 * y / var).astype(np.float32)
        L.setflags(write=False)
        _cache[key] = L
    return _cache[key]


def p0_stream(cc_len, B, snr=SNR):
    """The same stream as P(bit = 0), float64."""
    return 1.0 / (1.0 + np.exp(-llr_stream(cc_len, B, snr).astype(np.float64)))


def ctx_args(data_dir, Z, tmp_dir=None, **kw):
    """Keyword arguments of K.Context for the code with the 16QAM modem."""
    args = dict(matrix_file=matrix_path(data_dir, Z, tmp_dir), modem_file=os.path.join(data_dir, MODEM), is5g=True,
                max_iter=MAX_ITER)
    args.update(kw)
    return args


# ---- what the GPU tests and their child process run -------------------------

FAMILIES = {False: {"f32": "bp_irregular_lnms_kernel", "f16": "bp_irregular_lnms_h16_kernel"},
            True: {"f32": "bp_irregular_lnms_gt_kernel", "f16": "bp_irregular_lnms_h16_gt_kernel"}}
KEYS = ("ret", "uu_hat", "cc_hat", "llr_out")


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(r, m, what):
    """Equality of bit patterns on every key both sides have."""
    for key in KEYS:
        if key in r and key in m:
            x, y = (u32(r[key]), u32(m[key])) if key == "llr_out" else (np.asarray(r[key]), np.asarray(m[key]))
            bad = np.nonzero((x != y).reshape(len(y), -1).any(axis=1))[0]
            assert bad.size == 0, f"{what}: {key} differs from the model on codewords {bad[:8]} ({bad.size} in all)"


def llr_model(g, llr, budget, max_iter, alpha, beta, messages):
    from bp_oms_model import oms_llr_model
    key = ("llrm", g.N, llr.shape[0], float(llr.flat[0]), budget, max_iter, float(alpha), float(beta), messages)
    if key not in _cache:
        _cache[key] = dict(zip(KEYS, oms_llr_model(g, llr, budget, max_iter, alpha, beta, "layered", messages)))
    return _cache[key]


def p0_model(g, p0, budget, max_iter, alpha, beta, messages):
    from bp_oms_model import oms_decode
    return dict(zip(KEYS[:3], oms_decode(g, p0, budget, max_iter, alpha, beta, "layered", messages)))


def layered_mode(ctx, alpha, beta, messages):
    ctx.set_algorithm("nms", alpha)
    ctx.set_schedule("layered")
    ctx.set_messages(messages)
    ctx.set_offset(beta)


def check_llr_decodes(ctx, g, families, messages, alpha, beta, budgets=(25, 5, 1, 0), B=16):
    """llr_decode with llr_out on the stream, every budget: the model's bits, the expected kernel family."""
    layered_mode(ctx, alpha, beta, messages)
    llr = llr_stream(g.cc_len, B)
    for budget in budgets:
        m = llr_model(g, llr, budget, MAX_ITER, alpha, beta, messages)
        r = ctx.llr_decode(llr, budget, cc_hat=True, llr_out=True)
        assert ctx.bp_kernel() == families[messages], ctx.bp_kernel()
        same(r, m, f"{messages} budget {budget} ({alpha}, {beta})")
        same(ctx.llr_decode(llr, budget, cc_hat=True), m, f"{messages} budget {budget} ({alpha}, {beta}), no llr_out")
        if budget == MAX_ITER and B >= 16 and (alpha, beta) == (0.75, 0.0):  # (the setting the stream was chosen at)
            assert np.any(m["ret"] == MAX_ITER) and np.any(m["ret"] < MAX_ITER)
    ctx.set_algorithm("spa")


def check_batches(ctx, g, families, messages):
    """B = 1, 3 and 37, twice on one context: a codeword's result does not depend on its batch, its queue slot
    or (binary16) its partner; an odd B leaves the binary16 kernel an unpaired half."""
    layered_mode(ctx, 0.75, 0.0, messages)
    llr = llr_stream(g.cc_len, 37)
    m = llr_model(g, llr, MAX_ITER, MAX_ITER, 0.75, 0.0, messages)
    for _ in range(2):
        for B in (1, 3, 37):
            r = ctx.llr_decode(llr[:B], MAX_ITER, cc_hat=True, llr_out=True)
            assert ctx.bp_kernel() == families[messages]
            same(r, {k: v[:B] for k, v in m.items()}, f"{messages} B = {B}")
    ctx.set_algorithm("spa")


def check_p0_decode(ctx, g, families, messages, B=16):
    """bp_decode from P0: the exact front end's instances."""
    layered_mode(ctx, 0.75, 0.0, messages)
    p0 = p0_stream(g.cc_len, B)
    r = ctx.bp_decode(p0, MAX_ITER, cc_hat=True)
    assert ctx.bp_kernel() == families[messages]
    same(r, p0_model(g, p0, MAX_ITER, MAX_ITER, 0.75, 0.0, messages), f"{messages} P0")
    ctx.set_algorithm("spa")
