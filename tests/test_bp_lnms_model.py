"""The layered min-sum contract (tests/bp_lnms_model.py): CPU checks of the model
itself, on 5G BG2 K960, syn_irr1200 and syn_qc_l200 (the three codes of
tests/test_gpu_lnms.py, which holds the GPU kernel to the model bit for bit).

BG2's and syn_irr1200's streams are those of test_bp_nms_model.py; syn_qc_l200
(tests/golden/make_codes_layered.py: 4 layers of 200 rows, more than one pass of
the kernel's 96 rows and not a multiple of it) gets a QPSK stream of its own.
The model's decodes are made once per session and shared with the GPU tests
(read-only).
"""
import os

import numpy as np
import pytest

import test_bp_nms_model as F
from bp_lnms_model import layers, lnms_model, lnms_rowwise
from bp_nms_model import CLAMP
from oracle import oracle as O

# The new code's entry, in the format of test_bp_nms_model.CODES.  The SNR comes
# from a scan of the layered model over 128 seed-17 codewords (share converged:
# 1 dB 0.29, 2 dB 0.41, 3 dB 0.46, 4 dB 0.55, 5 dB 0.63, 6 dB 0.67).
QC = "syn_qc_l200"
CODES = dict(F.CODES)
CODES[QC] = ("syn_qc_l200.txt", False, 20, "2bits_QPSK.txt", 3.0)
N_STREAM = F.N_STREAM
MIN_SHARE = F.MIN_SHARE
# name: (layers, fewest rows of a layer, most)
LAYERS = {"bg2": (12, 96, 96), "syn_irr1200": (91, 1, 17), QC: (4, 200, 200)}

_cache = {}


def code(data_dir, name):
    """(oracle code, model graph) of a code, made once (BG2 and syn_irr1200: test_bp_nms_model's own)."""
    if name in F.CODES:
        return F.code(data_dir, name)
    key = ("code", data_dir, name)
    if key not in _cache:
        matrix, is5g, max_iter, _, _ = CODES[name]
        oc = O.Code(os.path.join(data_dir, matrix), is5g, True, False, max_iter)
        _cache[key] = (oc, F.Graph(oc))
    return _cache[key]


def stream(data_dir, name, n=N_STREAM):
    """The first n seed-17 codewords of the code's stream (read-only)."""
    if name in F.CODES:
        return F.stream(data_dir, name, n)
    key = ("stream", data_dir, name, n)
    if key not in _cache:
        _, _, _, modem, snr = CODES[name]
        oc, _ = code(data_dir, name)
        om = O.Modem(os.path.join(data_dir, modem))
        uu, cc, th, y = O.gen_frames(oc, om, snr, n)
        var = 10.0 ** (-0.1 * snr)
        p0 = np.stack([om.demap(y[i], th[i], var) for i in range(n)])
        for a in (uu, cc, th, y, p0):
            a.setflags(write=False)
        _cache[key] = dict(uu=uu, cc=cc, th=th, y=y, p0=p0, snr=snr, modem=modem)
    return _cache[key]


def layered_decode(data_dir, name, p0_key, p0, iter_count, alpha=0.75):
    """The layered model's decode of a named input at a budget (read-only, made once)."""
    key = ("dec", data_dir, name, p0_key, iter_count, float(np.float32(alpha)))
    if key not in _cache:
        _, g = code(data_dir, name)
        stats = {}
        ret, uh, cch = lnms_model(g, p0, iter_count, CODES[name][2], alpha, stats=stats)
        for a in (ret, uh, cch):
            a.setflags(write=False)
        _cache[key] = dict(ret=ret, uu_hat=uh, cc_hat=cch, stats=stats)
    return _cache[key]


def fer(d, uu):
    return float(np.mean((d["uu_hat"] != uu.astype(np.uint8)).any(axis=1)))


# ---- tests -----------------------------------------------------------------

@pytest.mark.parametrize("name", list(CODES))
def test_layers_of_the_greedy_rule(data_dir, name):
    _, g = code(data_dir, name)
    lp = layers(g)
    nl, lo, hi = LAYERS[name]
    sizes = np.diff(lp)
    assert (len(lp) - 1, int(sizes.min()), int(sizes.max())) == (nl, lo, hi)
    assert lp[0] == 0 and lp[-1] == g.M
    for a, b in zip(lp[:-1], lp[1:]):  # disjoint inside, and maximal: the next row shares a column
        cols = g.rc[g.rp[a]:g.rp[b]]
        assert len(set(cols.tolist())) == len(cols)
        if b < g.M:
            assert set(g.rc[g.rp[b]:g.rp[b + 1]].tolist()) & set(cols.tolist())


def test_the_new_code_is_what_its_generator_says(data_dir):
    oc, g = code(data_dir, QC)
    assert (g.M, g.N, g.E, g.K) == (800, 1600, 4400, 800)
    dv, dc = np.diff(g.cp), np.diff(g.rp)
    assert (dv.min(), dv.max(), dc.min(), dc.max()) == (2, 4, 5, 6)
    assert 200 > 96 and 200 % 96 != 0  # a layer is two full passes of the kernel and a partial one


@pytest.mark.parametrize("alpha", [0.75, 1.0])
@pytest.mark.parametrize("name", list(CODES))
def test_vectorised_model_equals_the_row_by_row_loop(data_dir, name, alpha):
    """4 stream codewords, 8 sweeps (the loop costs a second per code at that budget): bit for bit."""
    _, g = code(data_dir, name)
    p0 = stream(data_dir, name)["p0"][:4]
    max_iter = CODES[name][2]
    a = lnms_model(g, p0, 8, max_iter, alpha)
    b = lnms_rowwise(g, p0, 8, max_iter, alpha)
    for x, y, what in zip(a, b, ("ret", "uu_hat", "cc_hat")):
        assert np.array_equal(x, y), what
    if name == "bg2":
        assert a[0].max() == 9 and a[0].min() < 9  # both a stopped codeword and one that runs all 8 sweeps


@pytest.mark.parametrize("name", list(CODES))
def test_noiseless_codewords_decode(data_dir, name):
    oc, g = code(data_dir, name)
    rng = np.random.default_rng(5)
    uu = rng.integers(0, 2, (8, oc.K)).astype(np.int32)
    cc = np.stack([oc.encode(u) for u in uu])
    p0 = np.where(cc == 0, 0.95, 0.05)
    max_iter = CODES[name][2]
    ret, uh, cch = lnms_model(g, p0, max_iter, max_iter)
    assert np.array_equal(uh, uu.astype(np.uint8))
    assert np.array_equal(cch[:, g.punct:], cc.astype(np.uint8))
    if name == "bg2":  # the punctured columns start undecided: a sweep or two fills them in
        assert ret.min() >= 2 and ret.max() <= 4
    else:              # every row is satisfied by the priors' decisions: no sweep at all
        assert np.all(ret == 1)


@pytest.mark.parametrize("name", list(CODES))
def test_stream_has_both_outcomes(data_dir, name):
    oc, g = code(data_dir, name)
    s = stream(data_dir, name)
    max_iter = CODES[name][2]
    d = layered_decode(data_dir, name, "stream", s["p0"], max_iter)
    conv = d["stats"]["converged"]
    print(f"{name}: converged {conv.mean():.3f}, FER {fer(d, s['uu']):.3f}")
    assert conv.mean() >= MIN_SHARE and 1.0 - conv.mean() >= MIN_SHARE, f"stream is one-sided: {conv.mean():.3f}"
    assert all(oc.parity_count(c) == 0 for c in d["cc_hat"][conv])
    assert np.array_equal(d["ret"] < max_iter, d["stats"]["iters"] < max_iter)
    assert d["stats"]["finite"]


# (budget 5, full budget, half budget; FER of flooding at 5, layered at 5, flooding at full, layered at half,
# flooding at half).  On syn_irr1200 the layered schedule at 10 sweeps (0.492) equals flooding at 20 (0.492)
# and is below flooding at the same 10 (0.578).
EXPECTED = {"bg2": (5, 50, 25, 0.875, 0.734, 0.617, 0.617, 0.648),
            "syn_irr1200": (5, 20, 10, 0.766, 0.594, 0.492, 0.492, 0.578)}


@pytest.mark.parametrize("name", list(EXPECTED))
def test_layered_needs_half_the_budget(data_dir, name):
    """Deterministic CPU results: other values mean the contract was built differently."""
    small, full, half, f_small, l_small, f_full, l_half, f_half = EXPECTED[name]
    s = stream(data_dir, name)
    uu = s["uu"]
    fl = lambda b: fer(F.model_decode(data_dir, name, "stream", s["p0"], b), uu)
    la = lambda b: fer(layered_decode(data_dir, name, "stream", s["p0"], b), uu)
    got = (fl(small), la(small), fl(full), la(half), fl(half))
    print(f"{name}: flooding@{small} {got[0]:.3f} layered@{small} {got[1]:.3f} "
          f"flooding@{full} {got[2]:.3f} layered@{half} {got[3]:.3f} flooding@{half} {got[4]:.3f}")
    assert got[1] < got[0]
    assert got[3] <= got[2]
    assert got[3] <= got[4]
    assert [round(x, 3) for x in got] == [f_small, l_small, f_full, l_half, f_half]


def test_the_clamp_is_reached_and_everything_stays_finite(data_dir):
    """max |m| is exactly 256 on the syn_irr1200 stream and on the saturated priors; every posterior is
    m + c2v with |m| <= 256 and |c2v| <= alpha * 256."""
    s = stream(data_dir, "syn_irr1200")
    d = layered_decode(data_dir, "syn_irr1200", "stream", s["p0"], 20)
    assert d["stats"]["max_abs_m"] == float(CLAMP)
    sat = layered_decode(data_dir, "bg2", "saturated", F.saturated_p0(data_dir), 50)
    assert sat["stats"]["max_abs_m"] == float(CLAMP)
    rnd = layered_decode(data_dir, "bg2", "random", F.random_p0(data_dir), 50)
    for x in (d, sat, rnd):
        assert x["stats"]["finite"]
        assert x["stats"]["max_abs_T"] <= 256.0 + 256.0 * 0.75
    one = {}
    _, g = code(data_dir, "syn_irr1200")
    lnms_model(g, s["p0"][:32], 20, 20, 1.0, stats=one)
    assert one["finite"] and one["max_abs_T"] <= 512.0


def test_ret_semantics(data_dir):
    _, g = code(data_dir, "bg2")
    p0 = stream(data_dir, "bg2")["p0"][:16]
    full = layered_decode(data_dir, "bg2", "stream", stream(data_dir, "bg2")["p0"], 50)
    assert np.any(full["ret"][:16] == 50) and np.any(full["ret"][:16] < 50)
    ret, uh, cch = lnms_model(g, p0, 0, 50)  # no sweep: it = 0, outputs as passed (zeros here)
    assert np.all(ret == 1) and not uh.any() and not cch.any()
    ret, uh, cch = lnms_model(g, p0, 1, 50)  # one sweep, then the decisions of its posteriors
    assert np.all(ret == 2)                  # (none of these satisfies the checks before or after one sweep)
    assert cch.any()
    ret, _, _ = lnms_model(g, p0, 50, 50)    # it = max_iter is not incremented
    assert np.array_equal(ret, full["ret"][:16])
    ret5, _, _ = lnms_model(g, p0, 5, 50)    # a budget below max_iter: it + 1, converged or not
    assert np.array_equal(ret5, np.minimum(full["stats"]["iters"][:16], 5) + 1)
