"""The LLR front end's contract (tests/bp_llr_model.py): CPU checks of the models
themselves on the three codes and seed-17 streams of test_bp_lnms_model.py.
tests/test_gpu_llr.py holds the GPU kernels to these models bit for bit; the
streams' max-log LLRs and the models' decodes of them are made once per session
and shared with it (read-only).
"""
import os

import numpy as np
import pytest

import test_bp_nms_model as F
from bp_llr_model import (blind_metric, llr_decode_model, llr_priors, lnms_llr_model, maxlog_llr, nms_llr_model,
                          parity_counts)
from bp_nms_model import CLAMP, priors
from oracle import oracle as O
from test_bp_lnms_model import CODES, MIN_SHARE, QC, code, layered_decode, stream

import kmldpc_amd as K

SCHEDULES = ("flooding", "layered")
_cache = {}


def points(data_dir, name):
    """The context's normalised constellation (kml_constellation, a host-only context) and bits per symbol."""
    key = ("points", data_dir, name)
    if key not in _cache:
        matrix, is5g, max_iter, modem, _ = CODES[name]
        ctx = K.Context(matrix_file=os.path.join(data_dir, matrix), modem_file=os.path.join(data_dir, modem),
                        is5g=is5g, max_iter=max_iter, device=-1)
        pts = ctx.constellation()
        pts.setflags(write=False)
        _cache[key] = (pts, ctx.bits)
        ctx.close()
    return _cache[key]


def llr_stream(data_dir, name, n=F.N_STREAM):
    """Max-log LLRs [n, cc_len] of the stream's frames with the true channel (read-only)."""
    key = ("llr", data_dir, name, n)
    if key not in _cache:
        s = stream(data_dir, name, n)
        pts, bits = points(data_dir, name)
        llr = maxlog_llr(pts, bits, s["y"], s["th"], 10.0 ** (-0.1 * s["snr"]))
        llr.setflags(write=False)
        _cache[key] = llr
    return _cache[key]


def llr_decoded(data_dir, name, llr_key, llr, budget, alpha=0.75, schedule="flooding"):
    """The LLR-prior model's decode of a named input at a budget (read-only, made once)."""
    key = ("dec", data_dir, name, llr_key, budget, float(np.float32(alpha)), schedule)
    if key not in _cache:
        _, g = code(data_dir, name)
        stats = {}
        ret, uh, cch, T = llr_decode_model(g, llr, budget, CODES[name][2], alpha, schedule, stats=stats)
        for a in (ret, uh, cch, T):
            a.setflags(write=False)
        _cache[key] = dict(ret=ret, uu_hat=uh, cc_hat=cch, llr_out=T, stats=stats)
    return _cache[key]


def clamp_inputs(g, base):
    """8 codewords for the input clamp, from an LLR row `base`: its values scaled into +-inf, +-1e30, +-256 exactly,
    just past 256, +-0, denormals of both signs, and a mix of all of them."""
    rng = np.random.default_rng(9)
    sgn = np.where(np.signbit(base), np.float32(-1), np.float32(1))
    rows = [sgn * np.float32(np.inf), sgn * np.float32(1e30), sgn * np.float32(256.0),
            sgn * np.nextafter(np.float32(256.0), np.float32(np.inf)),
            np.where(rng.random(g.cc_len) < 0.5, np.float32(0.0), np.float32(-0.0)),
            sgn * np.float32(1e-42)]
    mix = base.copy()
    pick = rng.integers(0, 8, g.cc_len)
    for k, v in enumerate([np.inf, -np.inf, 1e30, -1e30, 256.0, -256.0, -0.0, 1e-42]):
        mix[pick == k] = np.float32(v)
    rows += [mix, base * np.float32(40.0)]
    x = np.stack(rows).astype(np.float32)
    x.setflags(write=False)
    return x


def fer(d, uu):
    return float(np.mean((d["uu_hat"] != uu.astype(np.uint8)).any(axis=1)))


# ---- tests -----------------------------------------------------------------

@pytest.mark.parametrize("name,budgets", [("bg2", (5, 2)), ("syn_irr1200", (20, 3)), (QC, (20, 4))])
def test_old_and_new_models_agree(data_dir, name, budgets):
    """The LLR-prior decoders fed priors(g, p0) return the P0 models' ret, uu_hat and cc_hat."""
    _, g = code(data_dir, name)
    p0 = stream(data_dir, name)["p0"][:32]
    L = priors(g, p0)[:, g.punct:]
    assert float(np.abs(L).max()) < 27.7  # the clamp does nothing to these
    max_iter = CODES[name][2]
    from bp_lnms_model import lnms_model
    from bp_nms_model import nms_model
    for b in budgets:
        for old, new in ((nms_model, nms_llr_model), (lnms_model, lnms_llr_model)):
            want = old(g, p0, b, max_iter)
            got = new(g, L, b, max_iter)
            for x, y, what in zip(want, got[:3], ("ret", "uu_hat", "cc_hat")):
                assert np.array_equal(x, y), (name, b, old.__name__, what)


# name: (budgets full / half / 5, flooding FER at each, layered FER at each) with max-log priors
EXPECTED = {"bg2": ((50, 25, 5), (0.6172, 0.6484, 0.8750), (0.6172, 0.6172, 0.7422)),
            "syn_irr1200": ((20, 10, 5), (0.4922, 0.5781, 0.7578), (0.4766, 0.4922, 0.5938))}
# ... and with the exact demapper's priors (the P0 models; test_bp_lnms_model.EXPECTED holds some of them)
EXACT = {"bg2": ((0.6172, 0.6484, 0.8750), (0.6172, 0.6172, 0.7344)),
         "syn_irr1200": ((0.4922, 0.5781, 0.7656), (0.4766, 0.4922, 0.5938))}


@pytest.mark.parametrize("name", list(EXPECTED))
def test_fer_table(data_dir, name):
    """Deterministic CPU results: other values mean the contract was built differently."""
    budgets, flood, lay = EXPECTED[name]
    s = stream(data_dir, name)
    llr = llr_stream(data_dir, name)
    got_f = [fer(llr_decoded(data_dir, name, "stream", llr, b, schedule="flooding"), s["uu"]) for b in budgets]
    got_l = [fer(llr_decoded(data_dir, name, "stream", llr, b, schedule="layered"), s["uu"]) for b in budgets]
    ex_f = [fer(F.model_decode(data_dir, name, "stream", s["p0"], b), s["uu"]) for b in budgets]
    ex_l = [fer(layered_decode(data_dir, name, "stream", s["p0"], b), s["uu"]) for b in budgets]
    print(f"{name}: max-log flooding {got_f} layered {got_l}; exact flooding {ex_f} layered {ex_l}")
    assert [round(x, 4) for x in got_f] == list(flood)
    assert [round(x, 4) for x in got_l] == list(lay)
    assert [round(x, 4) for x in ex_f] == list(EXACT[name][0])
    assert [round(x, 4) for x in ex_l] == list(EXACT[name][1])
    assert got_f[0] == ex_f[0] and got_l[0] == ex_l[0]  # the exact demapper's FER at the full budget


def test_qpsk_decodes_identically(data_dir):
    """On QPSK a bit's max-log LLR has the exact LLR's sign and the decodes agree bit for bit at every budget."""
    s = stream(data_dir, QC)
    llr = llr_stream(data_dir, QC)
    for b in (20, 10, 5):
        ml = llr_decoded(data_dir, QC, "stream", llr, b, schedule="flooding")
        assert np.array_equal(ml["uu_hat"], F_qc_flooding(data_dir, s["p0"], b)), b
        ml = llr_decoded(data_dir, QC, "stream", llr, b, schedule="layered")
        assert np.array_equal(ml["uu_hat"], layered_decode(data_dir, QC, "stream", s["p0"], b)["uu_hat"]), b


def F_qc_flooding(data_dir, p0, budget):
    from bp_nms_model import nms_model
    _, g = code(data_dir, QC)
    return nms_model(g, p0, budget, CODES[QC][2])[1]


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("name", list(CODES))
def test_stream_has_both_outcomes(data_dir, name, schedule):
    oc, g = code(data_dir, name)
    max_iter = CODES[name][2]
    d = llr_decoded(data_dir, name, "stream", llr_stream(data_dir, name), max_iter, schedule=schedule)
    conv = d["stats"]["converged"]
    print(f"{name} {schedule}: converged {conv.mean():.3f}")
    assert conv.mean() >= MIN_SHARE and 1.0 - conv.mean() >= MIN_SHARE, f"stream is one-sided: {conv.mean():.3f}"
    assert all(oc.parity_count(c) == 0 for c in d["cc_hat"][conv])
    assert np.array_equal(parity_counts(g, d["cc_hat"]) == 0, conv)


# name: measured agreement of the max-log decisions with the exact demapper's (P0 > 0.5), and the bound asserted
LABELLING = {"bg2": (0.9686, 0.95), "syn_irr1200": (0.9819, 0.95), QC: (1.0, 1.0)}


@pytest.mark.parametrize("name", list(LABELLING))
def test_labelling_agrees_with_the_oracles_demapper(data_dir, name):
    """A wrong bit order lands far below."""
    measured, bound = LABELLING[name]
    s = stream(data_dir, name)
    llr = llr_stream(data_dir, name)
    assert llr.dtype == np.float32 and llr.shape == s["p0"].shape
    agree = float(np.mean((llr > 0) == (s["p0"] > 0.5)))
    print(f"{name}: decisions agree on {agree:.4f} of the bits; largest |L| {np.abs(llr).max():.1f}")
    assert agree >= bound
    assert round(agree, 4) == measured
    assert float(np.abs(llr).max()) < 256.0  # the streams do not reach the decoder's input clamp: clamp_inputs does


def test_the_constellation_is_the_oracles(data_dir):
    for name in CODES:
        pts, bits = points(data_dir, name)
        om = O.Modem(os.path.join(data_dir, CODES[name][3]))
        assert bits == om.m and np.array_equal(pts.ravel(), om.points)


def test_demapper_special_values(data_dir):
    pts, bits = points(data_dir, "bg2")
    S = 6
    one = np.ones((1, 2)) * [0.6, -0.3]
    y = np.zeros((1, S, 2))
    # y exactly on a point (after rounding both to float32): that point's d is 0
    p32 = pts.astype(np.float32).astype(np.float64)
    y[0, :, :] = p32[[0, 5, 10, 15, 3, 12]]
    L = maxlog_llr(pts, bits, y, [[1.0, 0.0]], 0.2)
    k = np.array([0, 5, 10, 15, 3, 12])
    want_bits = (k[:, None] >> (bits - 1 - np.arange(bits))[None, :]) & 1
    assert np.array_equal((L.reshape(S, bits) > 0), want_bits == 0)
    # h = 0: every distance is |y|^2, every L is +0
    L = maxlog_llr(pts, bits, np.random.default_rng(1).normal(size=(1, S, 2)), [[0.0, 0.0]], 0.2)
    assert not L.any() and not np.signbit(L).any()
    # y = 0 with a real h: the Gray-mapped square constellation is symmetric, the LLRs are finite
    L = maxlog_llr(pts, bits, np.zeros((1, S, 2)), one, 0.2)
    assert np.isfinite(L).all()
    # tiny values: the distances are float32 denormals and the result is still exact arithmetic on them
    L = maxlog_llr(pts, bits, np.full((1, S, 2), 1e-21), [[1e-21, 0.0]], 1e-3)
    assert np.isfinite(L).all()


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_input_clamp(data_dir, schedule):
    """+-inf, +-1e30, +-256, just past 256, +-0 and denormals decode as their clamped values."""
    _, g = code(data_dir, "bg2")
    x = clamp_inputs(g, llr_stream(data_dir, "bg2")[0].copy())
    assert np.isinf(x).any() and (np.abs(x[np.isfinite(x)]) > 256).any() and (x == 0).any()
    assert ((x != 0) & (np.abs(x) < np.finfo(np.float32).tiny)).any()  # denormals
    L = llr_priors(g, x)
    assert float(np.abs(L).max()) == 256.0 and np.isfinite(L).all()
    assert np.array_equal(L[:, g.punct:][np.abs(x) <= 256].view(np.uint32), x[np.abs(x) <= 256].view(np.uint32))
    clamped = np.minimum(np.maximum(x, -CLAMP), CLAMP)
    a = llr_decode_model(g, x, 8, 50, schedule=schedule)
    b = llr_decode_model(g, clamped, 8, 50, schedule=schedule)
    for p, q in zip(a, b):
        assert np.array_equal(p.view(np.uint8), q.view(np.uint8))
    assert np.isfinite(a[3]).all()


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_posteriors(data_dir, schedule):
    """T holds the decisions it is returned with; |T| <= 256 + dv_max * alpha * 256 (flooding: the prior plus dv
    messages of at most alpha * 256) and <= 256 + alpha * 256 (layered: m + c2v)."""
    _, g = code(data_dir, "bg2")
    llr = llr_stream(data_dir, "bg2")
    for b in (50, 5, 1):
        d = llr_decoded(data_dir, "bg2", "stream", llr, b, schedule=schedule)
        T = d["llr_out"]
        assert T.dtype == np.float32 and T.shape == (llr.shape[0], g.N)
        assert np.array_equal(np.where(T > 0, 0, 1).astype(np.uint8), d["cc_hat"])
        bound = 256.0 + (g.dv_max if schedule == "flooding" else 1) * 0.75 * 256.0
        assert np.isfinite(T).all() and d["stats"]["max_abs_T"] <= bound
    x = clamp_inputs(g, llr[0].copy())
    stats = {}
    T = llr_decode_model(g, x, 50, 50, 1.0, schedule, stats=stats)[3]
    assert np.isfinite(T).all() and stats["max_abs_T"] <= 256.0 + (g.dv_max if schedule == "flooding" else 1) * 256.0
    ret, uh, cch, T0 = llr_decode_model(g, llr[:4], 0, 50, schedule=schedule)  # no iteration: as passed (zeros)
    assert np.all(ret == 1) and not uh.any() and not cch.any() and not T0.any()


def test_metric_function(data_dir):
    """The blind 5G metric on the BG2 stream: more than one rotation is chosen, and its metrics are not the
    exact front end's (the reference's fp64 sum-product count after metric_iter iterations)."""
    n = 24
    oc, g = code(data_dir, "bg2")
    s = stream(data_dir, "bg2")
    pts, bits = points(data_dir, "bg2")
    om = O.Modem(os.path.join(data_dir, CODES["bg2"][3]))
    y = s["y"][:n]
    h4 = np.stack([O.rotations(O.kmeans_hhat(y[i], om.points)) for i in range(n)])
    var = 10.0 ** (-0.1 * s["snr"])
    for schedule in SCHEDULES:
        met, chosen, llrs = blind_metric(g, pts, bits, y, h4, var, 5, 50, schedule=schedule)
        assert met.shape == (n, 4) and chosen.dtype == np.int32 and llrs.shape == (n, 4, g.cc_len)
        assert len(set(chosen.tolist())) > 1
        assert np.array_equal(chosen, np.argmin(met, axis=1))
        exact = np.stack([O.receive(oc, om, y[i], s["th"][i], s["snr"], True, False, 5)["metrics"] for i in range(n)])
        print(f"{schedule}: chosen {np.bincount(chosen, minlength=4).tolist()}, "
              f"frames whose metrics differ from the exact front end's {int((met != exact).any(axis=1).sum())} / {n}")
        assert (met != exact).any()
    met2, chosen2, _ = blind_metric(g, pts, bits, y[:4], h4[:4, :2], var, 5, 50)  # two candidates: entries >= 2 are 0
    assert not met2[:, 2:].any() and set(chosen2.tolist()) <= {0, 1}
