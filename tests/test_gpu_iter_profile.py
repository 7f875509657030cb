"""kml_sim_decode_profile: one decode, BER / FER / converged for every iteration
budget up to max_iter (bp_regular.hip / bp_irregular.hip PROF instances).

The reference for budget k is the existing path: ctx.bp_decode(ctx.demap(y, h,
var), iter_count=k) counted against uu, and contexts created with max_iter = k.
Every comparison is an exact equality.

Frames come from O.gen_frames with the oracle's own seed (17).  The streams of
the cases hold no codeword that converges at iteration 0 (the channel is
a per-codeword fading h; measured with the oracle: PEG2304 / QPSK at 2 dB
converges at iterations 1..7 or not at all within 8), so the last 16 of the 96
frames of every case are noise-free frames (60 dB, seed 18) received at the
case's SNR: they converge at iteration 0 (BG2: at iteration 1, its punctured
columns have no decision before that, so no BG2 codeword converges at 0).

Two statements of the issue were mended, asking no less:
  * "prof[k-1, 2] equals the number of codewords with ret <= k - (k == P ? 0 :
    1)": with ret = iter + (iter < max_iter) of the budget-k bp_decode on the
    max_iter = P context, a codeword that converged within budget k < P has
    ret <= k (one that exhausted it has k + 1), which is what is asserted; at
    k == P ret = P is both "converged at iteration P - 1" and "exhausted", so
    that row is pinned by the plain path's converged counter and rows 1 and 3
    by contexts created with max_iter = 1 and 3.
  * "PEG2304 / QPSK at 12 dB: every row is constant, prof[:, 2] == B for every
    budget": at 12 dB only 28 of the 64 seed-17 codewords pass the parity check
    at iteration 0 and 56 within 8 iterations (|h| goes down to 0.31), in the
    existing path itself.  The 12 dB batch is kept and checked for what holds
    there (budget by budget equality, most codewords converge, rows are
    constant from the converging iteration on), and the literal assertions are
    made on a noise-free batch.
"""
import os

import numpy as np
import pytest

from oracle import oracle as O

import kmldpc_amd as K
from conftest import load_case

pytestmark = pytest.mark.gpu

PEG, PEG8064, BG2 = "PEG2304regular0.5.txt", "PEG8064regular0.5.txt", "5GLDPCBG2a3_R12_K960.txt"
IRR = "syn_irr1200.txt"  # non-5G irregular, every column degree 1..9 and row degree 2..10 (tests/golden/make_codes.py)
# PEG2304-class, rank 1147: K = 1157, so the PROF instances' per-iteration error count has a partial last word
R1147 = "syn_reg36_2304_r1147.txt"
QPSK, QAM16, QAM64 = "2bits_QPSK.txt", "4bit_16QAM_Gray.txt", "6bits_64QAM_Gray.txt"
# name: matrix, modem, 5G, Es/N0, environment
CASES = {
    "peg_qpsk_fused": (PEG, QPSK, False, 2.0, {}),
    "peg_qpsk_unfused": (PEG, QPSK, False, 2.0, {"KML_FUSED_DEMAP": "0"}),
    "peg_16qam": (PEG, QAM16, False, 8.0, {}),
    "bg2_16qam": (BG2, QAM16, True, 9.0, {}),  # the oracle fails 61 % of the seed-17 codewords within 8 iterations
    "syn_irr1200_qpsk": (IRR, QPSK, False, 4.0, {}),  # the PROF instances of the degrees BG2 does not have
    "r1147_qpsk_fused": (R1147, QPSK, False, 4.0, {}),
    "r1147_qpsk_unfused": (R1147, QPSK, False, 4.0, {"KML_FUSED_DEMAP": "0"}),
}
UNSUP = "(code -4)"


class Env:
    def __init__(self, data_dir):
        self.d = data_dir
        self._ctx, self._oc, self._om, self._frames, self._ref = {}, {}, {}, {}, {}

    def ctx(self, matrix, modem, is5g, max_iter, **kw):
        key = (matrix, modem, max_iter, tuple(sorted(kw.items())))
        if key not in self._ctx:
            self._ctx[key] = K.Context(matrix_file=os.path.join(self.d, matrix), modem_file=os.path.join(self.d, modem),
                                       is5g=is5g, max_iter=max_iter, device=0, **kw)
        return self._ctx[key]

    def oracle(self, matrix, modem, is5g):
        if matrix not in self._oc:
            self._oc[matrix] = O.Code(os.path.join(self.d, matrix), is5g, True, False, 20)
        if modem not in self._om:
            self._om[modem] = O.Modem(os.path.join(self.d, modem))
        return self._oc[matrix], self._om[modem]

    def frames(self, matrix, modem, is5g, snr, n, clean=0):
        """n frames: n - clean of the seed-17 stream at snr, then `clean` noise-free ones (seed 18)."""
        key = (matrix, modem, snr, n, clean)
        if key not in self._frames:
            oc, om = self.oracle(matrix, modem, is5g)
            uu, _, th, y = O.gen_frames(oc, om, snr, n - clean)
            if clean:
                u2, _, t2, y2 = O.gen_frames(oc, om, 60.0, clean, state=18)
                uu, th, y = np.concatenate([uu, u2]), np.concatenate([th, t2]), np.concatenate([y, y2])
            self._frames[key] = (uu.astype(np.uint8), th, y)
        return self._frames[key]

    def reference(self, key, ctx, uu, h, y, snr, P):
        """Per-budget error bits and return values of the existing path, once per key."""
        if key not in self._ref:
            p0 = ctx.demap(y, h, 10.0 ** (-0.1 * snr))
            err = np.zeros((uu.shape[0], P), np.int32)
            ret = np.zeros((uu.shape[0], P), np.int32)
            for k in range(1, P + 1):
                r = ctx.bp_decode(p0, iter_count=k)
                err[:, k - 1] = (r["uu_hat"] != uu).sum(1)
                ret[:, k - 1] = r["ret"]
            self._ref[key] = (err, ret)
        return self._ref[key]

    def close(self):
        for c in self._ctx.values():
            c.close()


@pytest.fixture(scope="module")
def env(data_dir):
    e = Env(data_dir)
    yield e
    e.close()


def _setenv(monkeypatch, envv):
    for k, v in envv.items():
        monkeypatch.setenv(k, v)


def _conv_from_ret(ret, P):
    """converged within budget k < P: ret = iter + (iter < P) <= k (exhausted: k + 1)"""
    if P == 1:
        return np.zeros((ret.shape[0], 0), bool)
    return np.stack([ret[:, k - 1] <= k for k in range(1, P)], 1)


def _check_rows(prof, cwp, err, ret, conv_P, P):
    B = err.shape[0]
    assert cwp.shape == (B, P) and prof.shape == (P, 3)
    print("cw_prof column sums", cwp.sum(0), "reference", err.sum(0), "prof", prof.tolist())
    assert np.array_equal(cwp, err)
    assert np.array_equal(prof[:, 0], err.sum(0).astype(np.uint64))
    assert np.array_equal(prof[:, 1], (err > 0).sum(0).astype(np.uint64))
    conv = _conv_from_ret(ret, P)
    assert np.array_equal(prof[:P - 1, 2], conv.sum(0).astype(np.uint64))
    assert int(prof[P - 1, 2]) == conv_P
    assert (np.diff(prof[:, 2].astype(np.int64)) >= 0).all()


@pytest.mark.parametrize("case", list(CASES))
def test_per_budget_equality_and_plain_path(env, monkeypatch, case):
    """cw_prof[:, k-1], prof[k-1] against the budget-k decodes of the existing
    path for every k <= P = 8 (B = 96), the convergence convention against
    contexts created with max_iter = 1 and 3, and the same call's ordinary
    outputs against kml_sim_decode / kml_sim_decode_ex."""
    matrix, modem, is5g, snr, envv = CASES[case]
    _setenv(monkeypatch, envv)
    P, B = 8, 96
    ctx = env.ctx(matrix, modem, is5g, P)
    uu, h, y = env.frames(matrix, modem, is5g, snr, B, clean=16)
    err, ret = env.reference((case, P), ctx, uu, h, y, snr, P)
    ctx.sim_load(snr, uu, y, h)
    plain = ctx.sim_decode(snr, blind=False)
    cw_err, _, plain_ex = ctx.sim_decode_ex(snr, blind=False)
    prof, cwp, cnt = ctx.sim_decode_profile(snr, blind=False)
    assert ctx.bp_kernel() == ("bp_irregular_kernel" if is5g or matrix == IRR else "bp_regular_kernel")
    if matrix == R1147:
        assert ctx.K == 1157 and ctx.chk == 1147
    _check_rows(prof, cwp, err, ret, plain["converged"], P)
    # the ordinary outputs of the profile call are the plain call's
    assert cnt == plain == plain_ex
    assert np.array_equal(cwp[:, P - 1], cw_err)
    assert (int(prof[P - 1, 0]), int(prof[P - 1, 1]), int(prof[P - 1, 2])) == (plain["err_bit"], plain["err_blk"],
                                                                             plain["converged"])
    # the convention, pinned by contexts whose max_iter is the budget
    for k in (1, 3):
        ck = env.ctx(matrix, modem, is5g, k)
        ck.sim_load(snr, uu, y, h)
        e_k, _, c_k = ck.sim_decode_ex(snr, blind=False)
        assert np.array_equal(cwp[:, k - 1], e_k), k
        assert (int(prof[k - 1, 0]), int(prof[k - 1, 1]), int(prof[k - 1, 2])) == (c_k["err_bit"], c_k["err_blk"],
                                                                                 c_k["converged"]), k
    # the stream holds every kind of codeword
    conv = _conv_from_ret(ret, P)
    if is5g:  # BG2's punctured columns start from the prior 0.5: no decision before iteration 1
        assert not conv[:, 0].any() and conv[:, 1].any(), "the noise-free codewords converge at iteration 1"
    else:
        assert conv[:, 0].any(), "no codeword converges at iteration 0"
    assert (conv[:, P - 2] & ~conv[:, 1]).any(), "no codeword converges at iterations 2..P-2"
    assert plain["converged"] < B, "every codeword converges"
    if case == "bg2_16qam":  # the SNR was picked where the decoder fails 30-70 % of the stream's codewords
        share = (err[:B - 16, P - 1] > 0).mean()
        print("BG2 / 16QAM at", snr, "dB: share of failing codewords", share)
        assert 0.3 <= share <= 0.7


@pytest.mark.parametrize("case", ["peg_qpsk_fused", "bg2_16qam"])
def test_modes(env, monkeypatch, case):
    """FAST, forced redo and exact-only give the same rows (P = 5, B = 64); under
    forced redo every codeword is redone, so a FAST decode's partial counts
    reaching the rows would show."""
    matrix, modem, is5g, snr, _ = CASES[case]
    P, B = 5, 64
    ctx = env.ctx(matrix, modem, is5g, P)
    uu, h, y = env.frames(matrix, modem, is5g, snr, B, clean=8)
    err, ret = env.reference((case, P), ctx, uu, h, y, snr, P)
    ctx.sim_load(snr, uu, y, h)
    rows = {}
    for mode in ("fast", "KML_FORCE_REDO", "KML_NO_FAST"):
        with monkeypatch.context() as m:
            if mode != "fast":
                m.setenv(mode, "1")
            plain = ctx.sim_decode(snr, blind=False)
            prof, cwp, cnt = ctx.sim_decode_profile(snr, blind=False)
        assert cnt == plain, mode
        assert cnt["redone"] == (B if mode == "KML_FORCE_REDO" else 0), mode
        _check_rows(prof, cwp, err, ret, plain["converged"], P)
        rows[mode] = (prof, cwp)
    for mode in ("KML_FORCE_REDO", "KML_NO_FAST"):
        assert np.array_equal(rows[mode][0], rows["fast"][0]) and np.array_equal(rows[mode][1], rows["fast"][1])


def test_queue_reentry_and_batch_independence(env):
    """B = 1, 3 and 700 (more codewords than CUs: workgroups take several, perr
    and wprof are reused): a frame's row does not depend on the batch or the
    call, and prof is the column sums of cw_prof."""
    P = 8
    ctx = env.ctx(PEG, QPSK, False, P)
    uu, h, y = env.frames(PEG, QPSK, False, 2.0, 700)
    err96, _ = env.reference(("reentry", P), ctx, uu[:96], h[:96], y[:96], 2.0, P)
    big = None
    for B in (700, 3, 1):
        ctx.sim_load(2.0, uu[:B], y[:B], h[:B])
        prof, cwp, cnt = ctx.sim_decode_profile(2.0)
        prof2, cwp2, cnt2 = ctx.sim_decode_profile(2.0)
        assert np.array_equal(prof, prof2) and np.array_equal(cwp, cwp2) and cnt == cnt2
        assert np.array_equal(prof[:, 0], cwp.sum(0).astype(np.uint64))
        assert np.array_equal(prof[:, 1], (cwp > 0).sum(0).astype(np.uint64))
        assert cnt["tot_blk"] == B
        if B == 700:
            big = cwp
            assert np.array_equal(cwp[:96], err96)
        else:
            assert np.array_equal(cwp, big[:B])


def test_all_converge(env):
    """A noise-free batch: every row is constant and every budget has every
    codeword converged; and the 12 dB batch (see the module docstring)."""
    P, B = 8, 64
    ctx = env.ctx(PEG, QPSK, False, P)
    oc, om = env.oracle(PEG, QPSK, False)
    uu, _, h, y = O.gen_frames(oc, om, 60.0, B)
    ctx.sim_load(60.0, uu.astype(np.uint8), y, h)
    prof, cwp, cnt = ctx.sim_decode_profile(60.0)
    assert (cwp == cwp[:, :1]).all() and not cwp.any()
    assert (prof[:, 2] == B).all() and not prof[:, :2].any()
    assert cnt["converged"] == B and cnt["cn_phases"] == 0 and cnt["vn_phases"] == B
    uu, h, y = env.frames(PEG, QPSK, False, 12.0, B)
    err, ret = env.reference(("12dB", P), ctx, uu, h, y, 12.0, P)
    ctx.sim_load(12.0, uu, y, h)
    plain = ctx.sim_decode(12.0)
    prof, cwp, cnt = ctx.sim_decode_profile(12.0)
    _check_rows(prof, cwp, err, ret, plain["converged"], P)
    assert cnt == plain and B // 2 < cnt["converged"] == int(prof[P - 1, 2])
    conv = np.concatenate([_conv_from_ret(ret, P), np.ones((B, 1), bool)], 1)
    first = conv.argmax(1)  # the converging iteration
    for b in range(B):
        assert (cwp[b, first[b]:] == cwp[b, first[b]]).all(), b


def test_blind(env):
    """The blind path profiles the final decode only: per-budget bp_decode of the
    priors demapped with the chosen candidate."""
    P, B, snr = 6, 64, 2.0
    ctx = env.ctx(PEG, QPSK, False, P)
    uu, h, y = env.frames(PEG, QPSK, False, snr, B)
    chosen = ctx.decode_frames(y, snr)["chosen"]
    _, h4 = ctx.kmeans(y)
    hc = h4[np.arange(B), chosen]
    err, ret = env.reference(("blind", P), ctx, uu, hc, y, snr, P)
    ctx.sim_load(snr, uu, y, h)
    cw_err, _, plain = ctx.sim_decode_ex(snr, blind=True)
    prof, cwp, cnt = ctx.sim_decode_profile(snr, blind=True)
    _check_rows(prof, cwp, err, ret, plain["converged"], P)
    assert cnt == plain and np.array_equal(cwp[:, P - 1], cw_err)


@pytest.mark.parametrize("P", [1, 64])
def test_budget_extremes(env, P):
    B = 24
    ctx = env.ctx(PEG, QPSK, False, P)
    uu, h, y = env.frames(PEG, QPSK, False, 2.0, B, clean=4)
    err, ret = env.reference(("extreme", P), ctx, uu, h, y, 2.0, P)
    ctx.sim_load(2.0, uu, y, h)
    plain = ctx.sim_decode(2.0)
    prof, cwp, cnt = ctx.sim_decode_profile(2.0)
    _check_rows(prof, cwp, err, ret, plain["converged"], P)
    assert cnt == plain


def _golden_plain(env, name, n):
    """A context for a golden known-channel case with its first n seed-17 frames
    resident, and the golden counters of a plain decode of them."""
    hdr, z = load_case(name)
    uu, h, y = env.frames(hdr["matrix"], hdr["modem"], bool(hdr["is5g"]), hdr["snr"], n)
    errs = np.asarray(z["s_errs"][:n])
    return hdr, (uu, h, y), (int(errs.sum()), int((errs > 0).sum()), n * hdr["K"], n)


def _refused_then_plain(ctx, hdr, frames, golden, needle):
    uu, h, y = frames
    ctx.sim_load(hdr["snr"], uu, y, h)
    with pytest.raises(K.KmlError) as ei:
        ctx.sim_decode_profile(hdr["snr"])
    assert UNSUP in str(ei.value) and needle in str(ei.value), str(ei.value)
    c = ctx.sim_decode(hdr["snr"])
    assert (c["err_bit"], c["err_blk"], c["tot_bit"], c["tot_blk"]) == golden


def test_refusals(env, monkeypatch):
    """Host-side refusals (nothing is launched), each followed by a plain decode
    that still reproduces the golden counters on the same context."""
    hdr, fr, gold = _golden_plain(env, "peg2304_qpsk_known", 48)
    mk = lambda **kw: env.ctx(hdr["matrix"], hdr["modem"], False, hdr["max_iter"], **kw)
    ctx = mk()
    with monkeypatch.context() as m:
        m.setenv("KML_BP_KERNEL", "generic")
        _refused_then_plain(ctx, hdr, fr, gold, "generic")
    ctx.set_precision("f32")
    try:
        uu, h, y = fr
        ctx.sim_load(hdr["snr"], uu, y, h)
        with pytest.raises(K.KmlError) as ei:
            ctx.sim_decode_profile(hdr["snr"])
        assert UNSUP in str(ei.value) and "f32" in str(ei.value)
    finally:
        ctx.set_precision("f64")
    c = ctx.sim_decode(hdr["snr"])
    assert (c["err_bit"], c["err_blk"], c["tot_bit"], c["tot_blk"]) == gold
    prof, _, cnt = ctx.sim_decode_profile(hdr["snr"])  # and the context still profiles
    assert cnt == c and int(prof[-1, 0]) == gold[0]
    _refused_then_plain(mk(metric_soft=True), hdr, fr, gold, "soft")
    # max_iter = 65
    c65 = env.ctx(hdr["matrix"], hdr["modem"], False, 65)
    c65.sim_load(hdr["snr"], *[fr[i] for i in (0, 2, 1)])
    with pytest.raises(K.KmlError) as ei:
        c65.sim_decode_profile(hdr["snr"])
    assert UNSUP in str(ei.value) and "64" in str(ei.value)
    # PEG8064: the partitioned cooperative kernel
    hdr8, fr8, gold8 = _golden_plain(env, "peg8064_qpsk_known", 16)
    c8 = env.ctx(hdr8["matrix"], hdr8["modem"], False, hdr8["max_iter"])
    _refused_then_plain(c8, hdr8, fr8, gold8, "bp_part_kernel")
    assert c8.bp_kernel() == "bp_part_kernel"


def test_empty_batch(env):
    ctx = env.ctx(PEG, QPSK, False, 8)
    ctx.sim_load(2.0, np.zeros((0, ctx.K), np.uint8), np.zeros((0, ctx.S, 2)), np.zeros((0, 2)))
    prof, cwp, cnt = ctx.sim_decode_profile(2.0)
    assert prof.shape == (8, 3) and not prof.any() and cwp.shape == (0, 8) and not any(cnt.values())
