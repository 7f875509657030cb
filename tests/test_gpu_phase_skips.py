"""The two BP phases bp_regular_kernel no longer computes (bp_regular.hip):
the VN phase of iteration 0 in closed form on the FAST path
(every v2c is the prior pair, tests/test_iter0_model.py)
and the budget's last CN phase reduced to its parity check when no syndromes
are asked for.  Every output stays the reference's bit
for bit: PEG2304 + QPSK (N = 2304 is the only shape this kernel takes), and the
rank-1147 code of the same shape (K = 1157, chk = 1147: a partial last word of
decoded bits and another graph; the r1147 cases), against
the oracle's BP decode of the same priors and the oracle's receive path, with
iteration budgets that put the shortcuts in the same, in neighbouring and in
distant iterations, with and without syndrome output, on the FAST path, through
forced redos and on the exact path.
"""
import math
import os

import numpy as np
import pytest

from oracle import oracle as O

import kmldpc_amd as K

pytestmark = pytest.mark.gpu

MATRIX, MODEM = "PEG2304regular0.5.txt", "2bits_QPSK.txt"
R1147 = "syn_reg36_2304_r1147.txt"  # tests/golden/make_codes.py
SNR = 2.0  # the headline workload's Es/N0
MODES = ["fast", "KML_FORCE_REDO", "KML_NO_FAST"]
BUDGETS = [1, 2, 20]
LO = math.ldexp(1.0, 40 * 3 - 960)  # bp_common.hpp fast_prior_lo(dv = 3)


class Env:
    def __init__(self, data_dir, matrix=MATRIX):
        mk = lambda it: K.Context(matrix_file=os.path.join(data_dir, matrix), modem_file=os.path.join(data_dir, MODEM),
                                  max_iter=it, device=0)
        self.ctx = {20: mk(20), 1: mk(1)}
        self.oc = {it: O.Code(os.path.join(data_dir, matrix), False, True, False, it) for it in (20, 1)}
        self.om = O.Modem(os.path.join(data_dir, MODEM))
        self._batches = {}
        self._ref = {}
        self._rx = {}

    def frames(self, snr, n, state):
        return O.gen_frames(self.oc[20], self.om, snr, n, state=state)

    def priors(self, snr, n, state):
        uu, cc, th, y = self.frames(snr, n, state)
        var = 10.0 ** (-0.1 * snr)
        return np.stack([self.om.demap(y[i], th[i], var) for i in range(n)])

    def batch(self, name):
        if name not in self._batches:
            self._batches[name] = getattr(self, "_make_" + name)()
        return self._batches[name]

    def _make_noisy(self):  # 2 dB: early convergence and exhausted budgets in one batch
        return self.priors(SNR, 64, 31)

    def _make_clean(self):  # noise-free: converged at iteration 0
        return self.priors(60.0, 8, 32)

    def _make_adversarial(self):
        """Ordinary 2 dB codewords with columns at the closed form's edges: the
        tie 0.5 (decision 1) and its neighbours, exactly +0 and 1, and the FAST
        domain's boundary lo / 1 - lo (1 - 2^-840 rounds to 1; the largest
        double below 1 stands beside it)."""
        p0 = self.priors(SNR, 32, 33)
        rng = np.random.default_rng(34)
        ties = [0.5, math.nextafter(0.5, 0.0), math.nextafter(0.5, 1.0)]
        low = [0.0, LO, math.nextafter(LO, 1.0)]
        high = [1.0, 1.0 - LO, math.nextafter(1.0, 0.0)]
        for b in range(p0.shape[0]):
            cols = rng.choice(p0.shape[1], 90, replace=False)
            for j, c in enumerate(cols):
                k = (b + j) % 6
                # the saturated values sit on the column's own side, so frames still
                # converge; codeword 6 has them on the wrong side
                side = (p0[b, c] > 0.5) != (b == 6)
                p0[b, c] = ties[k] if k < 3 else (high if side else low)[k - 3]
        p0[5, :] = 0.5  # every column a tie
        return p0

    def _make_mixed(self):
        """Some codewords carry one prior below lo (but > 0): they go to the
        exact kernel while their neighbours take the FAST path."""
        p0 = self.priors(SNR, 32, 35).copy()
        for b, (col, v) in {3: (17, math.ldexp(1.0, -900)), 10: (2303, 5e-320), 11: (0, math.ldexp(1.5, -841)),
                            31: (1152, math.ldexp(1.0, -1000))}.items():
            assert 0.0 < v < LO
            p0[b, col] = v
        return p0

    def ref(self, name, it):
        """The oracle's decode of a batch at a budget, once: [(ret, uu_hat, cc_hat, syn)]"""
        if (name, it) not in self._ref:
            p0 = self.batch(name)
            self._ref[(name, it)] = [self.oc[20].bp_decode(p0[i], it) for i in range(p0.shape[0])]
        return self._ref[(name, it)]

    def rx(self, max_iter):
        """64 known-H frames at 2 dB and the oracle's receive path + decode at a
        configured max_iter, once."""
        if max_iter not in self._rx:
            if "frames" not in self._rx:
                self._rx["frames"] = self.frames(SNR, 64, 36)
            uu, cc, th, y = self._rx["frames"]
            oc = self.oc[max_iter]
            out = []
            for i in range(64):
                r = O.receive(oc, self.om, y[i], th[i], SNR, False)
                ret, uh, cch, _ = oc.bp_decode(r["p0"])
                assert ret == r["ret"] and np.array_equal(uh, r["uu_hat"])
                out.append(dict(ret=ret, uu_hat=uh, conv=oc.parity_count(cch) == 0))
            self._rx[max_iter] = out
        return self._rx["frames"], self._rx[max_iter]

    def close(self):
        for c in self.ctx.values():
            c.close()


@pytest.fixture(scope="module")
def envs(data_dir):
    """One Env per code, made when a case first asks for it."""
    made = {}

    def get(code):
        if code not in made:
            made[code] = Env(data_dir, {"peg": MATRIX, "r1147": R1147}[code])
        return made[code]
    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def env(envs):
    return envs("peg")


def _set_mode(monkeypatch, mode):
    if mode != "fast":
        monkeypatch.setenv(mode, "1")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("it", BUDGETS)
@pytest.mark.parametrize("name", ["noisy", "clean", "adversarial", "mixed",
                                  "r1147_noisy", "r1147_clean", "r1147_adversarial", "r1147_mixed"])
def test_bp_decode_matches_oracle(envs, monkeypatch, name, it, mode):
    """ret, uu_hat, cc_hat bit for bit without syndrome output (the last CN
    phase is the parity check alone) and with it (the last CN phase still
    writes the reference's syndromes).  Budget 1 puts both shortcuts in the
    same iteration."""
    _set_mode(monkeypatch, mode)
    env = envs("r1147" if name.startswith("r1147_") else "peg")
    name = name.removeprefix("r1147_")
    ctx = env.ctx[20]
    p0 = env.batch(name)
    B = p0.shape[0]
    assert B <= 64
    ref = env.ref(name, it)
    plain = ctx.bp_decode(p0, iter_count=it, cc_hat=True)
    assert ctx.bp_kernel() == "bp_regular_kernel"
    withsyn = ctx.bp_decode(p0, iter_count=it, cc_hat=True, syn=np.zeros((B, ctx.M)))
    for i in range(B):
        ret, uh, cch, syn = ref[i]
        for r in (plain, withsyn):
            assert r["ret"][i] == ret, (name, it, i)
            assert np.array_equal(r["uu_hat"][i], uh), (name, it, i)
            assert np.array_equal(r["cc_hat"][i], cch), (name, it, i)
        assert np.array_equal(withsyn["syn"][i], syn, equal_nan=True), (name, it, i)
    rets = np.array([r[0] for r in ref])
    if name == "clean":
        assert (rets == 1).all()  # converged at iteration 0
    if name == "noisy" and it == 20:  # the batch mixes early convergence and exhausted budgets
        conv = np.array([env.oc[20].parity_count(r[2]) == 0 for r in ref])
        assert conv.any() and not conv.all() and (rets[conv] < 20).any()


@pytest.mark.parametrize("mode", MODES)
def test_noise_free_frames_count_no_cn_phase(env, monkeypatch, mode):
    """Frames that converge at iteration 0 count one VN phase and no CN phase
    each (the speculative CN phase of a converged codeword is discarded)."""
    _set_mode(monkeypatch, mode)
    ctx = env.ctx[20]
    uu, cc, th, y = env.frames(60.0, 16, 37)
    r = ctx.decode_frames(y, 60.0, th)
    assert (r["ret"] == 1).all() and np.array_equal(r["uu_hat"], uu.astype(np.uint8))
    ctx.sim_load(60.0, uu.astype(np.uint8), y, th)
    errs, _, c = ctx.sim_decode_ex(60.0, blind=False)
    assert c["cn_phases"] == 0 and c["vn_phases"] == 16 and c["converged"] == 16
    assert c["err_bit"] == 0 and c["tot_blk"] == 16 and not errs.any()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("code,max_iter", [pytest.param("peg", 20, id="20"), pytest.param("peg", 1, id="1"),
                                           pytest.param("r1147", 20, id="r1147-20"),
                                           pytest.param("r1147", 1, id="r1147-1")])
def test_fused_demap_path_and_counters(envs, monkeypatch, code, max_iter, mode):
    """Known-H frames through the fused-demap launch (SYN = false, the headline
    kernel) at the configured max_iter and with a context configured for
    max_iter = 1, against the oracle's receive path; and the resident-batch
    counters against counts derived from the oracle's return values.  With
    iter the iterations run, ret = iter + (iter < max_iter); a codeword that
    converged at iteration i ran i + 1 VN and i CN phases, ret = i + 1; one that
    exhausted the budget ran max_iter of each, ret = max_iter.  ret = max_iter
    is both "converged at the last iteration" and "exhausted": the parity of the
    oracle's final decisions tells them apart."""
    _set_mode(monkeypatch, mode)
    env = envs(code)
    ctx = env.ctx[max_iter]
    assert (ctx.K, ctx.chk) == ((1157, 1147) if code == "r1147" else (1152, 1152))
    (uu, cc, th, y), ref = env.rx(max_iter)
    r = ctx.decode_frames(y, SNR, th)
    assert ctx.bp_kernel() == "bp_regular_kernel"
    for i in range(64):
        assert r["ret"][i] == ref[i]["ret"], i
        assert np.array_equal(r["uu_hat"][i], ref[i]["uu_hat"]), i
    vn = cn = conv = 0
    for d in ref:
        iters = d["ret"] - 1 if d["conv"] else d["ret"]
        assert iters == max_iter or d["conv"]
        vn += iters + 1 if d["conv"] else iters
        cn += iters
        conv += int(d["conv"])
    err = np.array([(ref[i]["uu_hat"] != uu[i]).sum() for i in range(64)])
    ctx.sim_load(SNR, uu.astype(np.uint8), y, th)
    cw_err, _, c = ctx.sim_decode_ex(SNR, blind=False)
    assert np.array_equal(cw_err, err)
    assert (c["vn_phases"], c["cn_phases"], c["converged"]) == (vn, cn, conv)
    assert c["err_bit"] == int(err.sum()) and c["err_blk"] == int((err > 0).sum()) and c["tot_blk"] == 64
    assert c["redone"] == (64 if mode == "KML_FORCE_REDO" else 0)
    if max_iter == 20:
        assert 0 < conv < 64  # early convergence and exhausted budgets in one batch
