"""The budget's last iteration of bp_regular_kernel without syndrome output
(bp_regular.hip): peeled out of the iteration loop, its VN phase the forward
chain and the decisions alone, its CN phase the parity check.

Every output stays the reference's: PEG2304 + QPSK (the only shape the kernel
takes) against the oracle's BP decode of the same priors and the oracle's
receive path, never against the library itself.  tests/test_gpu_phase_skips.py
covers budgets 1, 2 and 20; here budget 3 (one generic iteration between the
closed form and the peeled one), the iteration profile at max_iter 3, and the
fused-demap launch at batch sizes around the CU count (a workgroup that takes
no, one, two and several codewords), with every codeword deferred, and with
one codeword in the middle of the batch deferred alone.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

from oracle import oracle as O

import kmldpc_amd as K

pytestmark = pytest.mark.gpu

MATRIX, MODEM = "PEG2304regular0.5.txt", "2bits_QPSK.txt"
SNR = 2.0  # the headline workload's Es/N0
MODES = ["fast", "KML_FORCE_REDO", "KML_NO_FAST"]
P = 3  # the budget of every case here
# hipDeviceAttributeMultiprocessorCount (hip_runtime_api.h, hipDeviceAttribute_t; ROCm 6 and 7: 63).  ctypes
# cannot see the enum, so the value is restated here and the result checked for plausibility in _cus().
HIP_ATTR_MULTIPROCESSOR_COUNT = 63


def _cus():
    """The device's CU count (one persistent workgroup each), from the HIP runtime
    the library is linked against (dlsym through the library's handle)."""
    n = C.c_int(0)
    fn = K.lib().hipDeviceGetAttribute
    fn.argtypes = [C.POINTER(C.c_int), C.c_int, C.c_int]
    assert fn(C.byref(n), HIP_ATTR_MULTIPROCESSOR_COUNT, 0) == 0
    # a renumbered enum would return another attribute: CDNA parts have 64 ... 304 CUs, in multiples of 4
    assert 64 <= n.value <= 304 and n.value % 4 == 0, n.value
    return n.value


class Env:
    def __init__(self, data_dir):
        mk = lambda it: K.Context(matrix_file=os.path.join(data_dir, MATRIX), modem_file=os.path.join(data_dir, MODEM),
                                  max_iter=it, device=0)
        self.ctx = {20: mk(20), P: mk(P)}
        self.oc = O.Code(os.path.join(data_dir, MATRIX), False, True, False, P)
        self.oc20 = O.Code(os.path.join(data_dir, MATRIX), False, True, False, 20)  # ret counts against max_iter
        self.om = O.Modem(os.path.join(data_dir, MODEM))
        self._cache = {}

    def once(self, key, make):
        if key not in self._cache:
            self._cache[key] = make()
        return self._cache[key]

    def priors(self, n, state):
        uu, cc, th, y = O.gen_frames(self.oc, self.om, SNR, n, state=state)
        var = 10.0 ** (-0.1 * SNR)
        return np.stack([self.om.demap(y[i], th[i], var) for i in range(n)])

    def batch(self, name):
        return self.once(("batch", name), getattr(self, "_make_" + name))

    def _make_noisy(self):  # 2 dB: converged at iterations 1, 2 and exhausted budgets
        return self.priors(64, 41)

    def _make_ties(self):
        """2 dB codewords with scattered columns at the tie 0.5 and its two
        neighbours; codeword 5 with every prior 0.5 (every message stays exactly
        0.5 and every decision is the tie's 1: the all-ones word, which passes
        the degree-6 checks at iteration 0); and codeword 6 with the prior 0.5
        on the support of another codeword: a codeword meets every row in an
        even number of columns, so each of those columns shares each of its
        rows with another one, every message into them stays exactly 0.5, and
        their ties persist into the last iteration while the noisy rest of the
        frame, which those rows tell nothing, keeps the parity check failing."""
        uu, cc, th, y = O.gen_frames(self.oc, self.om, SNR, 32, state=42)
        var = 10.0 ** (-0.1 * SNR)
        p0 = np.stack([self.om.demap(y[i], th[i], var) for i in range(32)])
        self.tie_support = cc[7].astype(bool)
        rng = np.random.default_rng(43)
        ties = [0.5, math.nextafter(0.5, 0.0), math.nextafter(0.5, 1.0)]
        for b in range(p0.shape[0]):
            cols = rng.choice(p0.shape[1], 90, replace=False)
            for j, c in enumerate(cols):
                p0[b, c] = ties[(b + j) % 3]
        p0[5, :] = 0.5
        p0[6, self.tie_support] = 0.5
        return p0

    def ref(self, name, it):
        """The oracle's decode of a batch at a budget, configured max_iter 20 like
        the context that decodes it, once: [(ret, uu_hat, cc_hat, syn)]"""
        p0 = self.batch(name)
        return self.once(("ref", name, it), lambda: [self.oc20.bp_decode(p0[i], it) for i in range(p0.shape[0])])

    def frames(self, n):
        """The first n of one stream of known-H frames at 2 dB, with the oracle's
        receive path at max_iter = P for each: ret, error bits, converged."""
        def make():
            nmax = 3 * _cus() + 5
            uu, cc, th, y = O.gen_frames(self.oc, self.om, SNR, nmax, state=44)
            return uu.astype(np.uint8), th, y, self.receive(uu, th, y)
        uu, th, y, rx = self.once("frames", make)
        return uu[:n], th[:n], y[:n], rx[:n]

    def receive(self, uu, th, y):
        out = []
        for i in range(uu.shape[0]):
            r = O.receive(self.oc, self.om, y[i], th[i], SNR, False)
            ret, uh, cch, _ = self.oc.bp_decode(r["p0"])
            assert ret == r["ret"] and np.array_equal(uh, r["uu_hat"])
            out.append(dict(ret=ret, uu_hat=uh, err=int((uh != uu[i]).sum()), conv=self.oc.parity_count(cch) == 0,
                            p0=r["p0"]))
        return out

    def close(self):
        for c in self.ctx.values():
            c.close()


@pytest.fixture(scope="module")
def env(data_dir):
    e = Env(data_dir)
    yield e
    e.close()


def _set_mode(monkeypatch, mode):
    if mode != "fast":
        monkeypatch.setenv(mode, "1")


def _counts(rx, max_iter):
    """The resident-batch counters from the oracle's results (the convention of
    test_gpu_phase_skips.test_fused_demap_path_and_counters)."""
    vn = cn = conv = 0
    for d in rx:
        iters = d["ret"] - 1 if d["conv"] else d["ret"]
        assert iters == max_iter or d["conv"]
        vn += iters + 1 if d["conv"] else iters
        cn += iters
        conv += int(d["conv"])
    err = np.array([d["err"] for d in rx])
    return dict(err_bit=int(err.sum()), err_blk=int((err > 0).sum()), tot_bit=len(rx) * 1152, tot_blk=len(rx),
                vn_phases=vn, cn_phases=cn, converged=conv), err


def _check_fused(env, uu, th, y, rx, redone):
    ctx = env.ctx[P]
    B = uu.shape[0]
    r = ctx.decode_frames(y, SNR, th)
    assert ctx.bp_kernel() == "bp_regular_kernel"
    assert np.array_equal(r["ret"], np.array([d["ret"] for d in rx]))
    assert np.array_equal(r["uu_hat"], np.stack([d["uu_hat"] for d in rx]))
    want, err = _counts(rx, P)
    ctx.sim_load(SNR, uu, y, th)
    cw_err, _, c = ctx.sim_decode_ex(SNR, blind=False)
    assert np.array_equal(cw_err, err)
    assert c == dict(want, redone=redone), (B, c, want)
    return cw_err, c


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["noisy", "ties"])
def test_budget_3_matches_oracle(env, monkeypatch, name, mode):
    """ret, uu_hat, cc_hat without syndrome output (closed form, one generic
    iteration, the peeled one) and with it (the loop alone), and syn."""
    _set_mode(monkeypatch, mode)
    ctx = env.ctx[20]
    p0 = env.batch(name)
    B = p0.shape[0]
    ref = env.ref(name, P)
    plain = ctx.bp_decode(p0, iter_count=P, cc_hat=True)
    assert ctx.bp_kernel() == "bp_regular_kernel"
    withsyn = ctx.bp_decode(p0, iter_count=P, cc_hat=True, syn=np.zeros((B, ctx.M)))
    for i in range(B):
        ret, uh, cch, syn = ref[i]
        for r in (plain, withsyn):
            assert r["ret"][i] == ret, (name, i)
            assert np.array_equal(r["uu_hat"][i], uh), (name, i)
            assert np.array_equal(r["cc_hat"][i], cch), (name, i)
        assert np.array_equal(withsyn["syn"][i], syn, equal_nan=True), (name, i)
    rets = np.array([r[0] for r in ref])
    if name == "noisy":  # the peeled iteration is both reached and not reached (ret = iter + 1 below max_iter)
        assert (rets < P).any() and (rets == P + 1).any()
    if name == "ties":
        assert rets[5] == 1 and ref[5][2].all()  # all ones at iteration 0
        assert rets[6] == P + 1 and ref[6][2][env.tie_support].all()  # ties into the last iteration


def test_iteration_profile_at_max_iter_3(env):
    """cw_prof and prof of one decode at max_iter 3 against the oracle's separate
    decodes at budgets 1, 2, 3 of the same priors."""
    ctx = env.ctx[P]
    uu, th, y, rx = env.frames(64)
    ctx.sim_load(SNR, uu, y, th)
    prof, cwp, cnt = ctx.sim_decode_profile(SNR, blind=False)
    assert ctx.bp_kernel() == "bp_regular_kernel"
    err = np.zeros((64, P), np.int32)
    conv = np.zeros((64, P), bool)
    for i in range(64):
        for k in range(1, P + 1):
            ret, uh, cch, _ = env.oc.bp_decode(rx[i]["p0"], k)
            err[i, k - 1] = (uh != uu[i]).sum()
            conv[i, k - 1] = env.oc.parity_count(cch) == 0
    assert np.array_equal(cwp, err)
    assert np.array_equal(prof[:, 0], err.sum(0).astype(np.uint64))
    assert np.array_equal(prof[:, 1], (err > 0).sum(0).astype(np.uint64))
    assert np.array_equal(prof[:, 2], conv.sum(0).astype(np.uint64))
    want, _ = _counts(rx, P)
    assert cnt == dict(want, redone=0)
    assert 0 < conv[:, P - 1].sum() < 64


def _batch_sizes():
    # one workgroup per CU: a batch of 1, of 2, below the CU count, one more
    # than the CU count (one workgroup takes a second codeword), 3 x + 5
    return ["1", "2", "below", "cus+1", "3cus+5"]


def _size(tag):
    cus = _cus()
    return {"1": 1, "2": 2, "below": max(cus - 3, 3), "cus+1": cus + 1, "3cus+5": 3 * cus + 5}[tag]


@pytest.mark.parametrize("tag", _batch_sizes())
def test_fused_path_batch_sizes(env, tag):
    """cw_err, ret, uu_hat and all counters of the fused-demap launch against
    the oracle's receive path."""
    B = _size(tag)
    assert B <= 773 or _cus() > 256
    uu, th, y, rx = env.frames(B)
    _check_fused(env, uu, th, y, rx, redone=0)


def test_fused_path_every_codeword_deferred(env, monkeypatch):
    monkeypatch.setenv("KML_FORCE_REDO", "1")
    B = _size("cus+1")
    uu, th, y, rx = env.frames(B)
    _check_fused(env, uu, th, y, rx, redone=B)


def test_fused_path_one_codeword_deferred_alone(env):
    """One frame in the middle of the batch has a symbol exactly on a
    constellation point (the squared distance is 0, so the FAST demap declines
    and the codeword goes to the exact kernel alone, while the FAST kernel
    takes its next queue entry without an epilogue).

    One statement of the issue was mended: it asks for `redone == 1` here.  The
    counter counts FAST decodes given up mid-decode for an unproven quotient
    (include/kmldpc_amd.h, kernels.hpp CNT_REDONE), not codewords the FAST
    kernel hands over before decoding them, in the parent commit as well: this
    batch gives redone == 0 there too, and counting hand-overs would change
    the counters of every workload.  What is asserted instead asks no less of
    the hand-off: the frame can only have been decoded by the exact kernel
    (demap_symbol_t<FAST> returns false for a squared distance of 0 before it
    writes a prior), its outputs, its neighbours' and every counter of the
    batch are the oracle's, and the counter keeps its documented value.  That
    the distance is exactly 0 is checked here in the demap's own IEEE
    operations (demap_common.hpp demap_symbol_t; the library is built with
    -ffp-contract=off, so the device rounds each product and difference as
    numpy does), against the domain's floor 2^-512 below which it declines."""
    B = _size("cus+1")
    uu, th, y, rx = env.frames(B)
    mid = B // 2
    y = y.copy()
    cr, ci = env.om.points[2], env.om.points[3]
    hr, hi = th[mid]
    y[mid, 7] = (cr * hr - ci * hi, cr * hi + ci * hr)  # the demap's own products and order
    # demap_symbol_t for point k = 1: sr = cr hr - ci hi - yr, si = cr hi + ci hr - yi, n = sr sr + si si
    f = np.float64
    sr = (f(cr) * f(hr) - f(ci) * f(hi)) - f(y[mid, 7, 0])
    si = (f(cr) * f(hi) + f(ci) * f(hr)) - f(y[mid, 7, 1])
    n = sr * sr + si * si
    assert n == 0.0 and not n >= math.ldexp(1.0, -512)  # nmin >= 2^-512 fails: the FAST demap returns false
    others = [abs(complex(env.om.points[2 * k], env.om.points[2 * k + 1]) * complex(hr, hi)
                  - complex(*y[mid, 7])) ** 2 for k in (0, 2, 3)]
    assert min(others) > 0.0  # (one point only)
    one = env.receive(uu[mid:mid + 1], th[mid:mid + 1], y[mid:mid + 1])  # the oracle decodes that frame
    rx = rx[:mid] + one + rx[mid + 1:]
    assert all(0.0 < p < 1.0 for p in one[0]["p0"][14:16])
    _check_fused(env, uu, th, y, rx, redone=0)


def test_same_resident_batch_twice(env):
    ctx = env.ctx[P]
    B = _size("cus+1")
    uu, th, y, rx = env.frames(B)
    ctx.sim_load(SNR, uu, y, th)
    e1, m1, c1 = ctx.sim_decode_ex(SNR, blind=False)
    e2, m2, c2 = ctx.sim_decode_ex(SNR, blind=False)
    assert np.array_equal(e1, e2) and np.array_equal(m1, m2, equal_nan=True) and c1 == c2
    want, err = _counts(rx, P)
    assert np.array_equal(e1, err) and c1 == dict(want, redone=0)
