"""The near-one reciprocal as one fma (bp_common.hpp rcp_near1 = fma(X2, Y, -s),
tests/test_rcp_near1_model.py is its exact host model) on the device:

* the div probe on every double s with |s - 1| <= 2^-40, with numerators at the
  values BP saturates to (ProbClip's 1e-12 and 1 - 1e-12, and the tie 0.5);
* bp_regular_kernel, the kernel with the most near-one sites (27 per lane and
  iteration), on 32 PEG2304 + QPSK known-channel codewords at 2 dB against the
  oracle, bit for bit: with and without syndrome output (the SYN instances),
  from priors and through the fused-demap launch (the production instance), at
  budgets 2 and 20.  One codeword is one workgroup, the kernel's smallest shape.
"""
import os

import numpy as np
import pytest

from oracle import oracle as O

import kmldpc_amd as K

pytestmark = pytest.mark.gpu

MATRIX, MODEM = "PEG2304regular0.5.txt", "2bits_QPSK.txt"
SNR = 2.0
NCW = 32
BUDGETS = [2, 20]


def near_one_sums():
    j = np.arange(0, 2 ** 12 + 1, dtype=np.float64)
    k = np.arange(1, 2 ** 13 + 1, dtype=np.float64)
    s = np.concatenate([1.0 + j * 2.0 ** -52, 1.0 - k * 2.0 ** -53])
    assert s.size == 12289 and np.unique(s).size == s.size and np.all(np.abs(s - 1.0) <= 2.0 ** -40)
    return s


@pytest.fixture(scope="module")
def env(data_dir):
    mk = lambda it: K.Context(matrix_file=os.path.join(data_dir, MATRIX), modem_file=os.path.join(data_dir, MODEM),
                              max_iter=it, device=0)
    ctx = {it: mk(it) for it in BUDGETS}
    oc = {it: O.Code(os.path.join(data_dir, MATRIX), False, True, False, it) for it in BUDGETS}
    om = O.Modem(os.path.join(data_dir, MODEM))
    uu, cc, th, y = O.gen_frames(oc[20], om, SNR, NCW, state=41)
    var = 10.0 ** (-0.1 * SNR)
    p0 = np.stack([om.demap(y[i], th[i], var) for i in range(NCW)])
    # the oracle's decodes, once: [(ret, uu_hat, cc_hat, syn)] per budget
    ref = {it: [oc[20].bp_decode(p0[i], it) for i in range(NCW)] for it in BUDGETS}
    yield dict(ctx=ctx, oc=oc, om=om, frames=(uu, cc, th, y), p0=p0, ref=ref)
    for c in ctx.values():
        c.close()


@pytest.mark.parametrize("num", ["1e-12", "0.5", "1-1e-12"])
def test_probe_every_near_one_sum(env, num):
    """Column 6 is rcp_near1(s), columns 4 and 5 the CN division (n, s - n) / s."""
    s = near_one_sums()
    n = {"1e-12": 1e-12, "0.5": 0.5, "1-1e-12": 1.0 - 1e-12}[num] * s
    x = np.stack([n, s - n, s], axis=1)
    out = env["ctx"][20].div_probe(x)
    bad = out[:, 6] != 1.0 / s
    print(f"n = {num} s: rcp_near1 != 1/s on {int(bad.sum())} of {s.size}")
    assert np.array_equal(out[:, 6], 1.0 / s), s[bad][:4]
    for col, v in ((4, x[:, 0]), (5, x[:, 1])):
        bad = out[:, col] != v / s
        print(f"n = {num} s: column {col} != n / s on {int(bad.sum())} of {s.size}")
        assert np.array_equal(out[:, col], v / s), (s[bad][:4], v[bad][:4])


@pytest.mark.parametrize("it", BUDGETS)
def test_decode_from_priors_matches_oracle(env, it):
    """ret (the iterations run), uu_hat, cc_hat without syndrome output and
    with it, and the syndromes."""
    ctx, p0, ref = env["ctx"][20], env["p0"], env["ref"][it]
    plain = ctx.bp_decode(p0, iter_count=it, cc_hat=True)
    assert ctx.bp_kernel() == "bp_regular_kernel"
    withsyn = ctx.bp_decode(p0, iter_count=it, cc_hat=True, syn=np.zeros((NCW, ctx.M)))
    assert ctx.bp_kernel() == "bp_regular_kernel"
    for i in range(NCW):
        ret, uh, cch, syn = ref[i]
        for r in (plain, withsyn):
            assert r["ret"][i] == ret, (it, i)
            assert np.array_equal(r["uu_hat"][i], uh), (it, i)
            assert np.array_equal(r["cc_hat"][i], cch), (it, i)
        assert np.array_equal(withsyn["syn"][i], syn, equal_nan=True), (it, i)
    rets = np.array([r[0] for r in ref])
    if it == 20:  # early convergence and exhausted budgets in one batch
        conv = np.array([env["oc"][20].parity_count(r[2]) == 0 for r in ref])
        assert conv.any() and not conv.all() and (rets[conv] < 20).any()


@pytest.mark.parametrize("it", BUDGETS)
def test_fused_demap_launch_matches_oracle(env, it):
    """The production instance (fused demap, no syndromes) at a configured
    max_iter: ret and uu_hat, and the iteration counters of the resident batch
    (a codeword that converged at iteration i ran i + 1 VN and i CN phases)."""
    ctx, oc, om = env["ctx"][it], env["oc"][it], env["om"]
    uu, cc, th, y = env["frames"]
    r = ctx.decode_frames(y, SNR, th)
    assert ctx.bp_kernel() == "bp_regular_kernel"
    vn = cn = nconv = 0
    err = np.zeros(NCW, np.int64)
    for i in range(NCW):
        o = O.receive(oc, om, y[i], th[i], SNR, False)
        ret, uh, cch, _ = oc.bp_decode(o["p0"])
        assert o["ret"] == ret and np.array_equal(o["uu_hat"], uh)
        assert r["ret"][i] == ret, (it, i)
        assert np.array_equal(r["uu_hat"][i], uh), (it, i)
        conv = oc.parity_count(cch) == 0
        iters = ret - 1 if conv else ret
        assert conv or iters == it
        vn += iters + 1 if conv else iters
        cn += iters
        nconv += int(conv)
        err[i] = (uh != uu[i]).sum()
    ctx.sim_load(SNR, uu.astype(np.uint8), y, th)
    cw_err, _, c = ctx.sim_decode_ex(SNR, blind=False)
    assert np.array_equal(cw_err, err)
    assert (c["vn_phases"], c["cn_phases"], c["converged"]) == (vn, cn, nconv)
    assert c["redone"] == 0 and c["tot_blk"] == NCW
