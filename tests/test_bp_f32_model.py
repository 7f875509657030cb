"""The arithmetic contract of the single-precision BP mode (KML_PREC_F32), as a
numpy model, and its agreement with the reference arithmetic (the oracle).

bp_model() restates lab::BinaryLDPCCodec::Decoder (binaryldpccodec.cc:165-278,
oracle.c orc_bp_decode) for a regular code, vectorised over codewords, in the
reference's operation order:

  * the prior pair is (P0, 1 - P0) formed in float64 and each member cast to
    the working dtype;
  * VN phase per column, edges in column order: forward chain
    alpha <- (alpha0 c2v0, alpha1 c2v1) / sum, hard decision alpha0 > alpha1 ? 0 : 1
    on the last normalised alpha, backward chain from beta = (1, 1) giving
    v2c = alpha_k beta / sum;
  * early stop when every check row of the decisions has even parity, before
    the CN phase;
  * CN phase per row: forward trellis from (1, 0), backward trellis from (1, 0),
    c2v0 = clip(t0 / (t0 + t1)) with the clip constants cast to the working
    dtype (float32: 1e-12f and (float)(1 - 1e-12) = 1.0f), c2v1 = 1 - c2v0,
    syndrom_soft = the forward state past the row's last edge;
  * return value iter + (iter < max_iter).

Every value is of the working dtype.  A normalisation (n0, n1) / s is either
the IEEE quotient ("ieee") or n * r with r a reciprocal of s that is off by up
to one ulp ("rcp": RN(1 / s) moved by -1, 0 or +1 ulp, seeded) — harsher than
the GPU kernel's v_rcp_f32, which is within one ulp of 1 / s.

With float64 and "ieee" the model is the oracle, bit for bit; that is what makes
its float32 runs a statement about precision alone.  The GPU kernel
(kmldpc_amd/csrc/bp_regular_f32.hip) follows the same contract and is held to
the same 2 % cap (tests/test_gpu_f32.py).
"""
import os

import numpy as np
import pytest

from oracle import oracle as O

MATRIX = "PEG2304regular0.5.txt"
R1147 = "syn_reg36_2304_r1147.txt"  # the other PEG2304-class code: rank 1147, K = 1157 (tests/golden/make_codes.py)
# (modem file, snr): the three streams of the f32 mode's acceptance checks, and
# one on the rank-1147 code (QPSK at 4 dB: 0.43 of its codewords fail)
STREAMS = {
    "qpsk": ("2bits_QPSK.txt", 2.0),
    "16qam": ("4bit_16QAM_Gray.txt", 8.0),
    "64qam": ("6bits_64QAM_Gray.txt", 13.0),
    "r1147_qpsk": ("2bits_QPSK.txt", 4.0),
}
STREAM_MATRIX = {"r1147_qpsk": R1147}  # every other stream is on MATRIX
CAP = 0.02        # share of codewords that may differ from the oracle (a condition, not a measurement)
MIN_SHARE = 0.25  # each stream holds at least this share of converged and of failed codewords


class Graph:
    def __init__(self, oc):
        rp, rc, cp, cs = oc.graph()
        self.M, self.N, self.K, self.E, self.chk = oc.M, oc.N, oc.K, oc.E, oc.chk
        dv = np.diff(cp)
        dc = np.diff(rp)
        assert dv.min() == dv.max() and dc.min() == dc.max(), "the model is written for regular codes"
        self.dv, self.dc = int(dv[0]), int(dc[0])
        self.col_edge = cs.reshape(self.N, self.dv)    # edge (row-major index) of column v's k-th entry
        self.row_col = rc.reshape(self.M, self.dc)     # column of row r's j-th edge (edges r*dc + j)


def _normaliser(dt, division, seed):
    one = dt(1.0)
    if division == "ieee":
        return lambda n0, n1: (n0 / (n0 + n1), n1 / (n0 + n1))
    assert division == "rcp"
    rng = np.random.default_rng(seed)
    bits = np.int32 if dt is np.float32 else np.int64

    def norm(n0, n1):
        s = n0 + n1
        r = one / s
        # one ulp down, none or one ulp up: neighbours of a positive finite float are its bit pattern -+ 1
        step = rng.integers(-1, 2, size=s.shape, dtype=bits)
        moved = (r.view(bits) + step).view(r.dtype)
        r = np.where(np.isfinite(r) & (r > 0), moved, r)
        return n0 * r, n1 * r
    return norm


def bp_model(g, p0, iter_count, max_iter, dtype=np.float32, division="ieee", seed=1, syn_init=0.0):
    """Decode p0[B, N] (float64 P(bit = 0)); returns ret[B], uu_hat[B, K], cc_hat[B, N], syn[B, M] (float64).
    A codeword leaves the working set when it stops, so its outputs are what the reference's loop leaves."""
    dt = np.dtype(dtype).type
    norm = _normaliser(dt, division, seed)
    p0 = np.ascontiguousarray(p0, np.float64)
    B = p0.shape[0]
    one, half = dt(1.0), dt(0.5)
    lo, hi = dt(1.0e-12), dt(1.0 - 1.0e-12)
    cc_hat = np.zeros((B, g.N), np.uint8)
    syn = np.full((B, g.M), syn_init, np.float64)
    iters = np.full(B, iter_count, np.int64)
    live = np.arange(B)  # codewords still iterating; the arrays below hold their rows
    pa0 = p0.astype(dt)
    pa1 = (1.0 - p0).astype(dt)
    c2v0 = np.full((B, g.E), half, dt)
    c2v1 = np.full((B, g.E), half, dt)
    with np.errstate(all="ignore"):
        for it in range(iter_count):
            n = live.size
            # VN phase
            a0, a1 = pa0, pa1
            al0, al1 = [], []
            for k in range(g.dv):
                e = g.col_edge[:, k]
                al0.append(a0)
                al1.append(a1)
                a0, a1 = norm(a0 * c2v0[:, e], a1 * c2v1[:, e])
            hard = np.where(a0 > a1, 0, 1).astype(np.uint8)
            cc_hat[live] = hard
            v2c0 = np.empty((n, g.E), dt)
            v2c1 = np.empty((n, g.E), dt)
            b0 = np.full((n, g.N), one, dt)
            b1 = np.full((n, g.N), one, dt)
            for k in range(g.dv - 1, -1, -1):
                e = g.col_edge[:, k]
                v2c0[:, e], v2c1[:, e] = norm(al0[k] * b0, al1[k] * b1)
                b0, b1 = norm(b0 * c2v0[:, e], b1 * c2v1[:, e])
            # early stop
            ok = ~np.bitwise_xor.reduce(hard[:, g.row_col], axis=2).any(axis=1)
            iters[live[ok]] = it
            keep = ~ok
            live = live[keep]
            if live.size == 0:
                break
            pa0, pa1, v2c0, v2c1 = pa0[keep], pa1[keep], v2c0[keep], v2c1[keep]
            n = live.size
            # CN phase
            x0 = v2c0.reshape(n, g.M, g.dc)
            x1 = v2c1.reshape(n, g.M, g.dc)
            a0 = np.full((n, g.M), one, dt)
            a1 = np.zeros((n, g.M), dt)
            al0, al1 = [], []
            for j in range(g.dc):
                al0.append(a0)
                al1.append(a1)
                a0, a1 = norm(a0 * x0[:, :, j] + a1 * x1[:, :, j], a0 * x1[:, :, j] + a1 * x0[:, :, j])
            b0 = np.full((n, g.M), one, dt)
            b1 = np.zeros((n, g.M), dt)
            q0 = np.empty((n, g.M, g.dc), dt)
            q1 = np.empty((n, g.M, g.dc), dt)
            for j in range(g.dc - 1, -1, -1):
                q, _ = norm(al0[j] * b0 + al1[j] * b1, al0[j] * b1 + al1[j] * b0)
                q = np.where(q > hi, hi, q)
                q = np.where(q < lo, lo, q)
                q0[:, :, j] = q
                q1[:, :, j] = one - q
                b0, b1 = norm(b0 * x0[:, :, j] + b1 * x1[:, :, j], b0 * x1[:, :, j] + b1 * x0[:, :, j])
            c2v0 = q0.reshape(n, g.E)
            c2v1 = q1.reshape(n, g.E)
            syn[live] = a0.astype(np.float64)
    ret = (iters + (iters < max_iter)).astype(np.int32)
    uu_hat = cc_hat[:, g.chk:g.chk + g.K].copy()
    return ret, uu_hat, cc_hat, syn


# ---- the streams, generated and oracle-decoded once per session ------------

_cache = {}


def oracle_code(data_dir, max_iter=20, name="qpsk"):
    """The oracle's code and its graph for a stream's matrix."""
    matrix = STREAM_MATRIX.get(name, MATRIX)
    key = ("code", data_dir, max_iter, matrix)
    if key not in _cache:
        oc = O.Code(os.path.join(data_dir, matrix), False, True, False, max_iter)
        _cache[key] = (oc, Graph(oc))
    return _cache[key]


def stream(data_dir, name, n):
    """The first n seed-17 codewords of a stream: frames and the oracle's P0 (read-only, made once)."""
    key = ("stream", data_dir, name, n)
    if key not in _cache:
        modem, snr = STREAMS[name]
        oc, _ = oracle_code(data_dir, name=name)
        om = O.Modem(os.path.join(data_dir, modem))
        uu, cc, th, y = O.gen_frames(oc, om, snr, n)
        var = 10.0 ** (-0.1 * snr)
        p0 = np.stack([om.demap(y[i], th[i], var) for i in range(n)])
        for a in (uu, th, y, p0):
            a.setflags(write=False)
        _cache[key] = dict(uu=uu, th=th, y=y, p0=p0, snr=snr, modem=modem)
    return _cache[key]


SYN_FILL = -1.0  # what a never-written syndrome row reads as, in the oracle's runs and the others'


def oracle_decode(data_dir, name, n, iter_count=20):
    """The oracle's decode of those n codewords at a budget (read-only, made once)."""
    key = ("dec", data_dir, name, n, iter_count)
    if key not in _cache:
        oc, _ = oracle_code(data_dir, name=name)
        p0 = stream(data_dir, name, n)["p0"]
        ret = np.zeros(n, np.int32)
        uh = np.zeros((n, oc.K), np.uint8)
        cch = np.zeros((n, oc.N), np.uint8)
        syn = np.full((n, oc.M), SYN_FILL)
        for i in range(n):
            ret[i], uh[i], cch[i], syn[i] = oc.bp_decode(p0[i], iter_count, syn=syn[i].copy())
        for a in (ret, uh, cch, syn):
            a.setflags(write=False)
        _cache[key] = dict(ret=ret, uu_hat=uh, cc_hat=cch, syn=syn)
    return _cache[key]


def assert_both_outcomes(ret, max_iter=20):
    """At least MIN_SHARE of the codewords converged and at least MIN_SHARE failed (full budget)."""
    failed = np.mean(ret == max_iter)
    assert failed >= MIN_SHARE and 1.0 - failed >= MIN_SHARE, f"stream is one-sided: {failed:.3f} failed"


def differing(a, b):
    """Per-codeword flags: any element of the row differs."""
    a, b = np.asarray(a), np.asarray(b)
    return (a != b).reshape(a.shape[0], -1).any(axis=1)


# ---- tests -----------------------------------------------------------------

def test_float64_model_is_the_oracle(data_dir):
    _float64_model_is_the_oracle(data_dir, "qpsk", 256)


def test_float64_model_is_the_oracle_at_rank_1147(data_dir):
    """The same on the rank-1147 graph: uu_hat = cc_hat[chk : chk + K] with chk = 1147, K = 1157."""
    _float64_model_is_the_oracle(data_dir, "r1147_qpsk", 192)


def _float64_model_is_the_oracle(data_dir, name, n_stream):
    oc, g = oracle_code(data_dir, name=name)
    n = 128
    p0 = stream(data_dir, name, n_stream)["p0"][:n]  # (the stream is shared with the float32 test)
    ref = oracle_decode(data_dir, name, n_stream)
    assert_both_outcomes(ref["ret"][:n])
    ret, uh, cch, syn = bp_model(g, p0, 20, 20, np.float64, "ieee", syn_init=SYN_FILL)
    assert np.array_equal(ret, ref["ret"][:n])
    assert np.array_equal(uh, ref["uu_hat"][:n])
    assert np.array_equal(cch, ref["cc_hat"][:n])
    assert np.array_equal(syn, ref["syn"][:n])


@pytest.mark.parametrize("division", ["ieee", "rcp"])
@pytest.mark.parametrize("name,n", [("qpsk", 256), ("16qam", 128), ("64qam", 128), ("r1147_qpsk", 192)])
def test_float32_model_within_cap(data_dir, name, n, division):
    oc, g = oracle_code(data_dir, name=name)
    p0 = stream(data_dir, name, n)["p0"]
    ref = oracle_decode(data_dir, name, n)
    assert_both_outcomes(ref["ret"])
    ret, uh, cch, syn = bp_model(g, p0, 20, 20, np.float32, division, seed=7)
    bad = differing(uh, ref["uu_hat"]) | (ret != ref["ret"])
    print(f"{name} {division}: {int(bad.sum())} of {n} codewords differ in uu_hat or ret")
    assert bad.mean() <= CAP


def model_syn_delta(data_dir, name, n, iter_count):
    """max |syn(float32 ieee model) - syn(oracle)| over the codewords whose ret agrees."""
    oc, g = oracle_code(data_dir, name=name)
    ref = oracle_decode(data_dir, name, n, iter_count)
    ret, _, _, syn = bp_model(g, stream(data_dir, name, n)["p0"], iter_count, 20, np.float32, "ieee",
                              syn_init=SYN_FILL)
    same = ret == ref["ret"]
    return float(np.max(np.abs(syn[same] - ref["syn"][same]))), int(same.sum())
