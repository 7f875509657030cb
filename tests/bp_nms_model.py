"""The arithmetic contract of the normalized min-sum mode (KML_ALG_NMS,
include/kmldpc_amd.h), as a numpy model vectorised over codewords, for any
graph from oracle.Code.graph().  The GPU kernel
(kmldpc_amd/csrc/bp_irregular_nms.hip) equals it bit for bit
(tests/test_gpu_nms.py).

Every value is IEEE binary32 (numpy float32: denormals kept, no fma, each
operation rounded once):

  * prior: q = min(max(P0, 1e-12), 1 - 1e-12) in float64,
    L = float32(log(q) - log(1 - q)), the subtraction in float64, the logs by
    math.log, one call per value (glibc's correctly rounded log, which the
    device's kml_log restates); a punctured 5G column (v < N - cc_len) has
    L = +0; messages start at +0;
  * VN phase, column v, edges in column order (col_ptr / col_slot):
    t = L; t = t + c2v_k for each k in order; T = t; decision T > 0 ? 0 : 1;
    v2c_k = clamp(T - c2v_k, -256, 256);
  * stop: after the VN phase, when every check row's decisions have even parity,
    before the CN phase; ret = iter + (iter < max_iter); iter_count = 0 leaves
    the outputs as passed (here: zeros);
  * CN phase, row with incoming m_j: a_j = min over i != j of |m_i|,
    s_j = XOR over i != j of signbit(m_i) (-0 counts as negative),
    c2v_j = float32(alpha * a_j) with its sign bit set to s_j.
"""
import math

import numpy as np

CLAMP = np.float32(256.0)
PROB_LO = 1.0e-12
PROB_HI = 1.0 - 1.0e-12
DEFAULT_ALPHA = 0.75


class Graph:
    """The Tanner graph of an oracle.Code, any degrees."""

    def __init__(self, oc):
        rp, rc, cp, cs = oc.graph()
        self.M, self.N, self.K, self.E, self.cc_len = oc.M, oc.N, oc.K, oc.E, oc.cc_len
        self.punct = oc.N - oc.cc_len                 # leading punctured columns (5G: 2Z)
        self.info_off = 0 if oc.is5g else oc.chk      # uu_hat[i] = cc_hat[i + info_off]
        self.rp, self.rc, self.cp, self.cs = rp, rc, cp, cs
        dv = np.diff(cp)
        dc = np.diff(rp)
        self.dv_max, self.dc_max = int(dv.max()), int(dc.max())
        # VN step k: the columns of degree > k and the (row-major) edge of their k-th entry
        self.vn_steps = []
        for k in range(self.dv_max):
            cols = np.nonzero(dv > k)[0]
            self.vn_steps.append((cols, cs[cp[cols] + k]))
        # CN: rows grouped by degree; edges[r, j] = row r's j-th edge (row-major edges are contiguous per row)
        self.cn_groups = []
        for d in sorted(set(int(x) for x in dc)):
            rows = np.nonzero(dc == d)[0]
            self.cn_groups.append((d, rp[rows][:, None] + np.arange(d)[None, :]))
        self.row_start = rp[:-1].astype(np.intp)


def priors(g, p0):
    """float32 LLR priors [B, N] of p0[B, cc_len] (float64 P(bit = 0))."""
    p0 = np.ascontiguousarray(p0, np.float64).reshape(-1, g.cc_len)
    q = np.minimum(np.maximum(p0, PROB_LO), PROB_HI)
    llr = np.array([math.log(x) - math.log(1.0 - x) for x in q.ravel()], np.float64).reshape(q.shape)
    L = np.zeros((p0.shape[0], g.N), np.float32)
    L[:, g.punct:] = llr.astype(np.float32)
    return L


def _set_sign(mag, neg):
    """mag (float32, sign clear) with its sign bit set where neg."""
    return (mag.view(np.uint32) | (neg.astype(np.uint32) << np.uint32(31))).view(np.float32)


def cn_phase(g, v2c, alpha, reverse=False):
    """c2v[n, E] from v2c[n, E]; reverse = walk every row's edges in the opposite order."""
    a32 = np.float32(alpha)
    c2v = np.empty_like(v2c)
    mag = np.abs(v2c)
    neg = np.signbit(v2c)
    inf = np.float32(np.inf)
    for d, edges in g.cn_groups:
        order = range(d - 1, -1, -1) if reverse else range(d)
        x = mag[:, edges]      # [n, R, d]
        s = neg[:, edges]
        n, R = x.shape[0], x.shape[1]
        # running minimum / sign over the edges before j in walk order, then over those after j
        before_m, before_s = {}, {}
        rm = np.full((n, R), inf, np.float32)
        rs = np.zeros((n, R), bool)
        for j in order:
            before_m[j], before_s[j] = rm, rs
            rm = np.minimum(rm, x[:, :, j])
            rs = rs ^ s[:, :, j]
        rm = np.full((n, R), inf, np.float32)
        rs = np.zeros((n, R), bool)
        for j in reversed(order):
            a = np.minimum(before_m[j], rm)
            sg = before_s[j] ^ rs
            c2v[:, edges[:, j]] = _set_sign((a32 * a).astype(np.float32), sg)
            rm = np.minimum(rm, x[:, :, j])
            rs = rs ^ s[:, :, j]
    return c2v


def nms_model(g, p0, iter_count, max_iter, alpha=DEFAULT_ALPHA, reverse_rows=False, stats=None):
    """Decode p0[B, cc_len]; returns ret[B] int32, uu_hat[B, K], cc_hat[B, N] uint8.
    A codeword leaves the working set when it stops.  stats (a dict) receives
    max_abs_v2c, the largest |v2c| written, and finite, whether every message was finite."""
    L = priors(g, p0)
    B = L.shape[0]
    cc_hat = np.zeros((B, g.N), np.uint8)
    iters = np.full(B, iter_count, np.int64)
    live = np.arange(B)
    c2v = np.zeros((B, g.E), np.float32)
    top, finite = 0.0, True
    for it in range(iter_count):
        n = live.size
        t = L.copy()
        for cols, e in g.vn_steps:
            t[:, cols] = t[:, cols] + c2v[:, e]
        hard = np.where(t > 0, 0, 1).astype(np.uint8)
        cc_hat[live] = hard
        v2c = np.empty((n, g.E), np.float32)
        for cols, e in g.vn_steps:
            v2c[:, e] = np.minimum(np.maximum(t[:, cols] - c2v[:, e], -CLAMP), CLAMP)
        top = max(top, float(np.max(np.abs(v2c))))
        finite = finite and bool(np.isfinite(v2c).all() and np.isfinite(t).all())
        ok = ~np.bitwise_xor.reduceat(hard[:, g.rc], g.row_start, axis=1).any(axis=1)
        iters[live[ok]] = it
        keep = ~ok
        live = live[keep]
        if live.size == 0:
            break
        L, v2c = L[keep], v2c[keep]
        c2v = cn_phase(g, v2c, alpha, reverse_rows)
        finite = finite and bool(np.isfinite(c2v).all())
    if stats is not None:
        stats["max_abs_v2c"] = top
        stats["finite"] = finite
    ret = (iters + (iters < max_iter)).astype(np.int32)
    uu_hat = cc_hat[:, g.info_off:g.info_off + g.K].copy()
    return ret, uu_hat, cc_hat
