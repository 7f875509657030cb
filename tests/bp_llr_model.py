"""The arithmetic contract of the LLR front end of the min-sum mode (kml_demap_llr,
kml_llr_decode and KML_DEMAP_MAXLOG, include/kmldpc_amd.h) as numpy models.
The GPU kernels (kmldpc_amd/csrc/demap_llr.hip and the LLR instances of
bp_irregular_nms.hip / bp_irregular_lnms.hip) equal them bit for bit
(tests/test_gpu_llr.py).

Every value is IEEE binary32 (numpy float32: denormals kept, no fma, each
operation rounded once).

Max-log demapper.  Rounded once to float32: y[s] and h (float64 in the
interface), the normalised constellation points x_k, and inv = float32(1 / var)
with the division in float64.  Per symbol s and point k

    gr = hr*xr_k - hi*xi_k      gi = hr*xi_k + hi*xr_k
    er = yr - gr                ei = yi - gi
    d_k = er*er + ei*ei

and for bit i of the symbol (the label's bits most significant first: bit i of
point k is (k >> (bits - 1 - i)) & 1, the exact demapper's order)

    L[s*bits + i] = (min_{k: bit_i(k) = 1} d_k - min_{k: bit_i(k) = 0} d_k) * inv.

Positive means bit 0.  No clamp, no clip.

LLR-in decode.  The contracts of tests/bp_nms_model.py (flooding) and
tests/bp_lnms_model.py (layered) with one change, the prior:
L[v] = min(max(x, -256), 256) of the caller's float32, +0 for a punctured
column.  Both decoders also return T, the posteriors the returned decisions
were taken from: in the flooding schedule the T of the VN phase whose decisions
are returned, in the layered schedule T as the loop left it; iter_count = 0
leaves it as passed (here: zeros).

Blind 5G metric under KML_DEMAP_MAXLOG: for each of the candidates (the four
rotations of k-means' estimate) the unsatisfied checks of the decisions the
context's min-sum decoder returns after metric_iter iterations on the max-log
LLRs of that candidate; chosen = the first minimum.
"""
import numpy as np

from bp_lnms_model import _layer_groups, _parity_ok
from bp_nms_model import CLAMP, DEFAULT_ALPHA, Graph, _set_sign, cn_phase

__all__ = ["Graph", "maxlog_llr", "llr_priors", "nms_llr_model", "lnms_llr_model", "llr_decode_model",
           "parity_counts", "blind_metric"]


def maxlog_llr(points, bits, y, h, var):
    """LLRs [B, S*bits] float32 of y[B, S, 2] with one channel h[B, 2] per codeword; points[Kc, 2] float64."""
    pts = np.asarray(points, np.float64).reshape(-1, 2).astype(np.float32)
    assert pts.shape[0] == 1 << bits
    y32 = np.asarray(y, np.float64).astype(np.float32)
    B, S = y32.shape[0], y32.shape[1]
    h32 = np.asarray(h, np.float64).reshape(B, 2).astype(np.float32)
    inv = np.float32(1.0 / float(var))
    yr, yi = y32[:, :, 0, None], y32[:, :, 1, None]          # [B, S, 1]
    hr, hi = h32[:, 0, None, None], h32[:, 1, None, None]    # [B, 1, 1]
    xr, xi = pts[None, None, :, 0], pts[None, None, :, 1]    # [1, 1, Kc]
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        gr = hr * xr - hi * xi
        gi = hr * xi + hi * xr
        er = yr - gr
        ei = yi - gi
        d = er * er + ei * ei                                # [B, S, Kc]
        out = np.empty((B, S, bits), np.float32)
        k = np.arange(1 << bits)
        for i in range(bits):
            one = ((k >> (bits - 1 - i)) & 1) == 1
            out[:, :, i] = (d[:, :, one].min(axis=2) - d[:, :, ~one].min(axis=2)) * inv
    assert out.dtype == np.float32
    return out.reshape(B, S * bits)


def llr_priors(g, llr):
    """The decoders' float32 priors [B, N] of llr[B, cc_len]: clamped to +-256, +0 on the punctured columns."""
    x = np.ascontiguousarray(llr, np.float32).reshape(-1, g.cc_len)
    L = np.zeros((x.shape[0], g.N), np.float32)
    L[:, g.punct:] = np.minimum(np.maximum(x, -CLAMP), CLAMP)
    return L


def nms_llr_model(g, llr, iter_count, max_iter, alpha=DEFAULT_ALPHA, stats=None):
    """bp_nms_model.nms_model on LLR priors; returns ret, uu_hat, cc_hat, T[B, N] float32."""
    L = llr_priors(g, llr)
    B = L.shape[0]
    cc_hat = np.zeros((B, g.N), np.uint8)
    post = np.zeros((B, g.N), np.float32)
    iters = np.full(B, iter_count, np.int64)
    conv = np.zeros(B, bool)
    live = np.arange(B)
    c2v = np.zeros((B, g.E), np.float32)
    top_T = 0.0
    for it in range(iter_count):
        n = live.size
        t = L.copy()
        for cols, e in g.vn_steps:
            t[:, cols] = t[:, cols] + c2v[:, e]
        hard = np.where(t > 0, 0, 1).astype(np.uint8)
        cc_hat[live] = hard
        post[live] = t
        top_T = max(top_T, float(np.abs(t).max()))
        v2c = np.empty((n, g.E), np.float32)
        for cols, e in g.vn_steps:
            v2c[:, e] = np.minimum(np.maximum(t[:, cols] - c2v[:, e], -CLAMP), CLAMP)
        ok = ~np.bitwise_xor.reduceat(hard[:, g.rc], g.row_start, axis=1).any(axis=1)
        iters[live[ok]] = it
        conv[live[ok]] = True
        keep = ~ok
        live = live[keep]
        if live.size == 0:
            break
        L, v2c = L[keep], v2c[keep]
        c2v = cn_phase(g, v2c, alpha)
    if stats is not None:
        stats.update(max_abs_T=top_T, iters=iters.copy(), converged=conv.copy())
    ret = (iters + (iters < max_iter)).astype(np.int32)
    return ret, cc_hat[:, g.info_off:g.info_off + g.K].copy(), cc_hat, post


def lnms_llr_model(g, llr, iter_count, max_iter, alpha=DEFAULT_ALPHA, stats=None):
    """bp_lnms_model.lnms_model on LLR priors; returns ret, uu_hat, cc_hat, T[B, N] float32."""
    a32 = np.float32(alpha)
    T = llr_priors(g, llr)
    B = T.shape[0]
    cc_hat = np.zeros((B, g.N), np.uint8)
    post = np.zeros((B, g.N), np.float32)
    iters = np.zeros(B, np.int64)
    conv = np.zeros(B, bool)
    live = np.arange(B)
    c2v = np.zeros((B, g.E), np.float32)
    top_T = 0.0
    groups = _layer_groups(g)
    it = 0
    while live.size:
        hard, ok = _parity_ok(g, T)
        if iter_count > 0:
            cc_hat[live] = hard
            post[live] = T
        top_T = max(top_T, float(np.abs(T).max()))
        iters[live] = it
        conv[live[ok]] = True
        if it == iter_count:
            break
        keep = ~ok
        live, T, c2v = live[keep], T[keep], c2v[keep]
        if live.size == 0:
            break
        for layer in groups:
            for edges, cols in layer:
                m = np.minimum(np.maximum(T[:, cols] - c2v[:, edges], -CLAMP), CLAMP)  # [n, R, d]
                mag = np.abs(m)
                neg = np.signbit(m)
                j1 = np.argmin(mag, axis=2)
                min1 = np.take_along_axis(mag, j1[:, :, None], axis=2)
                rest = mag.copy()
                np.put_along_axis(rest, j1[:, :, None], np.float32(np.inf), axis=2)
                min2 = rest.min(axis=2, keepdims=True)
                a = np.where(np.arange(mag.shape[2])[None, None, :] == j1[:, :, None], min2, min1)
                s = np.bitwise_xor.reduce(neg, axis=2)[:, :, None] ^ neg
                new = _set_sign((a32 * a).astype(np.float32), s)
                c2v[:, edges] = new
                T[:, cols] = m + new
        it += 1
    if stats is not None:
        stats.update(max_abs_T=top_T, iters=iters.copy(), converged=conv.copy())
    ret = (iters + (iters < max_iter)).astype(np.int32)
    return ret, cc_hat[:, g.info_off:g.info_off + g.K].copy(), cc_hat, post


def llr_decode_model(g, llr, iter_count, max_iter, alpha=DEFAULT_ALPHA, schedule="flooding", stats=None):
    f = {"flooding": nms_llr_model, "layered": lnms_llr_model}[schedule]
    return f(g, llr, iter_count, max_iter, alpha, stats=stats)


def parity_counts(g, cc_hat):
    """Unsatisfied checks of each row of cc_hat[B, N]."""
    return np.bitwise_xor.reduceat(cc_hat[:, g.rc], g.row_start, axis=1).sum(axis=1).astype(np.int32)


def blind_metric(g, points, bits, y, h_cand, var, metric_iter, max_iter, alpha=DEFAULT_ALPHA, schedule="flooding"):
    """The blind 5G metric: h_cand[B, nc, 2] (k-means' four rotations, or the caller's candidates).
    Returns metrics[B, 4] float64 (entries >= nc are 0), chosen[B] int32 (the first minimum) and the
    candidates' LLRs [B, nc, cc_len] float32."""
    h_cand = np.asarray(h_cand, np.float64)
    B, nc = h_cand.shape[0], h_cand.shape[1]
    met = np.zeros((B, 4))
    llrs = np.empty((B, nc, g.cc_len), np.float32)
    for j in range(nc):
        llrs[:, j] = maxlog_llr(points, bits, y, h_cand[:, j], var)
        _, _, cch, _ = llr_decode_model(g, llrs[:, j], metric_iter, max_iter, alpha, schedule)
        met[:, j] = parity_counts(g, cch)
    chosen = np.argmin(met[:, :nc], axis=1).astype(np.int32)
    return met, chosen, llrs
