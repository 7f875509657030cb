"""The arithmetic contract of the offset correction of the min-sum decoders
(kml_set_nms_offset, include/kmldpc_amd.h) as numpy models, for any graph from
oracle.Code.graph().  The offset instances of the three GPU kernels
(bp_irregular_nms.hip, bp_irregular_lnms.hip, bp_irregular_lnms_h16.hip) equal
them bit for bit (tests/test_gpu_oms.py).

The contracts of tests/bp_nms_model.py (flooding), tests/bp_lnms_model.py
(layered), tests/bp_h16_model.py (layered, binary16) and tests/bp_llr_model.py
(the LLR front end) with one change, in the check-node update.  Where those
write c2v_j = RN(alpha * a_j) with its sign bit set to s_j, this one writes

    c = RN(alpha * a_j)
    c = RN(c - b)              one rounding;  b = float32(beta)
    c = c > 0 ? c : +0
    c2v_j = c with its sign bit set to s_j

in binary32 (flooding, layered), and the same three operations in binary16 with
b16 = RN16(float32(beta)) in the binary16 format.  No -0 reaches the comparison:
alpha * a_j is never negative and x - x is +0 in round-to-nearest.  A message of
magnitude zero with its sign bit set (-0) is legal: it counts as negative in the
sign XOR and m + (-0) = m, as the existing rules already say.  Priors, the clamp,
the tie rule, the stop rule, ret and the counters are unchanged.

With beta = 0 the two extra operations change no bit (c - 0 = c, c >= +0), and
every function here equals the model it extends bit for bit
(tests/test_bp_oms_model.py); the kernels then run their instances without the
correction.
"""
import numpy as np

from bp_h16_model import CLAMP16, _set_sign16, alpha16, h16_llr_priors, h16_priors
from bp_llr_model import llr_priors, maxlog_llr, parity_counts
from bp_lnms_model import _layer_groups, _parity_ok
from bp_nms_model import CLAMP, DEFAULT_ALPHA, Graph, _set_sign, priors

__all__ = ["Graph", "beta16", "oms_mag", "oms_mag16", "oms_cn_phase", "oms_nms_model", "oms_lnms_model",
           "oms_h16_model", "oms_llr_model", "oms_lnms_rowwise", "oms_decode", "oms_blind_metric"]


def beta16(beta):
    """RN16(float32(beta))."""
    return np.float16(np.float32(beta))


def oms_mag(a, alpha, beta):
    """The message magnitude of a (float32, sign clear): max(RN(RN(alpha * a) - b), +0)."""
    a32, b32 = np.float32(alpha), np.float32(beta)
    c = (a32 * np.asarray(a, np.float32)).astype(np.float32)
    c = (c - b32).astype(np.float32)
    return np.where(c > 0, c, np.float32(0.0)).astype(np.float32)


def oms_mag16(a, alpha, beta):
    """The same in binary16 (a float16, sign clear)."""
    a16, b16 = alpha16(alpha), beta16(beta)
    c = a16 * np.asarray(a, np.float16)
    c = c - b16
    assert c.dtype == np.float16
    return np.where(c > 0, c, np.float16(0.0)).astype(np.float16)


def oms_cn_phase(g, v2c, alpha, beta):
    """bp_nms_model.cn_phase with the correction: c2v[n, E] from v2c[n, E]."""
    c2v = np.empty_like(v2c)
    mag = np.abs(v2c)
    neg = np.signbit(v2c)
    inf = np.float32(np.inf)
    for d, edges in g.cn_groups:
        x = mag[:, edges]  # [n, R, d]
        s = neg[:, edges]
        tot = np.bitwise_xor.reduce(s, axis=2)
        for j in range(d):
            others = np.delete(x, j, axis=2)
            a = others.min(axis=2) if d > 1 else np.full(x.shape[:2], inf, np.float32)
            c2v[:, edges[:, j]] = _set_sign(oms_mag(a, alpha, beta), tot ^ s[:, :, j])
    return c2v


def _flood(g, L, iter_count, max_iter, alpha, beta, stats):
    """The flooding loop on float32 priors L[B, N]; returns ret, uu_hat, cc_hat, post."""
    B = L.shape[0]
    cc_hat = np.zeros((B, g.N), np.uint8)
    post = np.zeros((B, g.N), np.float32)
    iters = np.full(B, iter_count, np.int64)
    conv = np.zeros(B, bool)
    live = np.arange(B)
    c2v = np.zeros((B, g.E), np.float32)
    top, top_T, finite = 0.0, 0.0, True
    for it in range(iter_count):
        n = live.size
        t = L.copy()
        for cols, e in g.vn_steps:
            t[:, cols] = t[:, cols] + c2v[:, e]
        hard = np.where(t > 0, 0, 1).astype(np.uint8)
        cc_hat[live] = hard
        post[live] = t
        v2c = np.empty((n, g.E), np.float32)
        for cols, e in g.vn_steps:
            v2c[:, e] = np.minimum(np.maximum(t[:, cols] - c2v[:, e], -CLAMP), CLAMP)
        top = max(top, float(np.max(np.abs(v2c))))
        top_T = max(top_T, float(np.abs(t).max()))
        finite = finite and bool(np.isfinite(v2c).all() and np.isfinite(t).all())
        ok = ~np.bitwise_xor.reduceat(hard[:, g.rc], g.row_start, axis=1).any(axis=1)
        iters[live[ok]] = it
        conv[live[ok]] = True
        keep = ~ok
        live = live[keep]
        if live.size == 0:
            break
        L, v2c = L[keep], v2c[keep]
        c2v = oms_cn_phase(g, v2c, alpha, beta)
        finite = finite and bool(np.isfinite(c2v).all())
    if stats is not None:
        stats.update(max_abs_v2c=top, max_abs_m=top, max_abs_T=top_T, finite=finite, iters=iters.copy(),
                     converged=conv.copy())
    ret = (iters + (iters < max_iter)).astype(np.int32)
    return ret, cc_hat[:, g.info_off:g.info_off + g.K].copy(), cc_hat, post


def _layered(g, T, iter_count, max_iter, alpha, beta, stats):
    """The layered loop on priors T[B, N] (consumed), float32 or float16 by T's dtype; returns ret, uu_hat,
    cc_hat, post[B, N] float32."""
    half = T.dtype == np.float16
    assert half or T.dtype == np.float32
    ft = np.float16 if half else np.float32
    clamp = CLAMP16 if half else CLAMP
    bits = np.uint16 if half else np.uint32
    mag_of = oms_mag16 if half else oms_mag
    set_sign = _set_sign16 if half else _set_sign
    B = T.shape[0]
    cc_hat = np.zeros((B, g.N), np.uint8)
    post = np.zeros((B, g.N), np.float32)
    iters = np.zeros(B, np.int64)
    conv = np.zeros(B, bool)
    live = np.arange(B)
    c2v = np.zeros((B, g.E), ft)
    top_m, top_T, finite = 0.0, 0.0, True
    groups = _layer_groups(g)
    it = 0
    while live.size:
        hard, ok = _parity_ok(g, T)
        if iter_count > 0:
            cc_hat[live] = hard
            post[live] = T.astype(np.float32)
        top_T = max(top_T, float(np.abs(T).max()))
        finite = finite and bool(np.isfinite(T).all())
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
                m = np.minimum(np.maximum(T[:, cols] - c2v[:, edges], -clamp), clamp)  # [n, R, d]
                mag = np.abs(m)
                neg = np.signbit(m)
                j1 = np.argmin(mag.view(bits), axis=2)  # (magnitudes compare as their bit patterns)
                min1 = np.take_along_axis(mag, j1[:, :, None], axis=2)
                rest = mag.copy()
                np.put_along_axis(rest, j1[:, :, None], ft(np.inf), axis=2)
                min2 = rest.min(axis=2, keepdims=True)
                a = np.where(np.arange(mag.shape[2])[None, None, :] == j1[:, :, None], min2, min1)
                s = np.bitwise_xor.reduce(neg, axis=2)[:, :, None] ^ neg
                new = set_sign(mag_of(a, alpha, beta), s)
                assert m.dtype == ft and new.dtype == ft
                c2v[:, edges] = new
                T[:, cols] = m + new
                top_m = max(top_m, float(mag.max()))
                finite = finite and bool(np.isfinite(new).all())
        it += 1
    if stats is not None:
        stats.update(max_abs_m=top_m, max_abs_T=top_T, finite=finite, iters=iters.copy(), converged=conv.copy())
    ret = (iters + (iters < max_iter)).astype(np.int32)
    return ret, cc_hat[:, g.info_off:g.info_off + g.K].copy(), cc_hat, post


def oms_nms_model(g, p0, iter_count, max_iter, alpha=DEFAULT_ALPHA, beta=0.0, stats=None):
    """bp_nms_model.nms_model (flooding, P0 priors) with the correction; returns ret, uu_hat, cc_hat."""
    return _flood(g, priors(g, p0), iter_count, max_iter, alpha, beta, stats)[:3]


def oms_lnms_model(g, p0, iter_count, max_iter, alpha=DEFAULT_ALPHA, beta=0.0, stats=None):
    """bp_lnms_model.lnms_model (layered, P0 priors) with the correction; returns ret, uu_hat, cc_hat."""
    return _layered(g, priors(g, p0), iter_count, max_iter, alpha, beta, stats)[:3]


def oms_h16_model(g, p0, iter_count, max_iter, alpha=DEFAULT_ALPHA, beta=0.0, stats=None):
    """bp_h16_model.lnms_h16_model (layered binary16, P0 priors) with the correction; returns ret, uu_hat, cc_hat."""
    return _layered(g, h16_priors(g, p0), iter_count, max_iter, alpha, beta, stats)[:3]


def oms_llr_model(g, llr, iter_count, max_iter, alpha=DEFAULT_ALPHA, beta=0.0, schedule="flooding", messages="f32",
                  stats=None):
    """The LLR front end (bp_llr_model.llr_decode_model, bp_h16_model.lnms_h16_llr_model) with the correction;
    returns ret, uu_hat, cc_hat, T[B, N] float32."""
    if messages == "f16":
        assert schedule == "layered"
        return _layered(g, h16_llr_priors(g, llr), iter_count, max_iter, alpha, beta, stats)
    if schedule == "layered":
        return _layered(g, llr_priors(g, llr), iter_count, max_iter, alpha, beta, stats)
    return _flood(g, llr_priors(g, llr), iter_count, max_iter, alpha, beta, stats)


def oms_decode(g, p0, iter_count, max_iter, alpha=DEFAULT_ALPHA, beta=0.0, schedule="flooding", messages="f32",
               stats=None):
    """The P0 front end of any of the three decoders; returns ret, uu_hat, cc_hat."""
    if messages == "f16":
        assert schedule == "layered"
        return oms_h16_model(g, p0, iter_count, max_iter, alpha, beta, stats)
    f = oms_lnms_model if schedule == "layered" else oms_nms_model
    return f(g, p0, iter_count, max_iter, alpha, beta, stats)


def oms_lnms_rowwise(g, p0, iter_count, max_iter, alpha=DEFAULT_ALPHA, beta=0.0):
    """The layered f32 contract as written: one row after the other, one edge after the other (vectorised over
    codewords only; a codeword that has stopped is frozen by restoring its state)."""
    T = priors(g, p0)
    B = T.shape[0]
    c2v = np.zeros((B, g.E), np.float32)
    cc_hat = np.zeros((B, g.N), np.uint8)
    iters = np.zeros(B, np.int64)
    done = np.zeros(B, bool)
    inf = np.float32(np.inf)
    for it in range(iter_count + 1):
        hard, ok = _parity_ok(g, T)
        run = ~done
        if iter_count > 0:
            cc_hat[run] = hard[run]
        iters[run] = it
        done |= ok
        if it == iter_count or done.all():
            break
        T0, c0 = T.copy(), c2v.copy()
        for r in range(g.M):
            e0, e1 = int(g.rp[r]), int(g.rp[r + 1])
            m = []
            for e in range(e0, e1):
                m.append(np.minimum(np.maximum(T[:, g.rc[e]] - c2v[:, e], -CLAMP), CLAMP))
            for j, e in enumerate(range(e0, e1)):
                a = np.full(B, inf, np.float32)
                s = np.zeros(B, bool)
                for i in range(e1 - e0):
                    if i != j:
                        a = np.minimum(a, np.abs(m[i]))
                        s = s ^ np.signbit(m[i])
                c2v[:, e] = _set_sign(oms_mag(a, alpha, beta), s)
                T[:, g.rc[e]] = m[j] + c2v[:, e]
        T[done], c2v[done] = T0[done], c0[done]
    ret = (iters + (iters < max_iter)).astype(np.int32)
    return ret, cc_hat[:, g.info_off:g.info_off + g.K].copy(), cc_hat


def oms_blind_metric(g, points, bits, y, h_cand, var, metric_iter, max_iter, alpha=DEFAULT_ALPHA, beta=0.0,
                     schedule="flooding", messages="f32"):
    """bp_llr_model.blind_metric with the correction: the blind 5G metric under KML_DEMAP_MAXLOG.  h_cand[B, nc, 2];
    returns metrics[B, 4] float64 (entries >= nc are 0), chosen[B] int32 (the first minimum) and the candidates'
    LLRs [B, nc, cc_len] float32."""
    h_cand = np.asarray(h_cand, np.float64)
    B, nc = h_cand.shape[0], h_cand.shape[1]
    met = np.zeros((B, 4))
    llrs = np.empty((B, nc, g.cc_len), np.float32)
    for j in range(nc):
        llrs[:, j] = maxlog_llr(points, bits, y, h_cand[:, j], var)
        _, _, cch, _ = oms_llr_model(g, llrs[:, j], metric_iter, max_iter, alpha, beta, schedule, messages)
        met[:, j] = parity_counts(g, cch)
    chosen = np.argmin(met[:, :nc], axis=1).astype(np.int32)
    return met, chosen, llrs
