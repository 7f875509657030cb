"""The arithmetic contract of the binary16 message format of the layered min-sum
decoder (KML_MSG_F16, include/kmldpc_amd.h) as numpy models, for any graph from
oracle.Code.graph().  The GPU kernel (kmldpc_amd/csrc/bp_irregular_lnms_h16.hip)
equals them bit for bit (tests/test_gpu_h16.py).

It is the layered contract of tests/bp_lnms_model.py with one change: every
value of the decoder state is IEEE binary16, denormals kept, no fma, each
operation rounded once to nearest-even.

    prior   L16 = RN16(L), L the float32 prior of the f32 contract: the P0 front
            end's float32(log q - log(1 - q)) (bp_nms_model.priors) or the LLR
            front end's min(max(x, -256), 256) (bp_llr_model.llr_priors); +0 for
            a punctured column
    alpha   a16 = RN16(float32(alpha)): to float first, then to half
    sweep   m_j   = clamp(T[v_j] - c2v_j, -256, 256)
            a_j   = min over i != j of |m_i|, the magnitudes compared as the
                    unsigned integers their 15-bit patterns are
            s_j   = XOR over i != j of the sign bits (-0 counts as negative)
            c2v_j = RN16(a16 * a_j) with its sign bit set to s_j
            T[v_j] = m_j + c2v_j

Decisions (T > 0 ? 0 : 1, a tie decides 1), the stop rule, ret = it + (it <
max_iter) and iter_count = 0 (outputs as passed, here zeros) are the f32
contract's.  The posteriors returned are the binary16 T widened to float32,
which is exact: -0 and +0 differ.

numpy's float16 is an exact model of the hardware's packed half arithmetic: it
computes each operation in float32 and rounds the result to half.  A float32
significand has 24 >= 2 * 11 + 2 bits, so for +, - and x the double rounding is
innocuous (the float32 result of two halves is exact or far enough from a half
tie), min, max and the comparisons are exact anyway, and the conversion from
float32 is one round-to-nearest-even with denormal results kept.  Every contract
operation below is one numpy operation on float16 arrays.
"""
import numpy as np

from bp_llr_model import llr_priors, maxlog_llr, parity_counts
from bp_lnms_model import _layer_groups, _parity_ok
from bp_nms_model import DEFAULT_ALPHA, Graph, priors

__all__ = ["Graph", "CLAMP16", "alpha16", "h16_priors", "h16_llr_priors", "lnms_h16_model", "lnms_h16_llr_model",
           "lnms_h16_rowwise", "blind_metric_h16"]

CLAMP16 = np.float16(256.0)


def alpha16(alpha):
    """RN16(float32(alpha))."""
    return np.float16(np.float32(alpha))


def h16_priors(g, p0):
    """The P0 front end's priors [B, N] float16."""
    return priors(g, p0).astype(np.float16)


def h16_llr_priors(g, llr):
    """The LLR front end's priors [B, N] float16."""
    return llr_priors(g, llr).astype(np.float16)


def _set_sign16(mag, neg):
    return (mag.view(np.uint16) | (neg.astype(np.uint16) << np.uint16(15))).view(np.float16)


def _decode(g, T, iter_count, max_iter, alpha, stats):
    """The loop on float16 priors T[B, N] (consumed); returns ret, uu_hat, cc_hat, post[B, N] float32."""
    assert T.dtype == np.float16
    a16 = alpha16(alpha)
    B = T.shape[0]
    cc_hat = np.zeros((B, g.N), np.uint8)
    post = np.zeros((B, g.N), np.float32)
    iters = np.zeros(B, np.int64)
    conv = np.zeros(B, bool)
    live = np.arange(B)
    c2v = np.zeros((B, g.E), np.float16)
    top_m, top_T, finite = 0.0, 0.0, True
    groups = _layer_groups(g)
    inf = np.float16(np.inf)
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
                m = np.minimum(np.maximum(T[:, cols] - c2v[:, edges], -CLAMP16), CLAMP16)  # [n, R, d]
                mag = np.abs(m)
                neg = np.signbit(m)
                j1 = np.argmin(mag.view(np.uint16), axis=2)
                min1 = np.take_along_axis(mag, j1[:, :, None], axis=2)
                rest = mag.copy()
                np.put_along_axis(rest, j1[:, :, None], inf, axis=2)
                min2 = rest.min(axis=2, keepdims=True)
                a = np.where(np.arange(mag.shape[2])[None, None, :] == j1[:, :, None], min2, min1)
                s = np.bitwise_xor.reduce(neg, axis=2)[:, :, None] ^ neg
                new = _set_sign16(a16 * a, s)
                assert m.dtype == np.float16 and new.dtype == np.float16
                c2v[:, edges] = new
                T[:, cols] = m + new
                top_m = max(top_m, float(mag.max()))
                finite = finite and bool(np.isfinite(new).all())
        it += 1
    if stats is not None:
        stats.update(max_abs_m=top_m, max_abs_T=top_T, finite=finite, iters=iters.copy(), converged=conv.copy())
    ret = (iters + (iters < max_iter)).astype(np.int32)
    return ret, cc_hat[:, g.info_off:g.info_off + g.K].copy(), cc_hat, post


def lnms_h16_model(g, p0, iter_count, max_iter, alpha=DEFAULT_ALPHA, stats=None):
    """Decode p0[B, cc_len] (float64 P(bit = 0)); returns ret[B] int32, uu_hat[B, K], cc_hat[B, N] uint8.
    stats (a dict) receives max_abs_m, max_abs_T, finite, iters[B] and converged[B]."""
    return _decode(g, h16_priors(g, p0), iter_count, max_iter, alpha, stats)[:3]


def lnms_h16_llr_model(g, llr, iter_count, max_iter, alpha=DEFAULT_ALPHA, stats=None, priors16=None):
    """Decode llr[B, cc_len] float32; returns ret, uu_hat, cc_hat, T[B, N] float32 (the binary16 posteriors the
    decisions came from, widened).  priors16: float16 priors [B, N] to use in place of llr's."""
    T = h16_llr_priors(g, llr) if priors16 is None else np.array(priors16, np.float16)
    return _decode(g, T, iter_count, max_iter, alpha, stats)


def lnms_h16_rowwise(g, p0, iter_count, max_iter, alpha=DEFAULT_ALPHA):
    """The contract as written: one row after the other, one edge after the other (vectorised over codewords
    only; a codeword that has stopped is frozen by restoring its state)."""
    a16 = alpha16(alpha)
    T = h16_priors(g, p0)
    B = T.shape[0]
    c2v = np.zeros((B, g.E), np.float16)
    cc_hat = np.zeros((B, g.N), np.uint8)
    iters = np.zeros(B, np.int64)
    done = np.zeros(B, bool)
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
                m.append(np.minimum(np.maximum(T[:, g.rc[e]] - c2v[:, e], -CLAMP16), CLAMP16))
            for j, e in enumerate(range(e0, e1)):
                a = np.full(B, 0x7C00, np.uint16)  # above every magnitude's 15-bit pattern
                s = np.zeros(B, bool)
                for i in range(e1 - e0):
                    if i != j:
                        a = np.minimum(a, m[i].view(np.uint16) & np.uint16(0x7FFF))
                        s = s ^ np.signbit(m[i])
                c2v[:, e] = _set_sign16(a16 * a.view(np.float16), s)
                T[:, g.rc[e]] = m[j] + c2v[:, e]
        T[done], c2v[done] = T0[done], c0[done]
    ret = (iters + (iters < max_iter)).astype(np.int32)
    return ret, cc_hat[:, g.info_off:g.info_off + g.K].copy(), cc_hat


def blind_metric_h16(g, points, bits, y, h_cand, var, metric_iter, max_iter, alpha=DEFAULT_ALPHA):
    """bp_llr_model.blind_metric with the binary16 layered decoder: h_cand[B, nc, 2]; returns metrics[B, 4]
    float64 (entries >= nc are 0), chosen[B] int32 (the first minimum) and the candidates' LLRs
    [B, nc, cc_len] float32."""
    h_cand = np.asarray(h_cand, np.float64)
    B, nc = h_cand.shape[0], h_cand.shape[1]
    met = np.zeros((B, 4))
    llrs = np.empty((B, nc, g.cc_len), np.float32)
    for j in range(nc):
        llrs[:, j] = maxlog_llr(points, bits, y, h_cand[:, j], var)
        _, _, cch, _ = lnms_h16_llr_model(g, llrs[:, j], metric_iter, max_iter, alpha)
        met[:, j] = parity_counts(g, cch)
    chosen = np.argmin(met[:, :nc], axis=1).astype(np.int32)
    return met, chosen, llrs
