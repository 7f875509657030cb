"""The arithmetic contract of the layered schedule of the normalized min-sum
mode (KML_SCHED_LAYERED, include/kmldpc_amd.h), as a numpy model vectorised
over codewords and over the rows of a layer, for any graph from
oracle.Code.graph().  The GPU kernel (kmldpc_amd/csrc/bp_irregular_lnms.hip)
equals it bit for bit (tests/test_gpu_lnms.py).

What tests/bp_nms_model.py fixes stays fixed: IEEE binary32 values with
denormals kept, no fma, each operation rounded once; the priors
(L = float32(log(q) - log(1 - q)) with the 1e-12 clip and the subtraction in
float64, +0 for a punctured column); alpha rounded once to float; the +-256
clamp; a tie decides 1.

The state is T[v] = L[v], one posterior per column, and c2v[e] = +0, one value
per edge in row-major order.

    hard = (T > 0 ? 0 : 1);  it = 0
    loop:
      if every row of hard has even parity: converged, stop
      if it == iter_count: stop
      for r = 0 .. M-1 in row index order:                    # one sweep
          for each edge j of r (column v_j):
              m_j = clamp(T[v_j] - c2v_j, -256, 256)
          a_j = min_{i != j} |m_i|
          s_j = XOR_{i != j} signbit(m_i)                     # -0 counts as negative
          c2v_j = float32(alpha * a_j) with its sign bit set to s_j
          T[v_j] = m_j + c2v_j
      it += 1
      hard = (T > 0 ? 0 : 1)

ret = it + (it < max_iter); iter_count = 0 leaves the outputs as passed (here:
zeros).  A budget of k uses all k sweeps (the flooding schedule's last CN phase
is never read: a deliberate difference).

A layer is a maximal run of consecutive rows with pairwise disjoint columns,
found greedily in row order (layers()).  The rows of a layer touch disjoint T
and c2v entries, so working on them at once gives exactly the serial result:
lnms_model does, lnms_rowwise is the plain row-by-row loop it is held to.
"""
import numpy as np

from bp_nms_model import CLAMP, DEFAULT_ALPHA, Graph, _set_sign, priors

__all__ = ["Graph", "layers", "lnms_model", "lnms_rowwise"]


def layers(g):
    """layer_ptr[nl + 1]: a row that shares a column with the open layer closes it and opens the next."""
    ptr = [0]
    seen = np.zeros(g.N, bool)
    for r in range(g.M):
        cols = g.rc[g.rp[r]:g.rp[r + 1]]
        if seen[cols].any():
            ptr.append(r)
            seen[:] = False
        seen[cols] = True
    ptr.append(g.M)
    return np.array(ptr, np.int32)


def _layer_groups(g):
    """Per layer, its rows grouped by degree: [(edges[R, d], cols[R, d]), ...] (made once per graph)."""
    if not hasattr(g, "_lnms_groups"):
        lp = layers(g)
        dc = np.diff(g.rp)
        out = []
        for a, b in zip(lp[:-1], lp[1:]):
            rows = np.arange(a, b)
            groups = []
            for d in sorted(set(int(x) for x in dc[rows])):
                rr = rows[dc[rows] == d]
                edges = g.rp[rr][:, None] + np.arange(d)[None, :]
                groups.append((edges, g.rc[edges]))
            out.append(groups)
        g._lnms_groups = out
    return g._lnms_groups


def _parity_ok(g, T):
    hard = np.where(T > 0, 0, 1).astype(np.uint8)
    return hard, ~np.bitwise_xor.reduceat(hard[:, g.rc], g.row_start, axis=1).any(axis=1)


def lnms_model(g, p0, iter_count, max_iter, alpha=DEFAULT_ALPHA, stats=None):
    """Decode p0[B, cc_len]; returns ret[B] int32, uu_hat[B, K], cc_hat[B, N] uint8.
    stats (a dict) receives max_abs_m (the largest |m|), max_abs_T, finite, iters[B] and converged[B]."""
    a32 = np.float32(alpha)
    T = priors(g, p0)
    B = T.shape[0]
    cc_hat = np.zeros((B, g.N), np.uint8)
    iters = np.zeros(B, np.int64)
    conv = np.zeros(B, bool)
    live = np.arange(B)
    c2v = np.zeros((B, g.E), np.float32)
    top_m, top_T, finite = 0.0, 0.0, True
    groups = _layer_groups(g)
    it = 0
    while live.size:
        hard, ok = _parity_ok(g, T)
        if iter_count > 0:
            cc_hat[live] = hard
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
                top_m = max(top_m, float(mag.max()))
                finite = finite and bool(np.isfinite(new).all())
        top_T = max(top_T, float(np.abs(T).max()))
        finite = finite and bool(np.isfinite(T).all())
        it += 1
    if stats is not None:
        stats.update(max_abs_m=top_m, max_abs_T=top_T, finite=finite, iters=iters.copy(), converged=conv.copy())
    ret = (iters + (iters < max_iter)).astype(np.int32)
    uu_hat = cc_hat[:, g.info_off:g.info_off + g.K].copy()
    return ret, uu_hat, cc_hat


def lnms_rowwise(g, p0, iter_count, max_iter, alpha=DEFAULT_ALPHA):
    """The contract as written: one row after the other, one edge after the other (vectorised over
    codewords only; a codeword that has stopped is frozen by restoring its state)."""
    a32 = np.float32(alpha)
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
                c2v[:, e] = _set_sign((a32 * a).astype(np.float32), s)
                T[:, g.rc[e]] = m[j] + c2v[:, e]
        T[done], c2v[done] = T0[done], c0[done]
    ret = (iters + (iters < max_iter)).astype(np.int32)
    return ret, cc_hat[:, g.info_off:g.info_off + g.K].copy(), cc_hat
