"""Generate the synthetic parity-check matrices tests/golden/data/syn_*.txt.gz.

PROVENANCE ONLY: the outputs are committed and the tests never regenerate
them.  numpy with a fixed seed per file; every graph is a configuration model
(column and row stubs matched by a random permutation) whose duplicate edges
are repaired by column swaps with random other edges.  Rows are written in the
reference's H text format (rows' columns ascending, the header's third number
= M).

    python tests/golden/make_codes.py          # writes every file
    python tests/golden/make_codes.py --check  # regenerates in memory, compares with the committed files

What each code is for (the kernel family it must decode on):
  syn_irr1200      1200 x 600, columns of degree 1..9, rows of degree 2..10:
                   bp_irregular_kernel, every degree instance, mixed / idle /
                   partial pair waves, the non-5G epilogue, K = 600
  syn_reg36_192    (3,6) regular, fits LDS, not N = 2304: bp_kernel <3,6> in LDS
  syn_reg48_240    (4,8) regular, rank 119 (the rows sum to zero): bp_kernel
                   <12,12>, the rank-deficient elimination, K = 121
  syn_high120      120 x 60 with degrees up to 30: bp_kernel <32,32>, K = 60 < 64
  syn_reg36_4080   (3,6) regular beyond LDS, 4080 / 4 not a multiple of 16:
                   bp_kernel with global slots
  syn_reg36_4160   (3,6) regular, NG = 1040, MG = 520: bp_part_kernel
  syn_reg36_2304   (3,6) regular, 2304 x 1152, full rank: bp_regular_kernel and
                   bp_regular_f32_kernel on a graph that is not PEG2304 (26 4-cycles
                   where PEG2304 has none, its own placement plan and
                   systematic-form column swaps), K = 1152
  syn_reg36_2304_r1147  the same class with five pairs of identical rows (rows
                   that share six columns; 93 4-cycles): rank 1147, K = 1157
                   (Kw = 19, five bits in the last word), chk = 1147
"""
import gzip
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DATA = os.path.join(HERE, "data")


def expand(profile):
    """{degree: count} -> the degree of every node, in ascending degree order."""
    return np.concatenate([np.full(c, d, np.int64) for d, c in sorted(profile.items())])


# name: (seed, column profile {degree: count}, row profile, expected GF(2) rank)
CODES = {
    "syn_irr1200": (1200, {1: 70, 2: 300, 3: 400, 4: 200, 5: 50, 6: 70, 7: 40, 8: 40, 9: 30},
                    {2: 40, 3: 70, 4: 30, 5: 30, 6: 40, 7: 70, 8: 120, 9: 40, 10: 160}, 600),
    "syn_reg36_192": (192, {3: 192}, {6: 96}, 96),
    "syn_reg48_240": (240, {4: 240}, {8: 120}, 119),
    "syn_high120": (120, {20: 6, 12: 12, 5: 30, 3: 72}, {30: 4, 13: 10, 9: 12, 8: 34}, 60),
    "syn_reg36_4080": (4080, {3: 4080}, {6: 2040}, 2040),
    "syn_reg36_4160": (4160, {3: 4160}, {6: 2080}, 2080),
    "syn_reg36_2304": (2304, {3: 2304}, {6: 1152}, 1152),
    "syn_reg36_2304_r1147": (2305, {3: 2304}, {6: 1152}, 1147),
}
# Pairs of identical rows.  A code whose columns all have odd degree cannot lose
# rank the way syn_reg48_240 does (its rows do not sum to zero), so d pairs of
# equal rows take d off the rank instead: 6 d columns keep one edge for the
# configuration model over the other M - 2 d rows, each pair then covers six of
# them twice, and the row order is shuffled.  Two equal rows share six columns
# and no edge, so the graph stays simple and the degrees are the profiles'.
TWIN_ROWS = {"syn_reg36_2304_r1147": 5}


def configuration_model(rng, col_deg, row_deg):
    """Edges (row, col) of a simple bipartite graph with the given degrees."""
    assert col_deg.sum() == row_deg.sum()
    cols = np.repeat(np.arange(len(col_deg)), col_deg)
    rows = np.repeat(np.arange(len(row_deg)), row_deg)
    cols = cols[rng.permutation(len(cols))]
    E = len(cols)
    N = len(col_deg)
    for _ in range(1000):
        key = rows * N + cols
        order = np.argsort(key, kind="stable")
        dup = order[1:][key[order][1:] == key[order][:-1]]
        if len(dup) == 0:
            return rows, cols
        present = set(key.tolist())
        for e in dup:  # swap the duplicate's column with a random edge's, if both new edges are new
            for _ in range(1000):
                f = int(rng.integers(E))
                a, b = rows[e] * N + cols[f], rows[f] * N + cols[e]
                if rows[f] != rows[e] and a not in present and b not in present:
                    cols[e], cols[f] = cols[f], cols[e]
                    present.update((int(a), int(b)))
                    break
    raise RuntimeError("duplicate edges left")


def gf2_rank(rows, cols, M, N):
    W = (N + 63) // 64
    A = np.zeros((M, W), np.uint64)
    np.bitwise_or.at(A, (rows, cols // 64), np.uint64(1) << (cols % 64).astype(np.uint64))
    rank = 0
    for c in range(N):
        w, bit = c // 64, np.uint64(1) << np.uint64(c % 64)
        hit = np.nonzero(A[rank:, w] & bit)[0]
        if len(hit) == 0:
            continue
        p = rank + int(hit[0])
        A[[rank, p]] = A[[p, rank]]
        below = rank + 1 + np.nonzero(A[rank + 1:, w] & bit)[0]
        A[below] ^= A[rank]
        rank += 1
        if rank == M:
            break
    return rank


def make(name):
    seed, cprof, rprof, want_rank = CODES[name]
    rng = np.random.default_rng(seed)
    col_deg = expand(cprof)
    row_deg = expand(rprof)
    col_deg = col_deg[rng.permutation(len(col_deg))]
    row_deg = row_deg[rng.permutation(len(row_deg))]
    M, N = len(row_deg), len(col_deg)
    d = TWIN_ROWS.get(name, 0)
    if d:
        assert (row_deg[M - 2 * d:] == 6).all()
        twin_cols = rng.permutation(N)[:6 * d]
        col_deg[twin_cols] -= 2
        rows, cols = configuration_model(rng, col_deg, row_deg[:M - 2 * d])
        col_deg[twin_cols] += 2
        rows = np.concatenate([rows, M - 2 * d + np.repeat(np.arange(2 * d), 6)])
        cols = np.concatenate([cols, np.repeat(twin_cols.reshape(d, 6), 2, axis=0).reshape(-1)])
        shuffle = rng.permutation(M)
        rows = shuffle[rows]
        row_deg = np.bincount(rows, minlength=M)
    else:
        rows, cols = configuration_model(rng, col_deg, row_deg)
    assert len(set((rows * N + cols).tolist())) == len(rows)
    assert np.array_equal(np.bincount(cols, minlength=N), col_deg)
    assert np.array_equal(np.bincount(rows, minlength=M), row_deg)
    rank = gf2_rank(rows, cols, M, N)
    assert rank == want_rank, f"{name}: rank {rank}, expected {want_rank}"
    lines = ["num_of_row--num_of_col--rank_of_H", f"{M}\t{N}\t{M}", "no_of_row--degree_of_row--no_of_col"]
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    ptr = np.concatenate([[0], np.cumsum(row_deg)])
    for r in range(M):
        cs = cols[ptr[r]:ptr[r + 1]]
        lines.append(f"{r} {len(cs)} " + " ".join(str(int(c)) for c in cs) + " ")
    return ("\n".join(lines) + "\n").encode(), dict(M=M, N=N, E=len(rows), rank=rank)


def main():
    check = "--check" in sys.argv
    for name in CODES:
        raw, info = make(name)
        path = os.path.join(DATA, name + ".txt.gz")
        if check:
            with gzip.open(path, "rb") as g:
                assert g.read() == raw, f"{name}: committed file differs"
        else:
            with gzip.GzipFile(path, "wb", mtime=0) as g:
                g.write(raw)
        print(name, info, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
