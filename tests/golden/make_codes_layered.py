"""Generate tests/golden/data/syn_qc_l200.txt.gz: a small quasi-cyclic irregular
code whose greedy layers (include/kmldpc_amd.h, kml_code_layers) are its block
rows, each larger than one pass of bp_irregular_lnms_kernel's row mapping.

PROVENANCE ONLY: the output is committed and the tests never regenerate it.
numpy with a fixed seed.

    python tests/golden/make_codes_layered.py          # writes the file
    python tests/golden/make_codes_layered.py --check  # regenerates in memory, compares with the committed file

The code: a 4 x 8 base matrix, every entry a Z x Z circulant permutation
(row i of a block with shift s holds column (i + s) mod Z), Z = 200: M = 800,
N = 1600, E = 4400.  Base column degrees 4 4 3 3 2 2 2 2, base row degrees
6 5 6 5, so the code is irregular with column degrees 2..4 and row degrees 5..6
and takes bp_irregular_kernel.  The rows of a block row have pairwise disjoint
columns, and consecutive block rows share a base column, so the greedy layers
are the 4 block rows of 200 rows: two full passes of 96 rows and a partial one
of 8.  The shifts are drawn until the matrix has full rank and no 4-cycles.
"""
import gzip
import os
import sys

import numpy as np

from make_codes import gf2_rank

HERE = os.path.dirname(os.path.abspath(__file__))
DATA = os.path.join(HERE, "data")
NAME = "syn_qc_l200"
SEED = 200
Z = 200
BASE = np.array([[1, 1, 1, 1, 1, 0, 1, 0],
                 [1, 1, 1, 0, 0, 1, 0, 1],
                 [1, 1, 0, 1, 1, 1, 1, 0],
                 [1, 1, 1, 1, 0, 0, 0, 1]], np.int64)


def has_4cycle(shift):
    """Two base rows a, b and two base columns c, d close a 4-cycle when s[a,c] - s[b,c] = s[a,d] - s[b,d] mod Z."""
    R, C = BASE.shape
    for a in range(R):
        for b in range(a + 1, R):
            both = np.nonzero(BASE[a] & BASE[b])[0]
            diff = (shift[a, both] - shift[b, both]) % Z
            if len(set(diff.tolist())) != len(diff):
                return True
    return False


def make():
    rng = np.random.default_rng(SEED)
    R, C = BASE.shape
    M, N = R * Z, C * Z
    assert sorted(BASE.sum(axis=0).tolist()) == [2, 2, 2, 2, 3, 3, 4, 4] and BASE.sum(axis=1).tolist() == [6, 5, 6, 5]
    for _ in range(1000):
        shift = rng.integers(0, Z, BASE.shape)
        if has_4cycle(shift):
            continue
        br, bc = np.nonzero(BASE)
        i = np.arange(Z)
        rows = (br[:, None] * Z + i[None, :]).reshape(-1)
        cols = (bc[:, None] * Z + (i[None, :] + shift[br, bc][:, None]) % Z).reshape(-1)
        if gf2_rank(rows, cols, M, N) == M:
            break
    else:
        raise RuntimeError("no full-rank draw")
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    row_deg = np.bincount(rows, minlength=M)
    lines = ["num_of_row--num_of_col--rank_of_H", f"{M}\t{N}\t{M}", "no_of_row--degree_of_row--no_of_col"]
    ptr = np.concatenate([[0], np.cumsum(row_deg)])
    for r in range(M):
        cs = cols[ptr[r]:ptr[r + 1]]
        lines.append(f"{r} {len(cs)} " + " ".join(str(int(c)) for c in cs) + " ")
    return ("\n".join(lines) + "\n").encode(), dict(M=M, N=N, E=len(rows), rank=M)


def main():
    raw, info = make()
    path = os.path.join(DATA, NAME + ".txt.gz")
    if "--check" in sys.argv:
        with gzip.open(path, "rb") as g:
            assert g.read() == raw, f"{NAME}: committed file differs"
    else:
        with gzip.GzipFile(path, "wb", mtime=0) as g:
            g.write(raw)
    print(NAME, info, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
