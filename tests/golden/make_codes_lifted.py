"""Generate tests/golden/data/syn_bg2_z128.txt.gz, and build its larger siblings
on demand: the R = 1/2 structure of the committed 5G BG2 code
(5GLDPCBG2a3_R12_K960, a 12 x 22 base graph of 96 x 96 circulants) lifted to
another circulant size Z.  The layered min-sum kernels take these codes where
bp_irregular_kernel's round plan no longer fits (N = 22 Z > 2304).

PROVENANCE ONLY for the committed file: the tests never regenerate it.  The
larger codes (Z = 288, 384, 416) are NOT committed: the tests build them into a
temporary directory with lifted(Z).  numpy with a fixed seed per Z.

    python tests/golden/make_codes_lifted.py          # writes syn_bg2_z128.txt.gz
    python tests/golden/make_codes_lifted.py --check  # regenerates in memory, compares with the committed file

lifted(Z):
  * the base graph and the shifts are read out of the committed K960 file:
    every block is a circulant, row i of a block with shift s holds column
    (i + s) mod 96;
  * the shifts of base columns 10..21 (the parity part: 0s and one 1) are kept,
    so the parity part keeps its dual-diagonal structure and rank M for any Z;
  * the shift of every present entry in base columns 0..9 is drawn anew with
    np.random.default_rng(Z).integers(0, Z), base rows ascending and, within a
    row, base columns ascending;
  * the output is the reference's 5G file format: four header numbers, the last
    one Z.
These are synthetic test codes with BG2's degrees and layer structure, not the
3GPP lifting of BG2 for that Z.  N = 22 Z, M = 12 Z, E = 77 Z; the first 2 Z
columns are punctured, K = 10 Z, cc_len = 20 Z; 12 greedy layers of Z rows.
"""
import gzip
import os
import sys

import numpy as np

from make_codes import gf2_rank

HERE = os.path.dirname(os.path.abspath(__file__))
DATA = os.path.join(HERE, "data")
BASE_FILE = "5GLDPCBG2a3_R12_K960.txt.gz"
BASE_Z = 96
NAME = "syn_bg2_z128"
COMMITTED_Z = 128
INFO_COLS = 10  # base columns 0..9 are redrawn, 10..21 (parity) keep their shifts


def base_graph(path=None):
    """[(base row, base column, shift), ...] of the committed K960 file, base rows then base columns ascending."""
    with gzip.open(path or os.path.join(DATA, BASE_FILE), "rt") as f:
        tok = f.read().split()
    M, N, rank, z = (int(x) for x in tok[1:5])
    assert z == BASE_Z and M % z == 0 and N % z == 0 and rank == M
    pos = 6
    rows = []
    for r in range(M):
        assert int(tok[pos]) == r
        d = int(tok[pos + 1])
        rows.append([int(x) for x in tok[pos + 2:pos + 2 + d]])
        pos += 2 + d
    assert pos == len(tok)
    out = []
    for bi in range(M // z):
        first = rows[bi * z]
        for c in sorted(first):
            bj = c // z
            s = c % z
            for k in range(z):  # every block is a circulant
                assert bj * z + (k + s) % z in rows[bi * z + k]
            out.append((bi, bj, s))
        assert all(len(rows[bi * z + k]) == len(first) for k in range(z))
    assert sum(len(r) for r in rows) == len(out) * z
    return out, M // z, N // z


def lifted(Z, path=None):
    """(file bytes, dict(M, N, E, Z)) of the structure lifted to circulants of size Z."""
    base, R, C = base_graph(path)
    rng = np.random.default_rng(Z)
    lines = ["num_of_row--num_of_col--rank_of_H ", f"{R * Z}      {C * Z}      {R * Z}    {Z}",
             "no_of_row--degree_of_row--no_of_col "]
    blocks = [[] for _ in range(R)]
    for bi, bj, s in base:
        if bj < INFO_COLS:
            s = int(rng.integers(0, Z))
        assert 0 <= s < Z
        blocks[bi].append((bj, s))
    E = 0
    for bi in range(R):
        for k in range(Z):
            cs = sorted(bj * Z + (k + s) % Z for bj, s in blocks[bi])
            E += len(cs)
            lines.append(f"{bi * Z + k}    {len(cs)}    " + " ".join(str(c) for c in cs) + " ")
    return ("\n".join(lines) + "\n").encode(), dict(M=R * Z, N=C * Z, E=E, Z=Z)


def edges(raw):
    """(rows, cols, M, N) of a file's bytes, for gf2_rank."""
    tok = raw.decode().split()
    M, N = int(tok[1]), int(tok[2])
    pos, rr, cc = 6, [], []
    for r in range(M):
        d = int(tok[pos + 1])
        rr += [r] * d
        cc += [int(x) for x in tok[pos + 2:pos + 2 + d]]
        pos += 2 + d
    return np.array(rr), np.array(cc), M, N


def write(Z, directory, name=None):
    """Write the lifted code as plain text into a directory (the tests' temporary ones); returns the path."""
    raw, _ = lifted(Z)
    path = os.path.join(directory, name or f"syn_bg2_z{Z}.txt")
    with open(path, "wb") as f:
        f.write(raw)
    return path


def main():
    raw, info = lifted(COMMITTED_Z)
    assert info == dict(M=1536, N=2816, E=9856, Z=128)
    rows, cols, M, N = edges(raw)
    assert gf2_rank(rows, cols, M, N) == M
    par = cols >= INFO_COLS * COMMITTED_Z  # the parity part alone has rank M
    assert gf2_rank(rows[par], cols[par] - INFO_COLS * COMMITTED_Z, M, N - INFO_COLS * COMMITTED_Z) == M
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
