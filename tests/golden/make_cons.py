"""Generate the synthetic constellation files tests/golden/data/syn_*bit*.txt.gz.

PROVENANCE ONLY: the outputs are committed and the tests never regenerate
them.  The reference ships 2-, 4- and 6-bit constellations only; these three
are our own, in the on-disk format its reader parses (three header tokens with
the two counts between them, then per point: index, label bits MSB first, re,
im), so that the 1- and 3-bit instances of the front end run against it.

    python tests/golden/make_cons.py          # writes every file
    python tests/golden/make_cons.py --check  # regenerates in memory, compares with the committed files

What each constellation is for:
  syn_1bit_BPSK         +1 and -1: two k-means clusters, so cluster 0 holds
                        about S/2 symbols on every ordinary frame (past
                        km_wave_kernel's member list); every per-bit loop of
                        the demapper runs once; S = N symbols per codeword
  syn_3bits_8PSK_Gray   eight unit-circle points at multiples of 45 degrees,
                        Gray-labelled around the circle: KC = 8 on the
                        compacted member list, hard_bits_screen<3>
  syn_3bits_star8       two rings of four: radius 1 (labels 0-3) and 2.2
                        (labels 4-7, turned by 45 degrees), energy not
                        normalised in the file (the loader's / sqrt(energy)
                        does real work), point 0 not of largest modulus
                        (h_hat = centre 0 / point 0, the metric screen's bound)
"""
import gzip
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
DATA = os.path.join(HERE, "data")


def unit(deg):
    """cos / sin of a multiple of 45 degrees: exact on the axes, +-sqrt(1/2) on
    the diagonals (the same double in all four quadrants)."""
    r = math.sqrt(0.5)
    return [(1.0, 0.0), (r, r), (0.0, 1.0), (-r, r), (-1.0, 0.0), (-r, -r), (0.0, -1.0), (r, -r)][deg // 45 % 8]


def bpsk():
    return 1, [(1.0, 0.0), (-1.0, 0.0)]


def psk8_gray():
    pts = [None] * 8
    for k in range(8):  # position k around the circle carries label k ^ (k >> 1)
        pts[k ^ (k >> 1)] = unit(45 * k)
    return 3, pts


def star8():
    inner = [unit(90 * k) for k in range(4)]
    outer = [tuple(2.2 * v for v in unit(90 * k + 45)) for k in range(4)]
    return 3, inner + outer


CONS = {"syn_1bit_BPSK": bpsk, "syn_3bits_8PSK_Gray": psk8_gray, "syn_3bits_star8": star8}


def make(name):
    bits, pts = CONS[name]()
    assert len(pts) == 1 << bits
    lines = ["number_of_bits_per_constellation_point", str(bits), "number_of_symbols_per_constallation_point", "2",
             '"decimal_expression"____"binary_expression"____"symbol(real_image_..._real_image)"']
    for i, (re, im) in enumerate(pts):
        lab = " ".join(str((i >> (bits - 1 - j)) & 1) for j in range(bits))
        lines.append(f"{i}   {lab}   {re!r}   {im!r}")
    return ("\n".join(lines) + "\n").encode()


def main():
    check = "--check" in sys.argv
    for name in CONS:
        raw = make(name)
        path = os.path.join(DATA, name + ".txt.gz")
        if check:
            with gzip.open(path, "rb") as g:
                assert g.read() == raw, f"{name}: committed file differs"
        else:
            with gzip.GzipFile(path, "wb", mtime=0) as g:
                g.write(raw)
        print(name, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
