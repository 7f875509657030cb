"""The 1- and 3-bit constellation paths where the widened lists of
test_gpu_parity.py do not reach: k-means cluster 0 on both sides of
km_wave_kernel's member list capacity, the native S > 4096 k-means route, and
the two refusals of kml_create that concern the constellation.  Run on an
MI355X with -m gpu.  Everything is bit-exact against the oracle.
"""
import os

import numpy as np
import pytest

from conftest import load_case
from oracle import oracle as O

import kmldpc_amd as K

pytestmark = pytest.mark.gpu

BPSK, QPSK, PSK8 = "syn_1bit_BPSK.txt", "2bits_QPSK.txt", "syn_3bits_8PSK_Gray.txt"
WATERFALL = {BPSK: 0.5, QPSK: 2.0}  # dB, the SNRs of the reference fixtures

_ctx = {}


def list_capacity(S):
    """The cluster-0 member list of km_wave_kernel (kmeans.hip km_wave_lds: cap)."""
    return ((S + 2) // 3 + 7) & ~7


def write_chain_h(path, M):
    """An M x 2M parity-check matrix of full rank (a cycle beside an identity
    block): k-means reads the code only for S = 2M / bits."""
    with open(path, "w") as f:
        f.write(f"num_of_row--num_of_col--rank_of_H\n{M}\t{2 * M}\t{M}\nno_of_row--degree_of_row--no_of_col\n")
        for r in range(M):
            cols = sorted({r, (r + 1) % M, M + r})
            f.write(f"{r} {len(cols)} " + " ".join(map(str, cols)) + " \n")


def kmeans_ctx(data_dir, tmp_path_factory, modem, S):
    """A context whose frames hold S symbols of `modem`."""
    key = (modem, S)
    if key not in _ctx:
        shipped = {(BPSK, 192): "syn_reg36_192.txt", (BPSK, 2304): "PEG2304regular0.5.txt"}
        if key in shipped:
            matrix = os.path.join(data_dir, shipped[key])
        else:  # no committed code has N = 2 S
            matrix = str(tmp_path_factory.mktemp("chain") / f"chain{S}.txt")
            write_chain_h(matrix, S)
        _ctx[key] = K.Context(matrix_file=matrix, modem_file=os.path.join(data_dir, modem), max_iter=20, device=0)
        assert _ctx[key].S == S
    return _ctx[key]


def capacity_frames(pts, S, snr_waterfall):
    """Frames with a chosen number n0 of point-0 symbols (the rest spread over the
    other points, positions shuffled) at 40 dB under a random channel, two
    channels per n0; then two frames of n0 = S // 2 at the waterfall SNR.  One
    point-0 symbol is sent at 1.5 (noisy frames: 6) times the amplitude, so that KMeans::Run's
    first estimate (largest symbol / point 0) starts from the true rotation and
    cluster 0 is point 0's.  Returns y[B][S][2] and, per frame, whether its
    final cluster 0 must fit the list (count <= cap) or exceed it.

    For at most four points the list holds per-word segments, each with one
    slot of slack, so the kernel's own boundary lies Sw = ceil(S / 64) lower:
    cap - Sw members fit, cap - Sw + 1 do not; both are below cap."""
    cap, Sw = list_capacity(S), (S + 63) // 64
    rng = np.random.default_rng(1000 + S + len(pts))
    kinds = [(cap - Sw, True), (cap - Sw + 1, True), (cap - 1, True), (cap, True), (cap + 1, False), (S // 2, False),
             (S, False)]
    ys, fits = [], []
    for n0, fit in kinds + [(S // 2, False)]:
        noisy = len(ys) == 2 * len(kinds)
        for _ in range(2):
            h = rng.uniform(0.5, 2.0) * np.exp(2j * np.pi * rng.random())
            lab = np.concatenate([np.zeros(n0, np.int64), rng.integers(1, len(pts), S - n0)])
            lab = lab[rng.permutation(S)]
            amp = np.ones(S)
            amp[np.flatnonzero(lab == 0)[0]] = 6.0 if noisy else 1.5  # above the largest noisy symbol
            sigma = np.sqrt(10.0 ** (-0.1 * (snr_waterfall if noisy else 40.0)) / 2) * (abs(h) if noisy else 1.0)
            z = amp * pts[lab] * h + sigma * (rng.normal(size=S) + 1j * rng.normal(size=S))
            ys.append(np.stack([z.real, z.imag], axis=1))
            fits.append(fit)
    return np.stack(ys), fits


_cap_ref = {}


def capacity_reference(om, S, modem):
    """The frames, and the oracle's h_hat / rotations / final cluster-0 counts, computed once."""
    key = (modem, S)
    if key not in _cap_ref:
        y, fits = capacity_frames(om.points.reshape(-1, 2) @ [1, 1j], S, WATERFALL[modem])
        hh = np.stack([O.kmeans_hhat(f, om.points) for f in y])
        n0 = np.array([int((O.kmeans_state(f, om.points)[1] == 0).sum()) for f in y])
        for a in (y, hh, n0):
            a.setflags(write=False)
        _cap_ref[key] = (y, fits, hh, n0)
    return _cap_ref[key]


@pytest.mark.parametrize("mode", ["wave", "wave_sequential_sum", "wave_every_word", "split"])
@pytest.mark.parametrize("S", [192, 2304])
@pytest.mark.parametrize("modem", [BPSK, QPSK])
def test_cluster0_on_both_sides_of_the_list_capacity(data_dir, tmp_path_factory, modem, S, mode, monkeypatch):
    """km_wave_kernel sums cluster 0 from its LDS value list while the members fit
    (cap = ((S + 2) / 3 + 7) & ~7 values) and straight from the membership words
    when they do not: frames whose final cluster 0 holds cap - 1, cap, cap + 1,
    S / 2 and S symbols (and the segment list's own boundary below cap), and
    noisy frames of about S / 2.  The precondition (which side of cap the
    oracle's final cluster 0 lies on) is asserted first; then h_hat and its
    four rotations equal the oracle bit for bit, in the four modes of
    test_kmeans_cumulative_sum_adversarial."""
    om = O.Modem(os.path.join(data_dir, modem))
    y, fits, hh_ref, n0 = capacity_reference(om, S, modem)
    cap = list_capacity(S)
    for b, fit in enumerate(fits):
        assert (n0[b] <= cap) == fit, (b, int(n0[b]), cap)
    assert {int(v) for v in n0} >= {cap - 1, cap, cap + 1, S}
    monkeypatch.setenv("KML_KMEANS", mode.split("_")[0])
    monkeypatch.setenv("KML_KM_SCAN", "0" if mode.endswith("sequential_sum") else "1")
    monkeypatch.setenv("KML_KM_INCR", "0" if mode.endswith("every_word") else "1")
    ctx = kmeans_ctx(data_dir, tmp_path_factory, modem, S)
    hh, h4 = ctx.kmeans(y)
    for b in range(y.shape[0]):
        assert np.array_equal(hh[b], hh_ref[b]), (b, int(n0[b]))
        assert np.array_equal(h4[b], O.rotations(hh_ref[b])), (b, int(n0[b]))


@pytest.mark.parametrize("matrix,n", [("syn_reg36_192.txt", 64), ("PEG2304regular0.5.txt", 64),
                                      ("syn_reg36_4080.txt", 24)])
def test_ordinary_bpsk_frames_overflow_the_member_list(data_dir, matrix, n):
    """With two points cluster 0 holds about S / 2 > cap symbols on EVERY
    ordinary frame (the streams of test_kmeans_vs_oracle's BPSK rows): the
    sum-from-the-words branch is BPSK's everyday path, here with the one-wave
    kernel as it ships (S <= 4096; no override)."""
    oc = O.Code(os.path.join(data_dir, matrix), False, True, False, 20)
    om = O.Modem(os.path.join(data_dir, BPSK))
    _, _, _, y = O.gen_frames(oc, om, 0.5, n)
    S = y.shape[1]
    counts = [int((O.kmeans_state(f, om.points)[1] == 0).sum()) for f in y]
    assert min(counts) > list_capacity(S), (min(counts), list_capacity(S))
    ctx = K.Context(matrix_file=os.path.join(data_dir, matrix), modem_file=os.path.join(data_dir, BPSK), max_iter=20,
                    device=0)
    hh, _ = ctx.kmeans(y)
    cl, idx = ctx.kmeans_state(y)
    for b in range(n):
        assert np.array_equal(hh[b], O.kmeans_hhat(y[b], om.points)), b
        rc, ri = O.kmeans_state(y[b], om.points)
        assert np.array_equal(cl[b], rc) and np.array_equal(idx[b], ri), b
    ctx.close()


@pytest.mark.parametrize("matrix,S", [("syn_reg36_4160.txt", 4160), ("syn_reg36_4080.txt", 4080)])
def test_kmeans_route_around_4096_symbols(data_dir, matrix, S, monkeypatch):
    """S = 4160 is the smallest case past the one-wave kernel's 4096 symbols
    (kmeans.hip kMaxS): the launcher takes the two-launch form on its own, and
    must do so under KML_KMEANS=wave too.  S = 4080 fills all 64 lane-words, the
    last one partly, and "wave" is the wave kernel.  With the override unset,
    "wave" and "split", h_hat and its rotations are identical and equal the
    oracle, on 12 frames."""
    ctx = K.Context(matrix_file=os.path.join(data_dir, matrix), modem_file=os.path.join(data_dir, BPSK), max_iter=20,
                    device=0)
    assert ctx.S == S
    oc = O.Code(os.path.join(data_dir, matrix), False, True, False, 20)
    om = O.Modem(os.path.join(data_dir, BPSK))
    _, _, _, y = O.gen_frames(oc, om, 0.5, 12, state=83)
    ref = np.stack([O.kmeans_hhat(f, om.points) for f in y])
    for mode in (None, "wave", "split"):
        if mode is None:
            monkeypatch.delenv("KML_KMEANS", raising=False)
        else:
            monkeypatch.setenv("KML_KMEANS", mode)
        hh, h4 = ctx.kmeans(y)
        assert np.array_equal(hh, ref), mode
        for b in range(12):
            assert np.array_equal(h4[b], O.rotations(ref[b])), (mode, b)
    ctx.close()


def _decodes_a_golden_case(data_dir):
    """A fresh context after a refusal: the reference's blind BPSK stream on syn_reg36_192."""
    hdr, z = load_case("syn_reg36_192_bpsk_blind")
    ctx = K.Context(matrix_file=os.path.join(data_dir, hdr["matrix"]), modem_file=os.path.join(data_dir, hdr["modem"]),
                    max_iter=hdr["max_iter"], device=0)
    nv = z["v_y"].shape[0]
    r = ctx.decode_frames(z["v_y"], hdr["snr"], None)
    assert np.array_equal(r["uu_hat"], z["v_uu_hat"])
    assert np.array_equal(r["ret"], z["s_ret"][:nv]) and np.array_equal(r["chosen"], z["s_chosen"][:nv])
    assert np.array_equal(r["h_hat"], z["s_hhat"][:nv]) and np.array_equal(r["metrics"], z["s_metrics"][:nv])
    ctx.close()


def test_five_bit_constellation_is_refused(data_dir, tmp_path):
    """A well-formed 5-bit, 32-point file (on a code whose length 5 divides):
    KML_E_UNSUP with the bits-per-symbol message; the next context is sound."""
    with open(tmp_path / "5bits_32PSK.txt", "w") as f:
        f.write("number_of_bits_per_constellation_point\n5\nnumber_of_symbols_per_constallation_point\n2\n"
                '"decimal_expression"____"binary_expression"____"symbol(real_image_..._real_image)"\n')
        for i in range(32):
            lab = " ".join(str((i >> (4 - j)) & 1) for j in range(5))
            f.write(f"{i}   {lab}   {float(np.cos(2 * np.pi * i / 32))!r}   {float(np.sin(2 * np.pi * i / 32))!r}\n")
    with pytest.raises(K.KmlError, match=r"bits per symbol must be 1, 2, 3, 4 or 6 \(code -4\)"):
        K.Context(matrix_file=os.path.join(data_dir, "syn_high120.txt"), modem_file=str(tmp_path / "5bits_32PSK.txt"),
                  max_iter=20, device=0)
    _decodes_a_golden_case(data_dir)


def test_code_length_not_a_multiple_of_the_symbol_bits_is_refused(data_dir):
    """syn_reg36_4160 with 8PSK: 4160 % 3 = 2 (modemlinearsystem.cc:7-12):
    KML_E_ARG with the reference's message; the next context is sound."""
    with pytest.raises(K.KmlError, match=r"\(cc_len = 4160\) % \(input_len = 3\) != 0 \(code -1\)"):
        K.Context(matrix_file=os.path.join(data_dir, "syn_reg36_4160.txt"), modem_file=os.path.join(data_dir, PSK8),
                  max_iter=20, device=0)
    _decodes_a_golden_case(data_dir)
