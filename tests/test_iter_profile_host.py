"""Host side of kml_sim_decode_profile: the entry point exists and refuses
without a GPU, and the premise it rests on holds in the reference arithmetic
(the oracle): the iteration budget only bounds BinaryLDPCCodec::Decoder's loop,
so a decode with budget k returns the decisions of iteration min(k - 1, c) of
the one trajectory, c the first iteration whose parity check passes."""
import os

import numpy as np
import pytest

from oracle import oracle as O

import kmldpc_amd as K

KML_E_ARG, KML_E_UNSUP = -1, -4


def test_header_declares_and_library_exports_the_entry_point():
    assert "kml_sim_decode_profile" in K.header_symbols()
    assert hasattr(K.lib(), "kml_sim_decode_profile")
    assert K.lib().kml_abi_version() == 2  # additive


def test_host_only_context_is_refused(data_dir):
    ctx = K.Context(matrix_file=os.path.join(data_dir, "PEG2304regular0.5.txt"),
                    modem_file=os.path.join(data_dir, "2bits_QPSK.txt"), max_iter=8, device=-1)
    prof = np.zeros((8, 3), np.uint64)
    r = K.lib().kml_sim_decode_profile(ctx._h, 2.0, 0, K._p(prof), None, None)
    assert r == KML_E_UNSUP
    assert "host-only" in K.lib().kml_last_error(ctx._h).decode()
    with pytest.raises(K.KmlError, match="host-only"):
        ctx.sim_decode_profile(2.0)
    ctx.close()


def test_null_context_is_an_argument_error():
    assert K.lib().kml_sim_decode_profile(None, 2.0, 0, None, None, None) == KML_E_ARG


@pytest.mark.parametrize("matrix,modem,is5g,snr", [("PEG2304regular0.5.txt", "2bits_QPSK.txt", False, 2.0),
                                                   ("5GLDPCBG2a3_R12_K960.txt", "4bit_16QAM_Gray.txt", True, 9.0)])
def test_budget_only_bounds_the_loop(data_dir, matrix, modem, is5g, snr):
    """uu_hat and ret of O.Code(..., max_iter=k), k = 1..6, from one budget-6
    code: its decisions after each iteration, its return value and the parity
    of its final decisions.  ret = iter + (iter < max_iter)."""
    P, n = 6, 32
    oc = {k: O.Code(os.path.join(data_dir, matrix), is5g, True, False, k) for k in range(1, P + 1)}
    om = O.Modem(os.path.join(data_dir, modem))
    uu, _, th, y = O.gen_frames(oc[P], om, snr, n)
    var = 10.0 ** (-0.1 * snr)
    seen = set()
    for i in range(n):
        p0 = om.demap(y[i], th[i], var)
        # the budget-6 code's decisions after iteration j (its loop cut at j + 1), and its own decode
        dec = [oc[P].bp_decode(p0, j + 1)[1] for j in range(P)]
        ret6, uh6, cch6, _ = oc[P].bp_decode(p0)
        assert np.array_equal(uh6, dec[P - 1])
        c = ret6 - 1 if oc[P].parity_count(cch6) == 0 else None  # first passing iteration (None: not within 6)
        seen.add(c)
        for k in range(1, P + 1):
            ret, uh, _, _ = oc[k].bp_decode(p0)
            conv = c is not None and c <= k - 1
            last = c if conv else k - 1
            assert np.array_equal(uh, dec[last]), (i, k)
            assert ret == (c + 1 if conv else k), (i, k)
    assert None in seen and len(seen) > 2  # exhausted budgets and several converging iterations
