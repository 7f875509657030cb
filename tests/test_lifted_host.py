"""The lifted BG2 codes (tests/golden/make_codes_lifted.py) on a host-only
context: the committed file is what its generator says, the loader sees a 5G code
of the expected shape, and kml_code_layers answers for these "layered-only"
codes, whose N = 22 Z is past bp_irregular_kernel's round plan, as it does on a
GPU context.  The codes that had no layer plan still have none."""
import os
import subprocess
import sys

import numpy as np
import pytest

import lifted_codes as LC
from bp_lnms_model import layers
from conftest import GOLDEN

import kmldpc_amd as K


def test_generator_check():
    p = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_codes_lifted.py"), "--check"], capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-1000:] + p.stderr[-1000:]
    assert "'M': 1536, 'N': 2816, 'E': 9856" in p.stdout


@pytest.mark.parametrize("Z", [128, 288])
def test_host_context_shape_and_layers(data_dir, tmp_path, Z):
    ctx = K.Context(device=-1, **LC.ctx_args(data_dir, Z, tmp_path))
    _, g = LC.graph(data_dir, Z, tmp_path)
    assert (ctx.M, ctx.Ncol, ctx.E, ctx.Z) == (12 * Z, 22 * Z, 77 * Z, Z)
    assert (ctx.K, ctx.cc_len, ctx.chk) == (10 * Z, 20 * Z, 12 * Z)  # rank M
    assert (g.M, g.N, g.E, g.K, g.cc_len) == (ctx.M, ctx.Ncol, ctx.E, ctx.K, ctx.cc_len)
    assert np.array_equal(ctx.perm(), np.arange(ctx.Ncol))
    dv, dc = np.diff(g.cp), np.diff(g.rp)
    assert 1 <= dv.min() and dv.max() <= 9 and 2 <= dc.min() and dc.max() <= 10
    assert 22 * Z > 2304  # past the round plan of bp_irregular_kernel: a layered-only code
    lp = ctx.layers()  # (KML_E_UNSUP before these codes were taken)
    assert lp.dtype == np.int32 and np.array_equal(lp, layers(g))
    assert lp.tolist() == list(range(0, 12 * Z + 1, Z))
    assert K.lib().kml_code_layers(ctx._h, None, 0) == 12
    # the min-sum mode itself still needs a GPU
    with pytest.raises(K.KmlError, match=r"\(code -4\)"):
        ctx.set_algorithm("nms")
    assert "host-only" in K.lib().kml_last_error(ctx._h).decode()
    assert ctx.algorithm[0] == "spa" and ctx.schedule == "flooding"
    ctx.close()


@pytest.mark.parametrize("matrix", ["PEG2304regular0.5.txt", "syn_reg36_192.txt", "syn_high120.txt"])
def test_codes_that_still_have_no_plan(data_dir, matrix):
    ctx = K.Context(matrix_file=os.path.join(data_dir, matrix), modem_file=os.path.join(data_dir, "2bits_QPSK.txt"),
                    device=-1)
    assert K.lib().kml_code_layers(ctx._h, None, 0) == -4  # KML_E_UNSUP
    ctx.close()


def test_a_code_past_one_cu_has_no_plan(data_dir, tmp_path):
    """Z = 416: the posteriors and messages alone (4 N + 4 E = 164,736 bytes) exceed one CU's 163,840 bytes of LDS."""
    Z = 416
    assert 4 * 22 * Z + 4 * 77 * Z > 160 * 1024 >= 4 * 22 * 384 + 4 * 77 * 384
    ctx = K.Context(device=-1, **LC.ctx_args(data_dir, Z, tmp_path))
    assert (ctx.K, ctx.cc_len) == (10 * Z, 20 * Z)
    assert K.lib().kml_code_layers(ctx._h, None, 0) == -4
    ctx.close()
