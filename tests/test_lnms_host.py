"""The layered min-sum schedule's public interface on a host-only context: the
symbols exist, kml_code_layers gives the layers of the greedy rule, arguments are
checked, and the schedule is refused, never silently accepted."""
import ctypes as C
import os

import numpy as np
import pytest

from bp_lnms_model import layers
from test_bp_lnms_model import CODES, LAYERS, code

import kmldpc_amd as K


def host_ctx(data_dir, name="bg2", **kw):
    matrix, is5g, max_iter, modem, _ = CODES[name]
    return K.Context(matrix_file=os.path.join(data_dir, matrix), modem_file=os.path.join(data_dir, modem), is5g=is5g,
                     max_iter=max_iter, device=-1, **kw)


def test_symbols_and_abi_version():
    L = K.lib()
    for name in ("kml_set_schedule", "kml_get_schedule", "kml_code_layers"):
        assert name in K.header_symbols()
        assert hasattr(L, name)
    hdr = open(K.INCLUDE).read()
    assert "#define KML_SCHED_FLOODING 0" in hdr and "#define KML_SCHED_LAYERED 1" in hdr
    assert L.kml_abi_version() == 2  # the change is additive
    assert K.SCHEDULES == {"flooding": 0, "layered": 1}
    assert K.ALGORITHMS == {"spa": 0, "nms": 1}


@pytest.mark.parametrize("name", list(CODES))
def test_code_layers_equal_the_rule(data_dir, name):
    ctx = host_ctx(data_dir, name)
    _, g = code(data_dir, name)
    lp = ctx.layers()
    assert lp.dtype == np.int32 and np.array_equal(lp, layers(g))
    nl, lo, hi = LAYERS[name]
    sizes = np.diff(lp)
    assert (len(lp) - 1, int(sizes.min()), int(sizes.max())) == (nl, lo, hi)
    # cap: min(cap, nl + 1) entries are written, the count is returned whatever cap is
    L = K.lib()
    assert L.kml_code_layers(ctx._h, None, 0) == nl
    buf = np.full(nl + 4, -7, np.int32)
    assert L.kml_code_layers(ctx._h, buf.ctypes.data_as(C.c_void_p), 2) == nl
    assert buf[:2].tolist() == lp[:2].tolist() and np.all(buf[2:] == -7)
    assert L.kml_code_layers(ctx._h, buf.ctypes.data_as(C.c_void_p), nl + 4) == nl
    assert np.array_equal(buf[:nl + 1], lp) and np.all(buf[nl + 1:] == -7)
    assert L.kml_code_layers(ctx._h, None, 3) == -1 and L.kml_code_layers(ctx._h, None, -1) == -1
    assert L.kml_code_layers(None, None, 0) == -1
    ctx.close()


@pytest.mark.parametrize("matrix", ["PEG2304regular0.5.txt", "syn_reg36_192.txt", "syn_high120.txt"])
def test_codes_without_a_plan(data_dir, matrix):
    ctx = K.Context(matrix_file=os.path.join(data_dir, matrix), modem_file=os.path.join(data_dir, "2bits_QPSK.txt"),
                    device=-1)
    assert K.lib().kml_code_layers(ctx._h, None, 0) == -4  # KML_E_UNSUP
    with pytest.raises(K.KmlError, match=r"\(code -4\)"):
        ctx.layers()
    ctx.close()


def test_host_only_context_refuses_layered(data_dir):
    ctx = host_ctx(data_dir)
    assert ctx.schedule == "flooding"
    with pytest.raises(K.KmlError, match=r"\(code -4\)"):  # KML_E_UNSUP
        ctx.set_schedule("layered")
    assert "host-only" in K.lib().kml_last_error(ctx._h).decode()
    assert ctx.schedule == "flooding"
    ctx.set_schedule("flooding")  # the default is always accepted
    assert K.lib().kml_set_schedule(ctx._h, 0) == 0
    assert ctx.schedule == "flooding" and ctx.algorithm == ("spa", 0.75)
    ctx.close()


def test_bad_arguments(data_dir):
    ctx = host_ctx(data_dir)
    L = K.lib()
    for v in (2, -1, 7, 1 << 20):
        assert L.kml_set_schedule(ctx._h, v) == -1, v  # KML_E_ARG, ahead of the host-only refusal
    assert L.kml_set_schedule(None, 0) == -1
    assert L.kml_get_schedule(None) == -1
    assert L.kml_get_schedule(ctx._h) == 0
    with pytest.raises(K.KmlError, match=r"\(code -1\)"):
        ctx.set_schedule("serial")
    assert ctx.schedule == "flooding"
    ctx.close()


def test_constructor_keyword(data_dir):
    host_ctx(data_dir, schedule="flooding").close()
    with pytest.raises(K.KmlError, match=r"\(code -4\)"):
        host_ctx(data_dir, schedule="layered")
    with pytest.raises(K.KmlError, match=r"\(code -4\)"):  # the algorithm's refusal comes first
        host_ctx(data_dir, algorithm="nms", schedule="layered")
    with pytest.raises(K.KmlError, match=r"\(code -1\)"):
        host_ctx(data_dir, schedule="zigzag")
