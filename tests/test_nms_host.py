"""The normalized min-sum mode's public interface on a host-only context: the
symbols exist, arguments are checked, and the mode is refused, never silently accepted."""
import math
import os

import pytest

import kmldpc_amd as K

BG2 = "5GLDPCBG2a3_R12_K960.txt"
MODEM = "4bit_16QAM_Gray.txt"


def host_ctx(data_dir, **kw):
    return K.Context(matrix_file=os.path.join(data_dir, BG2), modem_file=os.path.join(data_dir, MODEM), is5g=True,
                     max_iter=50, device=-1, **kw)


def test_symbols_and_abi_version():
    L = K.lib()
    for name in ("kml_set_algorithm", "kml_get_algorithm"):
        assert name in K.header_symbols()
        assert hasattr(L, name)
    assert L.kml_abi_version() == 2  # the change is additive
    assert K.ALGORITHMS == {"spa": 0, "nms": 1}


def test_host_only_context_refuses_nms(data_dir):
    ctx = host_ctx(data_dir)
    assert ctx.algorithm == ("spa", 0.75)
    with pytest.raises(K.KmlError, match=r"\(code -4\)"):  # KML_E_UNSUP
        ctx.set_algorithm("nms")
    assert "host-only" in K.lib().kml_last_error(ctx._h).decode()
    assert ctx.algorithm[0] == "spa"
    with pytest.raises(K.KmlError, match=r"\(code -4\)"):
        ctx.set_algorithm("nms", 0.8125)
    assert ctx.algorithm == ("spa", 0.75)
    ctx.set_algorithm("spa")  # the default is always accepted, whatever alpha says
    ctx.set_algorithm("spa", 7.0)
    assert K.lib().kml_set_algorithm(ctx._h, 0, float("nan")) == 0
    assert ctx.algorithm == ("spa", 0.75)
    ctx.close()


def test_bad_arguments(data_dir):
    ctx = host_ctx(data_dir)
    L = K.lib()
    for alpha in (-1.0, 1.5, float("nan"), float("inf"), -0.25, 1.0 + 2.0 ** -40):
        assert L.kml_set_algorithm(ctx._h, 1, alpha) == -1, alpha  # KML_E_ARG, ahead of the host-only refusal
    assert L.kml_set_algorithm(ctx._h, 7, 0.75) == -1
    assert L.kml_set_algorithm(ctx._h, -1, 0.0) == -1
    assert L.kml_set_algorithm(None, 1, 0.75) == -1
    assert L.kml_get_algorithm(None, None) == -1
    assert L.kml_get_algorithm(ctx._h, None) == 0  # alpha may be NULL
    with pytest.raises(K.KmlError, match=r"\(code -1\)"):
        ctx.set_algorithm("oms")
    with pytest.raises(K.KmlError, match=r"\(code -1\)"):
        ctx.set_algorithm("nms", 0.0)  # an explicit 0 is out of range in Python; only the C ABI reads it as "default"
    assert math.isclose(ctx.algorithm[1], 0.75) and ctx.algorithm[0] == "spa"
    ctx.close()


def test_constructor_keyword(data_dir):
    host_ctx(data_dir, algorithm="spa").close()
    for spec in ("nms", "nms:0.8125", "nms:1"):
        with pytest.raises(K.KmlError, match=r"\(code -4\)"):
            host_ctx(data_dir, algorithm=spec)
    with pytest.raises(K.KmlError, match=r"\(code -1\)"):
        host_ctx(data_dir, algorithm="nms:1.5")
    with pytest.raises(ValueError):  # a colon with no alpha, as the drivers refuse it
        host_ctx(data_dir, algorithm="nms:")
