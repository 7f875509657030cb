"""The LLR front end's public interface on a host-only context: the symbols
exist, arguments are checked, and every entry point that needs the min-sum
decoder is refused with a reason, never silently accepted."""
import ctypes as C

import numpy as np
import pytest

from test_lnms_host import host_ctx

import kmldpc_amd as K

UNSUP = r"\(code -4\)"
ptr = lambda a: a.ctypes.data_as(C.c_void_p)


def test_symbols_and_abi_version():
    L = K.lib()
    for name in ("kml_set_demapper", "kml_get_demapper", "kml_demap_llr", "kml_llr_decode"):
        assert name in K.header_symbols()
        assert hasattr(L, name)
    hdr = open(K.INCLUDE).read()
    assert "#define KML_DEMAP_EXACT 0" in hdr and "#define KML_DEMAP_MAXLOG 1" in hdr
    assert L.kml_abi_version() == 2  # the change is additive
    assert K.DEMAPPERS == {"exact": 0, "maxlog": 1}
    assert K.SCHEDULES == {"flooding": 0, "layered": 1}
    assert K.ALGORITHMS == {"spa": 0, "nms": 1}
    for name in ("demap_llr", "llr_decode", "set_demapper", "demapper"):
        assert hasattr(K.Context, name)


def test_host_only_context_refuses_maxlog(data_dir):
    ctx = host_ctx(data_dir)
    assert ctx.demapper == "exact"
    with pytest.raises(K.KmlError, match=UNSUP):
        ctx.set_demapper("maxlog")
    assert "host-only" in K.lib().kml_last_error(ctx._h).decode()
    assert ctx.demapper == "exact"
    ctx.set_demapper("exact")  # the default is always accepted
    assert K.lib().kml_set_demapper(ctx._h, 0) == 0
    assert ctx.demapper == "exact" and ctx.schedule == "flooding" and ctx.algorithm == ("spa", 0.75)
    ctx.close()


def test_host_only_context_refuses_the_entry_points(data_dir):
    ctx = host_ctx(data_dir)
    y = np.zeros((2, ctx.S, 2))
    h = np.ones((2, 2))
    with pytest.raises(K.KmlError, match=UNSUP):
        ctx.demap_llr(y, h, 0.2)
    assert "host-only" in K.lib().kml_last_error(ctx._h).decode()
    with pytest.raises(K.KmlError, match=UNSUP):
        ctx.llr_decode(np.zeros((2, ctx.cc_len), np.float32))
    assert "host-only" in K.lib().kml_last_error(ctx._h).decode()
    with pytest.raises(K.KmlError, match=UNSUP):
        ctx.llr_decode(np.zeros((2, ctx.cc_len), np.float32), cc_hat=True, llr_out=True)
    ctx.close()


def test_bad_arguments(data_dir):
    ctx = host_ctx(data_dir)
    L = K.lib()
    for v in (2, -1, 7, 1 << 20):
        assert L.kml_set_demapper(ctx._h, v) == -1, v  # KML_E_ARG, ahead of the host-only refusal
    assert L.kml_set_demapper(None, 0) == -1
    assert L.kml_get_demapper(None) == -1
    assert L.kml_get_demapper(ctx._h) == 0
    with pytest.raises(K.KmlError, match=r"\(code -1\)"):
        ctx.set_demapper("approx")
    assert ctx.demapper == "exact"
    y, h = np.zeros((1, ctx.S, 2)), np.ones((1, 2))
    llr = np.zeros((1, ctx.cc_len), np.float32)
    uh = np.zeros((1, ctx.K), np.uint8)
    # KML_E_ARG ahead of the host-only refusal: NULL pointers, B < 0, var not > 0, iter_count < 0
    assert L.kml_demap_llr(None, ptr(y), ptr(h), 0.2, 1, ptr(llr), 0) == -1
    assert L.kml_demap_llr(ctx._h, None, ptr(h), 0.2, 1, ptr(llr), 0) == -1
    assert L.kml_demap_llr(ctx._h, ptr(y), None, 0.2, 1, ptr(llr), 0) == -1
    assert L.kml_demap_llr(ctx._h, ptr(y), ptr(h), 0.2, 1, None, 0) == -1
    assert L.kml_demap_llr(ctx._h, ptr(y), ptr(h), 0.2, -1, ptr(llr), 0) == -1
    for var in (0.0, -1.0, float("nan")):
        assert L.kml_demap_llr(ctx._h, ptr(y), ptr(h), var, 1, ptr(llr), 0) == -1, var
    assert L.kml_llr_decode(None, ptr(llr), 1, 5, ptr(uh), None, None, None, 0) == -1
    assert L.kml_llr_decode(ctx._h, None, 1, 5, ptr(uh), None, None, None, 0) == -1
    assert L.kml_llr_decode(ctx._h, ptr(llr), -1, 5, ptr(uh), None, None, None, 0) == -1
    assert L.kml_llr_decode(ctx._h, ptr(llr), 1, -1, ptr(uh), None, None, None, 0) == -1
    # with good arguments the same calls are refused, not run
    assert L.kml_demap_llr(ctx._h, ptr(y), ptr(h), 0.2, 1, ptr(llr), 0) == -4
    assert L.kml_llr_decode(ctx._h, ptr(llr), 1, 5, ptr(uh), None, None, None, 0) == -4
    ctx.close()


def test_constructor_keyword(data_dir):
    host_ctx(data_dir, demapper="exact").close()
    with pytest.raises(K.KmlError, match=UNSUP):
        host_ctx(data_dir, demapper="maxlog")
    with pytest.raises(K.KmlError, match=UNSUP):  # the algorithm's refusal comes first
        host_ctx(data_dir, algorithm="nms", demapper="maxlog")
    with pytest.raises(K.KmlError, match=r"\(code -1\)"):
        host_ctx(data_dir, demapper="approx")
