"""The single-precision BP mode on a host-only context: refused, never silently accepted."""
import os

import pytest

import kmldpc_amd as K


def test_host_only_context_refuses_f32(data_dir):
    ctx = K.Context(matrix_file=os.path.join(data_dir, "PEG2304regular0.5.txt"),
                    modem_file=os.path.join(data_dir, "2bits_QPSK.txt"), device=-1)
    assert ctx.precision == "f64"
    with pytest.raises(K.KmlError, match=r"\(code -4\)"):  # KML_E_UNSUP
        ctx.set_precision("f32")
    assert "host-only" in K.lib().kml_last_error(ctx._h).decode()
    assert ctx.precision == "f64"
    ctx.set_precision("f64")  # the default is always accepted
    with pytest.raises(K.KmlError, match=r"\(code -1\)"):  # KML_E_ARG
        ctx.set_precision("f16")
    with pytest.raises(K.KmlError, match=r"\(code -4\)"):
        K.Context(matrix_file=os.path.join(data_dir, "PEG2304regular0.5.txt"),
                  modem_file=os.path.join(data_dir, "2bits_QPSK.txt"), device=-1, precision="f32")
    ctx.close()
