"""The offset axis (kml_set_nms_offset) on a host-only context: the symbols exist,
the ABI version stays, the default is 0 and always accepted, a positive offset is
refused with a reason, a bad value is an argument error ahead of that refusal,
and both drivers treat an unparsable --offset / KML_OFFSET as a usage error."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from conftest import REPO
from test_lnms_host import host_ctx

import kmldpc_amd as K

UNSUP = r"\(code -4\)"
ARG = r"\(code -1\)"


def _get(ctx):
    b = C.c_double(-1.0)
    assert K.lib().kml_get_nms_offset(ctx._h, C.byref(b)) == 0
    return b.value


def test_symbols_and_abi_version():
    L = K.lib()
    for name in ("kml_set_nms_offset", "kml_get_nms_offset"):
        assert name in K.header_symbols()
        assert hasattr(L, name)
    assert L.kml_abi_version() == 2  # the change is additive
    for name in ("set_offset", "offset"):
        assert hasattr(K.Context, name)
    assert K.MESSAGES == {"f32": 0, "f16": 1} and K.ALGORITHMS == {"spa": 0, "nms": 1}  # no new enum value


def test_default_and_zero_on_a_host_only_context(data_dir):
    ctx = host_ctx(data_dir)
    assert ctx.offset == 0.0 and _get(ctx) == 0.0
    ctx.set_offset(0)  # the default is always accepted
    ctx.set_offset(0.0)
    assert K.lib().kml_set_nms_offset(ctx._h, -0.0) == 0
    assert ctx.offset == 0.0
    assert (ctx.messages, ctx.demapper, ctx.schedule, ctx.algorithm) == ("f32", "exact", "flooding", ("spa", 0.75))
    ctx.close()


def test_host_only_context_refuses_a_positive_offset(data_dir):
    ctx = host_ctx(data_dir)
    with pytest.raises(K.KmlError, match=UNSUP):
        ctx.set_offset(0.5)
    assert "host-only" in K.lib().kml_last_error(ctx._h).decode()
    assert K.lib().kml_set_nms_offset(ctx._h, 256.0) == -4
    assert ctx.offset == 0.0  # the context keeps its value
    ctx.close()


def test_bad_arguments(data_dir):
    ctx = host_ctx(data_dir)
    L = K.lib()
    for v in (-0.5, float("nan"), float("inf"), -float("inf"), 257.0, 256.0000001, 1e-50, 1e-46):
        assert L.kml_set_nms_offset(ctx._h, v) == -1, v  # KML_E_ARG, ahead of the host-only refusal
    assert "single precision" in L.kml_last_error(ctx._h).decode()  # (1e-46 rounds to +0 in float)
    assert L.kml_set_nms_offset(None, 0.0) == -1
    b = C.c_double(0.0)
    assert L.kml_get_nms_offset(None, C.byref(b)) == -1
    assert L.kml_get_nms_offset(ctx._h, None) == -1
    with pytest.raises(K.KmlError, match=ARG):
        ctx.set_offset(-0.5)
    assert ctx.offset == 0.0
    ctx.close()


def test_constructor_keyword(data_dir):
    host_ctx(data_dir, offset=0.0).close()
    host_ctx(data_dir, offset=0).close()
    with pytest.raises(K.KmlError, match=UNSUP):
        host_ctx(data_dir, offset=0.5)
    with pytest.raises(K.KmlError, match=UNSUP):  # the algorithm's refusal comes first
        host_ctx(data_dir, algorithm="nms", offset=0.5)
    with pytest.raises(K.KmlError, match=ARG):
        host_ctx(data_dir, offset=-1.0)


def test_driver_usage_errors(tmp_path):
    """An unparsable or out-of-range --offset / KML_OFFSET, and a positive one without --algorithm nms, is a
    usage error (exit status 2) in both drivers, before any file is opened; --offset 0 is the default run."""
    env = dict(os.environ, PYTHONPATH=REPO)
    for k in ("KML_ALGORITHM", "KML_SCHEDULE", "KML_DEMAPPER", "KML_MESSAGES", "KML_OFFSET"):
        env.pop(k, None)
    exe = os.path.join(REPO, "kmldpc_amd", "bin", "kmldpc_sim")
    py = [sys.executable, "-m", "kmldpc_amd.simulate"]
    run = lambda cmd, e=env: subprocess.run(cmd, cwd=tmp_path, env=e, capture_output=True, text=True, timeout=120)
    for drv in ([exe], py):
        for bad in ("half", "0.5x", "", "nan", "-0.5", "257"):
            r = run(drv + ["--algorithm", "nms", "--offset", bad, "none.toml"])
            assert r.returncode == 2 and "--offset" in r.stdout + r.stderr, (drv, bad)
        assert run(drv + ["--algorithm", "nms", "none.toml"], dict(env, KML_OFFSET="half")).returncode == 2
        assert run(drv + ["--offset", "0.5", "none.toml"]).returncode == 2  # needs --algorithm nms
        assert run(drv + ["none.toml"], dict(env, KML_OFFSET="0.5")).returncode == 2
        # 0 is the default run: no new line, and the missing config ends it as before
        plain, zero = run(drv + ["none.toml"]), run(drv + ["--offset", "0", "none.toml"])
        assert plain.returncode == 0 and zero.returncode == 0
        assert "offset" not in plain.stdout and "offset" not in zero.stdout
        strip = lambda s: [ln.split("]", 1)[1] for ln in s.splitlines() if "Total time" not in ln]
        assert strip(plain.stdout) == strip(zero.stdout)
        # a positive offset states itself after the message-format line, ahead of "Start simulation"
        on = run(drv + ["--algorithm", "nms:1", "--schedule", "layered", "--messages", "f16", "--offset", "0.5",
                        "none.toml"])
        assert on.returncode == 0
        lines = strip(on.stdout)
        i = [k for k, ln in enumerate(lines) if "BP min-sum offset: 0.5" in ln]
        assert len(i) == 1 and "BP message format: f16" in lines[i[0] - 1] and "Start simulation" in lines[i[0] + 1]
