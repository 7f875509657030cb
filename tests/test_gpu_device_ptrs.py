"""KML_DEVICE_PTRS (include/kmldpc_amd.h): every entry point that takes the
flag, called through the C ABI with the caller's buffers in HBM, writes byte
for byte what the same call writes with host pointers.

The device buffers come from the HIP runtime the library itself is bound to
(its libamdhip64 mapping, found through the library's own hipMalloc), so the
pointers are valid in the library's HIP context.  Inputs are the first three
codewords of the committed fixtures' full vectors: the branches under test
are taken per call, not per size.  Every output starts from the same byte
pattern on both sides, so a part one side leaves unwritten is compared too.

On the known-channel path with device pointers, chosen / metrics / h_hat are
left unwritten (the host-pointer call zeroes them, kmcodec.cc:66-67): they
are not compared here."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import load_case

import kmldpc_amd as K

pytestmark = pytest.mark.gpu

NCW = 3
FILL = 0xA5
CONFIGS = ["peg2304_qpsk", "bg2_16qam", "peg2304_star8"]  # star8: a synthetic 3-bit constellation (make_cons.py)
H2D, D2H = 1, 2  # hipMemcpyHostToDevice, hipMemcpyDeviceToHost


class _DlInfo(C.Structure):
    _fields_ = [("dli_fname", C.c_char_p), ("dli_fbase", C.c_void_p), ("dli_sname", C.c_char_p),
                ("dli_saddr", C.c_void_p)]


_hip = None


def hip():
    """The libamdhip64 mapping libkmldpc_amd.so resolved its HIP calls to."""
    global _hip
    if _hip is None:
        fn = C.cast(K.lib().hipMalloc, C.c_void_p)  # dlsym on the library's handle searches its dependencies
        info = _DlInfo()
        dl = C.CDLL(None)
        dl.dladdr.argtypes = [C.c_void_p, C.POINTER(_DlInfo)]
        assert dl.dladdr(fn, C.byref(info)) != 0
        path = info.dli_fname.decode()
        assert "amdhip64" in os.path.basename(path), path
        h = C.CDLL(path)
        h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        h.hipFree.argtypes = [C.c_void_p]
        assert C.cast(h.hipMalloc, C.c_void_p).value == fn.value
        _hip = h
    return _hip


class DeviceBufs:
    """hipMalloc'ed copies of numpy arrays; freed on exit."""

    def __enter__(self):
        self.ptrs = []
        return self

    def __exit__(self, *a):
        for p in self.ptrs:
            assert hip().hipFree(p) == 0

    def put(self, a):
        a = np.ascontiguousarray(a)
        p = C.c_void_p()
        assert hip().hipMalloc(C.byref(p), max(a.nbytes, 1)) == 0
        self.ptrs.append(p)
        assert hip().hipMemcpy(p, a.ctypes.data_as(C.c_void_p), a.nbytes, H2D) == 0
        return p

    def get(self, p, like):
        out = np.empty_like(like)
        assert hip().hipMemcpy(out.ctypes.data_as(C.c_void_p), p, out.nbytes, D2H) == 0
        return out


def filled(shape, dtype):
    """An output buffer's starting bytes, the same for the host and the device call."""
    a = np.empty(shape, dtype)
    a.view(np.uint8)[...] = FILL
    return a


_cases = {}


def case(data_dir, cfg):
    """(ctx, hdr, known fixture, blind fixture) of one configuration."""
    if cfg not in _cases:
        hdr, zk = load_case(cfg + "_known")
        _, zb = load_case(cfg + "_blind")
        ctx = K.Context(matrix_file=os.path.join(data_dir, hdr["matrix"]),
                        modem_file=os.path.join(data_dir, hdr["modem"]), is5g=bool(hdr["is5g"]),
                        max_iter=hdr["max_iter"], device=0)
        _cases[cfg] = (ctx, hdr, zk, zb)
    return _cases[cfg]


def both_ways(ctx, fn, ins, outs, skip=()):
    """fn(ptr-of-name) -> return code, once with host pointers and once with
    device pointers; every output in `outs` (name -> starting array, None = a
    NULL argument) must come back identical, except the names in `skip`."""
    ins = {k: np.ascontiguousarray(v) for k, v in ins.items()}
    host = {k: (None if v is None else v.copy()) for k, v in outs.items()}
    hp = {k: K._p(v) for k, v in ins.items()}
    hp.update({k: K._p(v) for k, v in host.items()})
    assert fn(hp, 0) == 0, K.lib().kml_last_error(ctx._h)
    with DeviceBufs() as d:
        dp = {k: d.put(v) for k, v in ins.items()}
        dp.update({k: (None if v is None else d.put(v)) for k, v in outs.items()})
        assert fn(dp, K.KML_DEVICE_PTRS) == 0, K.lib().kml_last_error(ctx._h)
        for k, v in outs.items():
            if v is None or k in skip:
                continue
            got = d.get(dp[k], v)
            assert got.tobytes() == host[k].tobytes(), k
            assert host[k].tobytes() != v.tobytes(), f"{k}: the call wrote nothing"
    return host


@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("optional", [True, False])
def test_bp_decode(data_dir, cfg, optional):
    ctx, hdr, zk, _ = case(data_dir, cfg)
    p0 = zk["v_p0"][:NCW]
    outs = dict(uu_hat=filled((NCW, ctx.K), np.uint8), ret=filled(NCW, np.int32),
                cc_hat=filled((NCW, ctx.Ncol), np.uint8), syn=np.full((NCW, ctx.M), 0.25))
    if not optional:
        outs = dict.fromkeys(outs)
    L = K.lib()
    r = both_ways(ctx, lambda p, fl: L.kml_bp_decode(ctx._h, p["p0"], NCW, ctx.max_iter, p["uu_hat"], p["ret"],
                                                     p["cc_hat"], p["syn"], fl), dict(p0=p0), outs)
    if optional:
        assert np.array_equal(r["uu_hat"], zk["v_uu_hat"][:NCW])


@pytest.mark.parametrize("cfg", CONFIGS)
def test_demap(data_dir, cfg):
    ctx, hdr, zk, _ = case(data_dir, cfg)
    ins = dict(y=zk["v_y"][:NCW], h=zk["s_true_h"][:NCW])
    var = 10.0 ** (-hdr["snr"] / 10.0)
    L = K.lib()
    both_ways(ctx, lambda p, fl: L.kml_demap(ctx._h, p["y"], p["h"], var, NCW, p["p0"], fl), ins,
              dict(p0=filled((NCW, ctx.cc_len), np.float64)))


@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("with_h4", [False, True])
def test_kmeans(data_dir, cfg, with_h4):
    ctx, hdr, _, zb = case(data_dir, cfg)
    outs = dict(h_hat=filled((NCW, 2), np.float64), h4=filled((NCW, 4, 2), np.float64) if with_h4 else None)
    L = K.lib()
    both_ways(ctx, lambda p, fl: L.kml_kmeans(ctx._h, p["y"], NCW, 20, p["h_hat"], p["h4"], fl),
              dict(y=zb["v_y"][:NCW]), outs)


@pytest.mark.parametrize("cfg", CONFIGS)
def test_kmeans_state(data_dir, cfg):
    ctx, hdr, _, zb = case(data_dir, cfg)
    outs = dict(clusters=filled((NCW, ctx.Kc, 2), np.float64), idx=filled((NCW, ctx.S), np.int32))
    L = K.lib()
    both_ways(ctx, lambda p, fl: L.kml_kmeans_state(ctx._h, p["y"], NCW, 20, p["clusters"], p["idx"], fl),
              dict(y=zb["v_y"][:NCW]), outs)


@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("known", [True, False])
def test_decode_frames(data_dir, cfg, known):
    ctx, hdr, zk, zb = case(data_dir, cfg)
    z = zk if known else zb
    ins = dict(y=z["v_y"][:NCW])
    if known:
        ins["true_h"] = z["s_true_h"][:NCW]
    outs = dict(uu_hat=filled((NCW, ctx.K), np.uint8), chosen=filled(NCW, np.int32),
                metrics=filled((NCW, 4), np.float64), ret=filled(NCW, np.int32), h_hat=filled((NCW, 2), np.float64))
    L = K.lib()
    r = both_ways(ctx, lambda p, fl: L.kml_decode_frames(ctx._h, p["y"], p.get("true_h"), hdr["snr"], NCW, p["uu_hat"],
                                                         p["chosen"], p["metrics"], p["ret"], p["h_hat"], fl),
                  ins, outs, skip=("chosen", "metrics", "h_hat") if known else ())
    assert np.array_equal(r["uu_hat"], z["v_uu_hat"][:NCW])


@pytest.mark.parametrize("cfg", CONFIGS)
def test_decode_candidates(data_dir, cfg):
    ctx, hdr, _, zb = case(data_dir, cfg)
    y = zb["v_y"][:NCW]
    _, h4 = ctx.kmeans(y)
    outs = dict(uu_hat=filled((NCW, ctx.K), np.uint8), chosen=filled(NCW, np.int32),
                metrics=filled((NCW, 4), np.float64), ret=filled(NCW, np.int32))
    L = K.lib()
    r = both_ways(ctx, lambda p, fl: L.kml_decode_candidates(ctx._h, p["y"], p["h_hats"], 4, hdr["snr"], NCW,
                                                             p["uu_hat"], p["chosen"], p["metrics"], p["ret"], fl),
                  dict(y=y, h_hats=h4), outs)
    assert np.array_equal(r["uu_hat"], zb["v_uu_hat"][:NCW])


@pytest.mark.parametrize("cfg", CONFIGS)
def test_count_errors(data_dir, cfg):
    ctx, hdr, zk, _ = case(data_dir, cfg)
    uu = zk["v_uu"][:NCW].astype(np.uint8)
    uh = uu.copy()
    uh[0, 3] ^= 1
    uh[2, ::7] ^= 1
    cnt = {}
    L = K.lib()
    with DeviceBufs() as d:
        for name, fl, a, b in [("host", 0, K._p(uu), K._p(uh)), ("dev", K.KML_DEVICE_PTRS, d.put(uu), d.put(uh))]:
            cnt[name] = np.array([5, 6, 7, 8], np.uint64)  # the counters are the host's, and are added to
            assert L.kml_count_errors(ctx._h, a, b, NCW, K._p(cnt[name]), fl) == 0, L.kml_last_error(ctx._h)
    assert cnt["dev"].tobytes() == cnt["host"].tobytes()
    nerr = int((uu != uh).sum())
    assert list(cnt["host"]) == [5 + nerr, 6 + 2, 7 + NCW * ctx.K, 8 + NCW]
