"""Child process of test_gpu_llr.py::test_generic_kernel_refuses_maxlog.

The dispatch reads KML_BP_KERNEL once per process, so the refusals of the LLR
front end under KML_BP_KERNEL=generic are checked in a fresh process:

    python tests/llr_generic_child.py <data dir>

kml_set_demapper(KML_DEMAP_MAXLOG) and kml_llr_decode must answer KML_E_UNSUP
and name the reason, the context must keep the exact demapper,
KML_DEMAP_EXACT must be accepted, kml_demap_llr (a pure demapper) must still
equal its model, and the fp64 decode that follows must be the generic
kernel's, bit-exact with the reference; exits non-zero otherwise.
"""
import os
import sys

import numpy as np

from bp_llr_model import maxlog_llr
from conftest import load_case

import kmldpc_amd as K


def main(data_dir):
    if os.environ.get("KML_BP_KERNEL") != "generic":
        sys.exit("start with KML_BP_KERNEL=generic")
    hdr, z = load_case("bg2_16qam_known")
    ctx = K.Context(matrix_file=os.path.join(data_dir, hdr["matrix"]), modem_file=os.path.join(data_dir, hdr["modem"]),
                    is5g=True, max_iter=hdr["max_iter"], device=0)
    rc = K.lib().kml_set_demapper(ctx._h, 1)
    msg = K.lib().kml_last_error(ctx._h).decode()
    if rc != -4 or "generic" not in msg:
        sys.exit(f"kml_set_demapper answered {rc}: {msg}")
    if ctx.demapper != "exact" or ctx.algorithm[0] != "spa":
        sys.exit("the context left the exact demapper or SPA mode")
    if K.lib().kml_set_demapper(ctx._h, 0) != 0:
        sys.exit("KML_DEMAP_EXACT was refused")
    llr = np.zeros((1, ctx.cc_len), np.float32)
    uh = np.zeros((1, ctx.K), np.uint8)
    rc = K.lib().kml_llr_decode(ctx._h, K._p(llr), 1, 5, K._p(uh), None, None, None, 0)
    if rc != -4:
        sys.exit(f"kml_llr_decode answered {rc}")
    rng = np.random.default_rng(3)
    y, h = rng.normal(size=(3, ctx.S, 2)), rng.normal(size=(3, 2))
    if not np.array_equal(ctx.demap_llr(y, h, 0.2).view(np.uint32),
                          maxlog_llr(ctx.constellation(), ctx.bits, y, h, 0.2).view(np.uint32)):
        sys.exit("kml_demap_llr differs from its model")
    p0 = z["v_p0"]
    B = p0.shape[0]
    r = ctx.bp_decode(p0, cc_hat=True, syn=np.full((B, ctx.M), -1.0))
    family = ctx.bp_kernel()
    ctx.close()
    if family != "bp_kernel":
        sys.exit(f"decoded on {family}")
    for key, want in (("ret", z["s_ret"][:B]), ("uu_hat", z["v_uu_hat"]), ("cc_hat", z["v_cc_hat"])):
        if not np.array_equal(r[key], want):
            sys.exit(f"{key} differs from the reference")
    for i in range(B):
        if r["ret"][i] > 1 and not np.array_equal(r["syn"][i], z["v_syn"][i]):
            sys.exit(f"syndrom_soft of codeword {i} differs from the reference")
    print(f"refused under KML_BP_KERNEL=generic; bp_kernel decoded {B} codewords bit-exact")


if __name__ == "__main__":
    main(sys.argv[1])
