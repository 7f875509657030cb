"""Child process of test_gpu_oms.py::test_generic_kernel_refuses_the_offset.

The dispatch reads KML_BP_KERNEL once per process, so the refusal of a positive
min-sum offset under KML_BP_KERNEL=generic is checked in a fresh process:

    python tests/oms_generic_child.py <data dir>

kml_set_nms_offset(0.5) must answer KML_E_UNSUP and name the reason, the context
must keep offset 0 and SPA mode, a bad value must still be an argument error,
offset 0 must be accepted, and the fp64 decode that follows must be the generic
kernel's, bit-exact with the reference; exits non-zero otherwise.
"""
import os
import sys

import numpy as np

from conftest import load_case

import kmldpc_amd as K


def main(data_dir):
    if os.environ.get("KML_BP_KERNEL") != "generic":
        sys.exit("start with KML_BP_KERNEL=generic")
    hdr, z = load_case("bg2_16qam_known")
    ctx = K.Context(matrix_file=os.path.join(data_dir, hdr["matrix"]), modem_file=os.path.join(data_dir, hdr["modem"]),
                    is5g=True, max_iter=hdr["max_iter"], device=0)
    rc = K.lib().kml_set_nms_offset(ctx._h, 0.5)
    msg = K.lib().kml_last_error(ctx._h).decode()
    if rc != -4 or "generic" not in msg:
        sys.exit(f"kml_set_nms_offset answered {rc}: {msg}")
    if ctx.offset != 0.0 or ctx.algorithm[0] != "spa" or ctx.schedule != "flooding" or ctx.messages != "f32":
        sys.exit("the context left offset 0, SPA mode, the flooding schedule or F32")
    if K.lib().kml_set_nms_offset(ctx._h, -0.5) != -1 or K.lib().kml_set_nms_offset(ctx._h, 257.0) != -1:
        sys.exit("a bad offset was not an argument error")
    if K.lib().kml_set_nms_offset(ctx._h, 0.0) != 0:
        sys.exit("offset 0 was refused")
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
