"""Child process of test_gpu_parity.py::test_generic_kernel_on_the_shipped_codes.

The dispatch reads KML_BP_KERNEL once per process, so the generic bp_kernel is
forced on the shipped codes in a fresh process started with
KML_BP_KERNEL=generic:

    python tests/generic_kernel_child.py <data dir>

Decodes the reference's stored P0 vectors of three fixtures and compares ret,
uu_hat, cc_hat and syndrom_soft with the reference's, bit for bit; exits
non-zero at the first mismatch or when another kernel family ran.
"""
import os
import sys

import numpy as np

from conftest import load_case

import kmldpc_amd as K

# fixture: what it covers in bp_kernel
CASES = {
    "peg2304_qpsk_known": "<3,6>, slots in LDS",
    "bg2_16qam_known": "<12,12>, slots in LDS, the punctured-prior branch",
    "peg8064_qpsk_known": "<3,6>, global slots",
}


def main(data_dir):
    if os.environ.get("KML_BP_KERNEL") != "generic":
        sys.exit("start with KML_BP_KERNEL=generic")
    for case, what in CASES.items():
        hdr, z = load_case(case)
        ctx = K.Context(matrix_file=os.path.join(data_dir, hdr["matrix"]),
                        modem_file=os.path.join(data_dir, hdr["modem"]), is5g=bool(hdr["is5g"]),
                        active=bool(hdr["active"]), max_iter=hdr["max_iter"], device=0)
        p0 = z["v_p0"]
        B = p0.shape[0]
        r = ctx.bp_decode(p0, cc_hat=True, syn=np.full((B, ctx.M), -1.0))
        family = ctx.bp_kernel()
        ctx.close()
        if family != "bp_kernel":
            sys.exit(f"{case}: decoded on {family}")
        for key, want in (("ret", z["s_ret"][:B]), ("uu_hat", z["v_uu_hat"]), ("cc_hat", z["v_cc_hat"])):
            if not np.array_equal(r[key], want):
                sys.exit(f"{case}: {key} differs from the reference")
        for i in range(B):
            if r["ret"][i] > 1 and not np.array_equal(r["syn"][i], z["v_syn"][i]):
                sys.exit(f"{case}: syndrom_soft of codeword {i} differs from the reference")
        print(f"{case}: bp_kernel ok ({what}; {B} codewords)")


if __name__ == "__main__":
    main(sys.argv[1])
