"""Child process of tests/test_gpu_lifted.py: the layered kernels' global-table
instances on codes whose tables fit in LDS.

KML_LNMS_TABLES is read once per process, so the forced instances run in a fresh
one:

    KML_LNMS_TABLES=global python tests/lifted_global_child.py <data dir> tables
    KML_BP_KERNEL=generic  python tests/lifted_global_child.py <data dir> generic

tables: the Z = 128 shapes of the parent test file (equality with the models,
and so with the LDS-table instances), then 5G BG2 K960 (12 passes: the items
live in registers) and syn_qc_l200 (layers of two full passes and a partial
one) from P0 and from LLRs, f32 and binary16: every launch must report a
global-table family.
generic: the refusals of the min-sum mode under KML_BP_KERNEL=generic hold for
a layered-only code.  Exits non-zero on any difference.
"""
import os
import sys

import numpy as np

import lifted_codes as LC

import kmldpc_amd as K


def tables(data_dir):
    if os.environ.get("KML_LNMS_TABLES") != "global":
        sys.exit("start with KML_LNMS_TABLES=global")
    fam = LC.FAMILIES[True]
    _, g = LC.graph(data_dir, 128)
    ctx = K.Context(device=0, **LC.ctx_args(data_dir, 128))
    n = 0
    for messages in ("f32", "f16"):
        for alpha in (0.75, 1.0):
            for beta in (0.0, 0.5):
                LC.check_llr_decodes(ctx, g, fam, messages, alpha, beta)
                n += 1
        LC.check_batches(ctx, g, fam, messages)
        LC.check_p0_decode(ctx, g, fam, messages)
    ctx.close()
    # existing codes through the new instances
    from test_bp_llr_model import llr_stream
    from test_bp_lnms_model import CODES, QC, code, stream
    for name in ("bg2", QC):
        matrix, is5g, max_iter, modem, _ = CODES[name]
        _, g = code(data_dir, name)
        ctx = K.Context(matrix_file=os.path.join(data_dir, matrix), modem_file=os.path.join(data_dir, modem), is5g=is5g,
                        max_iter=max_iter, device=0)
        p0 = stream(data_dir, name)["p0"][:16]
        llr = llr_stream(data_dir, name)[:16]
        for messages in ("f32", "f16"):
            for alpha, beta in ((0.75, 0.0), (1.0, 0.5)):
                LC.layered_mode(ctx, alpha, beta, messages)
                r = ctx.bp_decode(p0, max_iter, cc_hat=True)
                if ctx.bp_kernel() != fam[messages]:
                    sys.exit(f"{name}: decoded on {ctx.bp_kernel()}")
                LC.same(r, LC.p0_model(g, p0, max_iter, max_iter, alpha, beta, messages), f"{name} {messages} P0")
                r = ctx.llr_decode(llr, max_iter, cc_hat=True, llr_out=True)
                if ctx.bp_kernel() != fam[messages]:
                    sys.exit(f"{name}: decoded on {ctx.bp_kernel()}")
                LC.same(r, LC.llr_model(g, llr, max_iter, max_iter, alpha, beta, messages), f"{name} {messages} LLR")
                n += 1
        ctx.close()
    print(f"global tables: {n} settings equal the models")


def generic(data_dir):
    if os.environ.get("KML_BP_KERNEL") != "generic":
        sys.exit("start with KML_BP_KERNEL=generic")
    ctx = K.Context(device=0, **LC.ctx_args(data_dir, 128))
    L = K.lib()
    for what, rc in (("kml_set_algorithm", L.kml_set_algorithm(ctx._h, 1, 0.0)),
                     ("kml_set_schedule", L.kml_set_schedule(ctx._h, 1))):
        msg = L.kml_last_error(ctx._h).decode()
        if rc != -4 or "generic" not in msg:
            sys.exit(f"{what} answered {rc}: {msg}")
    if ctx.algorithm[0] != "spa" or ctx.schedule != "flooding":
        sys.exit("the context left SPA mode")
    if ctx.layers().tolist() != list(range(0, 1537, 128)):
        sys.exit("kml_code_layers differs")
    r = ctx.bp_decode(LC.p0_stream(ctx.cc_len, 2, snr=3.0), 5)
    if ctx.bp_kernel() != "bp_kernel" or r["uu_hat"].any():
        sys.exit(f"the fp64 decode on {ctx.bp_kernel()} failed")
    ctx.close()
    print("refused under KML_BP_KERNEL=generic; bp_kernel decoded")


if __name__ == "__main__":
    {"tables": tables, "generic": generic}[sys.argv[2]](sys.argv[1])
