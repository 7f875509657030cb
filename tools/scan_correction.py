#!/usr/bin/env python3
"""Scan the min-sum correction (alpha, beta) on one set of resident frames per SNR.

    python tools/scan_correction.py [--snr 5.01 8.0] [--batch 16384] [--max-iter 25]
        [--alpha 0.625:1:0.0625] [--beta 0:0.75:0.125] [--schedule layered] [--demapper maxlog] [--messages f32]
        [--out profiles/oms_scan.json]

Default: 5G BG2 K960 + 16QAM (the bench workload's code and modem), 16,384
seed-17 frames at each of two SNRs, known H, layered schedule at 25 sweeps behind
the max-log front end, f32 messages.  For every SNR the frames are generated once
(kml_sim_generate) and decoded for every point of the grid: err_bit, err_blk,
converged, sweeps run (the CN phase counter) and the time of one synchronous
step after a warm-up step.  beta = 0 runs the kernels' instances without the
correction.  A second context decodes the same frames with sum-product (50
iterations, exact demapper): the count the surface stands beside.

The GPU step is a child process under its own time limit; a failure ends the
script with that step's status.  One JSON document goes to --out, the FER
surface as a table to stdout.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402  (the workload's config, fixtures and src_sha)

SPA_ITER = 50
STEP_LIMIT = 540


def grid(spec):
    """"lo:hi:step" -> the values lo, lo + step, ... up to hi (inclusive)."""
    lo, hi, step = (float(x) for x in spec.split(":"))
    n = int(round((hi - lo) / step))
    return [lo + k * step for k in range(n + 1)]


def scan(a):
    import kmldpc_amd as K
    d = bench.data_dir()
    wl = argparse.Namespace(snr=a.snr[0], batch=a.batch, blind=False, is5g=True, max_iter=a.max_iter,
                            matrix="5GLDPCBG2a3_R12_K960.txt", modem="4bit_16QAM_Gray.txt", seed=17, steps=1, warmup=1)
    ctx = K.Context(bench.write_config(d, wl), data_dir=d, device=0)
    spa = K.Context(matrix_file=os.path.join(d, wl.matrix), modem_file=os.path.join(d, wl.modem), is5g=True,
                    max_iter=SPA_ITER, device=0)
    out = []
    for snr in a.snr:
        ctx.set_algorithm("spa")
        ctx.sim_generate(snr, a.batch, seed=17, first_cw=0)
        uu, y, th = ctx.sim_frames(a.batch)
        spa.sim_load(snr, uu, y, th)
        _, _, c = spa.sim_decode_ex(snr)
        pt = {"snr": snr, "sum_product": {"max_iter": SPA_ITER, "err_bit": c["err_bit"], "err_blk": c["err_blk"],
                                          "converged": c["converged"], "tot_blk": c["tot_blk"]}, "points": []}
        for alpha in grid(a.alpha):
            ctx.set_algorithm("nms", alpha)
            ctx.set_schedule(a.schedule)
            ctx.set_demapper(a.demapper)
            ctx.set_messages(a.messages)
            for beta in grid(a.beta):
                ctx.set_offset(beta)
                ctx.sim_decode(snr)  # warm-up
                t0 = time.perf_counter()
                c = ctx.sim_decode(snr)
                ms = (time.perf_counter() - t0) * 1e3
                pt["points"].append({"alpha": ctx.algorithm[1], "beta": ctx.offset, "err_bit": c["err_bit"],
                                     "err_blk": c["err_blk"], "converged": c["converged"], "sweeps": c["cn_phases"],
                                     "tot_blk": c["tot_blk"], "step_ms": round(ms, 4), "kernel": ctx.bp_kernel()})
        out.append(pt)
    ctx.close()
    spa.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--snr", type=float, nargs="+", default=[5.01, 8.0])
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--max-iter", type=int, default=25)
    ap.add_argument("--alpha", default="0.625:1:0.0625")
    ap.add_argument("--beta", default="0:0.75:0.125")
    ap.add_argument("--schedule", default="layered", choices=["flooding", "layered"])
    ap.add_argument("--demapper", default="maxlog", choices=["exact", "maxlog"])
    ap.add_argument("--messages", default="f32", choices=["f32", "f16"])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "oms_scan.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(scan(a)), flush=True)
        return 0
    res = {"workload": f"5GLDPCBG2a3_R12_K960 + 4bit_16QAM_Gray, B = {a.batch}, seed 17, known H; min-sum, {a.schedule}, "
                       f"max_iter {a.max_iter}, {a.demapper} demapper, {a.messages} messages",
           "alpha": grid(a.alpha), "beta": grid(a.beta), "src_sha": bench.src_sha(), "box": socket.gethostname()}
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [x for x in sys.argv[1:] if x != "--child"]
    try:  # a fresh process for the GPU step, under its own time limit
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=STEP_LIMIT)
    except subprocess.TimeoutExpired:
        print(f"scan_correction: the scan exceeded {STEP_LIMIT} s", file=sys.stderr)
        return 124
    if p.returncode != 0:
        print(f"scan_correction: the scan failed ({p.returncode})", file=sys.stderr)
        return p.returncode if p.returncode > 0 else 1
    res["snrs"] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    for pt in res["snrs"]:
        sp = pt["sum_product"]
        print(f"Es/N0 {pt['snr']} dB: failed codewords of {sp['tot_blk']} (sum-product, {SPA_ITER} it.: {sp['err_blk']})")
        print("| alpha \\ beta | " + " | ".join(f"{b:g}" for b in res["beta"]) + " |")
        print("|---|" + "---|" * len(res["beta"]))
        nb = len(res["beta"])
        for i, al in enumerate(res["alpha"]):
            row = pt["points"][i * nb:(i + 1) * nb]
            print(f"| {al:g} | " + " | ".join(str(r["err_blk"]) for r in row) + " |")
    return 0


if __name__ == "__main__":
    sys.exit(main())
