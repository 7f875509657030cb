#!/usr/bin/env python3
"""Sum-product against the opt-in normalized min-sum mode on the BG2 workload, in one process.

    python tools/bench_algorithm.py [--steps 10] [--warmup 2] [--alpha 0.75] [--out profiles/nms_bench.json]

The workload is the BG2 bench line's (5G BG2 K960 + 16QAM, Es/N0 5.01 dB, known
H, 50 iterations, B = 16,384 resident frames) and the timed region is bench.py's
(warm-up, then `steps` asynchronous kml_sim_decode calls and one sync).  Both
algorithms run on the same context and the same frames, alternating, three
repeats each; one more (untimed) step of each gives its err_bit / err_blk /
converged on those frames.  Min-sum is a different decoder: its BER / FER are
reported next to sum-product's, not held to them.

The GPU step is a child process under its own time limit; a failure ends the
script with that step's status.  One JSON line goes to --out and to stdout.
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

REPEATS = 3
ALGORITHMS = ("spa", "nms")
STEP_LIMIT = 300


def workload_args(steps, warmup):
    return argparse.Namespace(snr=5.01, batch=16384, blind=False, is5g=True, max_iter=50,
                              matrix="5GLDPCBG2a3_R12_K960.txt", modem="4bit_16QAM_Gray.txt", seed=17,
                              steps=steps, warmup=warmup)


def step_timing(args, alpha):
    """ms per step of both algorithms, alternating, and the counters of one more (untimed) step of each."""
    import numpy as np
    import kmldpc_amd as K
    d = bench.data_dir()
    ctx = K.Context(bench.write_config(d, args), data_dir=d, device=0)
    ctx.sim_generate(args.snr, args.batch, seed=args.seed, first_cw=0)
    ms = {a: [] for a in ALGORITHMS}
    for _ in range(REPEATS):
        for a in ALGORITHMS:
            ctx.set_algorithm(a, alpha if a == "nms" else None)
            for _ in range(args.warmup):
                ctx.sim_decode(args.snr, sync=False)
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                ctx.sim_decode(args.snr, sync=False)
            ctx.sync()
            ms[a].append((time.perf_counter() - t0) / args.steps * 1e3)
    out = {"ms_per_step": {a: [round(v, 4) for v in ms[a]] for a in ALGORITHMS}}
    errs = {}
    for a in ALGORITHMS:
        ctx.set_algorithm(a, alpha if a == "nms" else None)
        e, _, c = ctx.sim_decode_ex(args.snr)
        errs[a] = e.astype(np.int64)
        out[a] = {"err_bit": c["err_bit"], "err_blk": c["err_blk"], "converged": c["converged"],
                  "tot_bit": c["tot_bit"], "tot_blk": c["tot_blk"], "ber": c["err_bit"] / c["tot_bit"],
                  "fer": c["err_blk"] / c["tot_blk"], "vn_phases": c["vn_phases"], "cn_phases": c["cn_phases"],
                  "redone": c["redone"], "kernel": ctx.bp_kernel()}
    out["nms"]["alpha"] = ctx.algorithm[1]
    out["codewords_whose_error_count_differs"] = int(np.sum(errs["spa"] != errs["nms"]))
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--alpha", type=float, default=0.75)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "nms_bench.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    args = workload_args(a.steps, a.warmup)
    if a.child:
        print("RESULT " + json.dumps(step_timing(args, a.alpha)), flush=True)
        return 0
    res = {"workload": "5GLDPCBG2a3_R12_K960 + 4bit_16QAM_Gray, Es/N0 5.01 dB, known H, 50 BP iterations, B = 16384",
           "steps": a.steps, "warmup": a.warmup, "repeats": REPEATS, "src_sha": bench.src_sha(),
           "box": socket.gethostname()}
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--steps", str(a.steps), "--warmup", str(a.warmup),
           "--alpha", str(a.alpha)]
    try:  # a fresh process for the GPU step, under its own time limit
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=STEP_LIMIT)
    except subprocess.TimeoutExpired:
        print(f"bench_algorithm: the timing step exceeded {STEP_LIMIT} s", file=sys.stderr)
        return 124
    if p.returncode != 0:
        print(f"bench_algorithm: the timing step failed ({p.returncode})", file=sys.stderr)
        return p.returncode if p.returncode > 0 else 1
    res.update(json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    t = res["ms_per_step"]
    med = {k: sorted(t[k])[len(t[k]) // 2] for k in ALGORITHMS}
    res["ms_per_step_median"] = {k: round(med[k], 4) for k in ALGORITHMS}
    res["spread_ms"] = {k: round(max(t[k]) - min(t[k]), 4) for k in ALGORITHMS}
    res["ratio_spa_over_nms"] = round(med["spa"] / med["nms"], 4)
    # min-sum counts as faster when its slowest repeat beats sum-product's fastest: a gap beyond the repeats' spread
    res["nms_faster_beyond_spread"] = bool(max(t["nms"]) < min(t["spa"]))
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
