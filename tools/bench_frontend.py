#!/usr/bin/env python3
"""The exact against the max-log front end of the min-sum mode on the BG2 workload, in one process.

    python tools/bench_frontend.py [--steps 10] [--warmup 2] [--alpha 0.75] [--out profiles/llr_bench.json]

The workload is the BG2 bench line's (5G BG2 K960 + 16QAM, Es/N0 5.01 dB,
B = 16,384 resident frames, seed 17) decoded by the layered min-sum schedule at
max_iter 25, and the timed region is bench.py's (warm-up, then `steps`
asynchronous kml_sim_decode calls and one sync).  Two front ends run on the same
frames, alternating, three repeats each: the exact fp64 demapper
(KML_DEMAP_EXACT: P0, and fp64 sum-product candidate metric decodes) and the
max-log front end (KML_DEMAP_MAXLOG: float LLRs, and min-sum candidate metric
decodes).  The known-channel path is timed first, then the blind path
(k-means, four candidates, metric_iter = 5).  After the timing, one more
(untimed) step of each gives its err_bit / err_blk / converged and phase
counters on those frames, and one profiled step (kml_prof_enable) gives the
summed device time of its stages: where a step's time goes.

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
MAX_ITER = 25
SNR = 5.01
FRONT_ENDS = ("exact", "maxlog")
PATHS = (("known", False), ("blind", True))  # name, blind; in this order
STAGES = ("kmeans", "demap", "metric", "bp")
STEP_LIMIT = 420


def workload_args(steps, warmup):
    return argparse.Namespace(snr=SNR, batch=16384, blind=False, is5g=True, max_iter=MAX_ITER,
                              matrix="5GLDPCBG2a3_R12_K960.txt", modem="4bit_16QAM_Gray.txt", seed=17,
                              steps=steps, warmup=warmup)


def step_timing(steps, warmup, alpha):
    """ms per step of path x front end, alternating the front ends, then the counters and the stage profile."""
    import kmldpc_amd as K
    d = bench.data_dir()
    args = workload_args(steps, warmup)
    ctx = K.Context(bench.write_config(d, args), data_dir=d, device=0)
    ctx.sim_generate(args.snr, args.batch, seed=args.seed, first_cw=0)
    ctx.set_algorithm("nms", alpha)
    ctx.set_schedule("layered")
    out = {"alpha": ctx.algorithm[1], "metric_iter": ctx.run_config()["metric_iter"]}
    for path, blind in PATHS:
        ms = {fe: [] for fe in FRONT_ENDS}
        for _ in range(REPEATS):
            for fe in FRONT_ENDS:
                ctx.set_demapper(fe)
                for _ in range(warmup):
                    ctx.sim_decode(SNR, blind=blind, sync=False)
                ctx.sync()
                t0 = time.perf_counter()
                for _ in range(steps):
                    ctx.sim_decode(SNR, blind=blind, sync=False)
                ctx.sync()
                ms[fe].append((time.perf_counter() - t0) / steps * 1e3)
        res = {"ms_per_step": {fe: [round(v, 4) for v in ms[fe]] for fe in FRONT_ENDS}}
        for fe in FRONT_ENDS:
            ctx.set_demapper(fe)
            _, _, c = ctx.sim_decode_ex(SNR, blind=blind)
            res[fe] = {"err_bit": c["err_bit"], "err_blk": c["err_blk"], "converged": c["converged"],
                       "tot_bit": c["tot_bit"], "tot_blk": c["tot_blk"], "ber": c["err_bit"] / c["tot_bit"],
                       "fer": c["err_blk"] / c["tot_blk"], "vn_phases": c["vn_phases"], "cn_phases": c["cn_phases"],
                       "redone": c["redone"], "kernel": ctx.bp_kernel()}
            ctx.prof_enable(True)

            def stages_of(run):
                ctx.prof_reset()
                run()
                got = {st: ctx.prof_read(st) for st in STAGES}
                return {st: {"launches": p["launches"], "ms": round(p["ms"], 4)} for st, p in got.items()}

            res[fe]["stage_ms"] = stages_of(lambda: ctx.sim_decode(SNR, blind=blind))
            if blind:  # the "bp" stage holds the metric decodes and the final decode: histogram mode runs the first alone
                res[fe]["stage_ms_metrics_only"] = stages_of(lambda: ctx.sim_decode_ex(SNR, blind=True, histogram=True))
            ctx.prof_enable(False)
            ctx.prof_reset()
        out[path] = res
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--alpha", type=float, default=0.75)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "llr_bench.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(step_timing(a.steps, a.warmup, a.alpha)), flush=True)
        return 0
    res = {"workload": "5GLDPCBG2a3_R12_K960 + 4bit_16QAM_Gray, Es/N0 5.01 dB, B = 16384, seed 17; min-sum, layered, "
                       "max_iter 25; exact against max-log front end, known H then blind (metric_iter 5)",
           "steps": a.steps, "warmup": a.warmup, "repeats": REPEATS, "src_sha": bench.src_sha(),
           "box": socket.gethostname()}
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--steps", str(a.steps), "--warmup", str(a.warmup),
           "--alpha", str(a.alpha)]
    try:  # a fresh process for the GPU step, under its own time limit
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=STEP_LIMIT)
    except subprocess.TimeoutExpired:
        print(f"bench_frontend: the timing step exceeded {STEP_LIMIT} s", file=sys.stderr)
        return 124
    if p.returncode != 0:
        print(f"bench_frontend: the timing step failed ({p.returncode})", file=sys.stderr)
        return p.returncode if p.returncode > 0 else 1
    res.update(json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    for path, _ in PATHS:
        t = res[path]["ms_per_step"]
        med = {fe: sorted(t[fe])[len(t[fe]) // 2] for fe in FRONT_ENDS}
        res[path]["ms_per_step_median"] = {fe: round(med[fe], 4) for fe in FRONT_ENDS}
        res[path]["spread_ms"] = {fe: round(max(t[fe]) - min(t[fe]), 4) for fe in FRONT_ENDS}
        res[path]["ratio_maxlog_over_exact"] = round(med["maxlog"] / med["exact"], 4)
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
