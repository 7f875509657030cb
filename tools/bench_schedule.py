#!/usr/bin/env python3
"""The flooding against the layered schedule of the min-sum mode on the BG2 workload, in one process.

    python tools/bench_schedule.py [--steps 10] [--warmup 2] [--alpha 0.75] [--out profiles/lnms_bench.json]

The workload is the BG2 bench line's (5G BG2 K960 + 16QAM, Es/N0 5.01 dB, known
H, B = 16,384 resident frames, seed 17) and the timed region is bench.py's
(warm-up, then `steps` asynchronous kml_sim_decode calls and one sync).  Three
configurations run on the same frames, alternating, three repeats each:
flooding min-sum at max_iter 50, layered at 50 and layered at 25 (a context of
its own with max_iter 25 and the same generated frames).  One more (untimed)
step of each gives its err_bit / err_blk / converged on those frames.  Two
ratios are read against flooding in the same process: layered@50 / flooding@50,
the cost of a sweep against an iteration (most codewords of this workload run
the whole budget), and layered@25 / flooding@50, the time to flooding's FER.

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
# name: (schedule, max_iter)
CONFIGS = {"flooding50": ("flooding", 50), "layered50": ("layered", 50), "layered25": ("layered", 25)}
STEP_LIMIT = 300


def workload_args(steps, warmup, max_iter):
    return argparse.Namespace(snr=5.01, batch=16384, blind=False, is5g=True, max_iter=max_iter,
                              matrix="5GLDPCBG2a3_R12_K960.txt", modem="4bit_16QAM_Gray.txt", seed=17,
                              steps=steps, warmup=warmup)


def step_timing(steps, warmup, alpha):
    """ms per step of the three configurations, alternating, and the counters of one more (untimed) step of each."""
    import kmldpc_amd as K
    d = bench.data_dir()
    ctxs = {}
    for mi in sorted({m for _, m in CONFIGS.values()}):
        args = workload_args(steps, warmup, mi)
        sub = os.path.join(d, f"max_iter_{mi}")  # (write_config names its file itself: one directory each)
        os.makedirs(sub, exist_ok=True)
        ctx = K.Context(bench.write_config(sub, args), data_dir=d, device=0)
        ctx.sim_generate(args.snr, args.batch, seed=args.seed, first_cw=0)
        ctx.set_algorithm("nms", alpha)
        ctxs[mi] = ctx
    snr = 5.01
    ms = {k: [] for k in CONFIGS}
    for _ in range(REPEATS):
        for k, (sched, mi) in CONFIGS.items():
            ctx = ctxs[mi]
            ctx.set_schedule(sched)
            for _ in range(warmup):
                ctx.sim_decode(snr, sync=False)
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(steps):
                ctx.sim_decode(snr, sync=False)
            ctx.sync()
            ms[k].append((time.perf_counter() - t0) / steps * 1e3)
    out = {"ms_per_step": {k: [round(v, 4) for v in ms[k]] for k in CONFIGS}, "alpha": ctxs[50].algorithm[1]}
    for k, (sched, mi) in CONFIGS.items():
        ctx = ctxs[mi]
        ctx.set_schedule(sched)
        _, _, c = ctx.sim_decode_ex(snr)
        out[k] = {"schedule": sched, "max_iter": mi, "err_bit": c["err_bit"], "err_blk": c["err_blk"],
                  "converged": c["converged"], "tot_bit": c["tot_bit"], "tot_blk": c["tot_blk"],
                  "ber": c["err_bit"] / c["tot_bit"], "fer": c["err_blk"] / c["tot_blk"],
                  "vn_phases": c["vn_phases"], "cn_phases": c["cn_phases"], "redone": c["redone"],
                  "kernel": ctx.bp_kernel()}
    for ctx in ctxs.values():
        ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--alpha", type=float, default=0.75)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lnms_bench.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(step_timing(a.steps, a.warmup, a.alpha)), flush=True)
        return 0
    res = {"workload": "5GLDPCBG2a3_R12_K960 + 4bit_16QAM_Gray, Es/N0 5.01 dB, known H, B = 16384, seed 17; "
                       "min-sum, flooding at max_iter 50 against layered at 50 and at 25",
           "steps": a.steps, "warmup": a.warmup, "repeats": REPEATS, "src_sha": bench.src_sha(),
           "box": socket.gethostname()}
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--steps", str(a.steps), "--warmup", str(a.warmup),
           "--alpha", str(a.alpha)]
    try:  # a fresh process for the GPU step, under its own time limit
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=STEP_LIMIT)
    except subprocess.TimeoutExpired:
        print(f"bench_schedule: the timing step exceeded {STEP_LIMIT} s", file=sys.stderr)
        return 124
    if p.returncode != 0:
        print(f"bench_schedule: the timing step failed ({p.returncode})", file=sys.stderr)
        return p.returncode if p.returncode > 0 else 1
    res.update(json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    t = res["ms_per_step"]
    med = {k: sorted(t[k])[len(t[k]) // 2] for k in CONFIGS}
    res["ms_per_step_median"] = {k: round(med[k], 4) for k in CONFIGS}
    res["spread_ms"] = {k: round(max(t[k]) - min(t[k]), 4) for k in CONFIGS}
    res["ratio_layered50_over_flooding50"] = round(med["layered50"] / med["flooding50"], 4)
    res["ratio_layered25_over_flooding50"] = round(med["layered25"] / med["flooding50"], 4)
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
