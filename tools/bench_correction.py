#!/usr/bin/env python3
"""Normalized (alpha 0.75, no offset) against offset (alpha 1, beta 0.5) min-sum on the BG2 workload, in one process.

    python tools/bench_correction.py [--steps 10] [--warmup 2] [--out profiles/oms_bench.json]

The workload is the BG2 bench line's (5G BG2 K960 + 16QAM, Es/N0 5.01 dB,
B = 16,384 resident frames, seed 17) decoded by the layered min-sum schedule at
max_iter 25 behind the max-log front end, and the timed region is bench.py's
(warm-up, then `steps` asynchronous kml_sim_decode calls and one sync).  Four
configurations (known H and blind with metric_iter = 5, each with f32 and with
binary16 messages), and in each the two parameter pairs (alpha, beta) = (0.75, 0)
and (1, 0.5) on the same frames, alternating, three repeats each.  After the
timing, one more (untimed) step of each gives its err_bit / err_blk / converged
and phase counters (the sweeps run) on those frames.

The yardstick for the offset's step time is the beta-0 step time of the same
configuration scaled by the ratio of sweeps run (`ms_expected_from_sweeps`); the
offset instances carry two more VALU instructions per edge and pass, and what
exceeds the yardstick by more than the repeats' spread is theirs.

A second context (max_iter 50, sum-product, exact demapper, known H) decodes the
same frames once: the count the min-sum counts stand beside.

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
SPA_ITER = 50
SNR = 5.01
PAIRS = (("nms_0.75", 0.75, 0.0), ("oms_1_0.5", 1.0, 0.5))  # name, alpha, beta; in this order
CONFIGS = (("known_f32", False, "f32"), ("known_f16", False, "f16"),
           ("blind_f32", True, "f32"), ("blind_f16", True, "f16"))  # name, blind, messages
STEP_LIMIT = 540


def workload_args(steps, warmup):
    return argparse.Namespace(snr=SNR, batch=16384, blind=False, is5g=True, max_iter=MAX_ITER,
                              matrix="5GLDPCBG2a3_R12_K960.txt", modem="4bit_16QAM_Gray.txt", seed=17,
                              steps=steps, warmup=warmup)


def counters(c, kernel):
    return {"err_bit": c["err_bit"], "err_blk": c["err_blk"], "converged": c["converged"], "tot_bit": c["tot_bit"],
            "tot_blk": c["tot_blk"], "ber": c["err_bit"] / c["tot_bit"], "fer": c["err_blk"] / c["tot_blk"],
            "vn_phases": c["vn_phases"], "sweeps": c["cn_phases"], "redone": c["redone"], "kernel": kernel}


def step_timing(steps, warmup):
    """ms per step of configuration x pair, alternating the pairs, then the counters; then sum-product's count."""
    import kmldpc_amd as K
    d = bench.data_dir()
    args = workload_args(steps, warmup)
    ctx = K.Context(bench.write_config(d, args), data_dir=d, device=0)
    ctx.sim_generate(args.snr, args.batch, seed=args.seed, first_cw=0)
    ctx.set_algorithm("nms")
    ctx.set_schedule("layered")
    ctx.set_demapper("maxlog")
    out = {"metric_iter": ctx.run_config()["metric_iter"]}

    def select(alpha, beta):
        ctx.set_algorithm("nms", alpha)  # (keeps the schedule, the demapper, the format and the offset)
        ctx.set_offset(beta)

    for name, blind, fmt in CONFIGS:
        ctx.set_messages(fmt)
        ms = {p: [] for p, _, _ in PAIRS}
        for _ in range(REPEATS):
            for p, alpha, beta in PAIRS:
                select(alpha, beta)
                for _ in range(warmup):
                    ctx.sim_decode(SNR, blind=blind, sync=False)
                ctx.sync()
                t0 = time.perf_counter()
                for _ in range(steps):
                    ctx.sim_decode(SNR, blind=blind, sync=False)
                ctx.sync()
                ms[p].append((time.perf_counter() - t0) / steps * 1e3)
        res = {"ms_per_step": {p: [round(v, 4) for v in ms[p]] for p in ms}}
        for p, alpha, beta in PAIRS:
            select(alpha, beta)
            _, _, c = ctx.sim_decode_ex(SNR, blind=blind)
            res[p] = counters(c, ctx.bp_kernel())
            res[p].update(alpha=ctx.algorithm[1], beta=ctx.offset)
        out[name] = res
    uu, y, th = ctx.sim_frames(args.batch)
    ctx.close()
    spa = K.Context(matrix_file=os.path.join(d, args.matrix), modem_file=os.path.join(d, args.modem), is5g=True,
                    max_iter=SPA_ITER, device=0)
    spa.sim_load(SNR, uu, y, th)
    _, _, c = spa.sim_decode_ex(SNR)
    out["sum_product"] = counters(c, spa.bp_kernel())
    out["sum_product"]["max_iter"] = SPA_ITER
    spa.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "oms_bench.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(step_timing(a.steps, a.warmup)), flush=True)
        return 0
    res = {"workload": "5GLDPCBG2a3_R12_K960 + 4bit_16QAM_Gray, Es/N0 5.01 dB, B = 16384, seed 17; min-sum, layered, "
                       "max_iter 25, max-log front end; (alpha, beta) = (0.75, 0) against (1, 0.5); known H and blind "
                       "(metric_iter 5), f32 and binary16 messages; sum-product (50 iterations, known H) beside them",
           "steps": a.steps, "warmup": a.warmup, "repeats": REPEATS, "src_sha": bench.src_sha(),
           "box": socket.gethostname()}
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--steps", str(a.steps), "--warmup", str(a.warmup)]
    try:  # a fresh process for the GPU step, under its own time limit
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=STEP_LIMIT)
    except subprocess.TimeoutExpired:
        print(f"bench_correction: the timing step exceeded {STEP_LIMIT} s", file=sys.stderr)
        return 124
    if p.returncode != 0:
        print(f"bench_correction: the timing step failed ({p.returncode})", file=sys.stderr)
        return p.returncode if p.returncode > 0 else 1
    res.update(json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    base, off = PAIRS[0][0], PAIRS[1][0]
    for name, _, _ in CONFIGS:
        t = res[name]["ms_per_step"]
        med = {k: sorted(t[k])[len(t[k]) // 2] for k in t}
        res[name]["ms_per_step_median"] = {k: round(med[k], 4) for k in t}
        res[name]["spread_ms"] = {k: round(max(t[k]) - min(t[k]), 4) for k in t}
        res[name]["ratio_offset_over_base"] = round(med[off] / med[base], 4)
        res[name]["sweeps_ratio"] = round(res[name][off]["sweeps"] / res[name][base]["sweeps"], 4)
        res[name]["ms_expected_from_sweeps"] = round(med[base] * res[name][off]["sweeps"] / res[name][base]["sweeps"], 4)
        res[name]["ms_over_expected"] = round(med[off] - res[name]["ms_expected_from_sweeps"], 4)
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
