#!/usr/bin/env python3
"""The f32 against the binary16 message format of the layered min-sum decoder on the BG2 workload, in one process.

    python tools/bench_messages.py [--steps 10] [--warmup 2] [--alpha 0.75] [--out profiles/h16_bench.json]

The workload is the BG2 bench line's (5G BG2 K960 + 16QAM, Es/N0 5.01 dB,
B = 16,384 resident frames, seed 17) decoded by the layered min-sum schedule at
max_iter 25, and the timed region is bench.py's (warm-up, then `steps`
asynchronous kml_sim_decode calls and one sync).  Four configurations (known H
and blind with metric_iter = 5, each behind the exact and the max-log front
end), and in each the two message formats (KML_MSG_F32, KML_MSG_F16) on the same
frames, alternating, three repeats each.  After the timing, one more (untimed)
step of each gives its err_bit / err_blk / converged and phase counters (the
sweeps run) on those frames, and one profiled step (kml_prof_enable) gives the
summed device time of its stages.

The binary16 kernel decodes two codewords a workgroup, and a pair runs as many
sweeps as its slower member: `pairing` gives, for the known-H decodes of these
frames, the sum of the codewords' own sweep counts against twice the sum of the
pairs' maxima (what the pairs' lanes execute).  The counts come from a second
context with max_iter 50 decoding at budget 25, where ret - 1 is the sweep
count without the it = max_iter ambiguity.

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
FORMATS = ("f32", "f16")
CONFIGS = (("known_exact", False, "exact"), ("known_maxlog", False, "maxlog"),
           ("blind_exact", True, "exact"), ("blind_maxlog", True, "maxlog"))  # name, blind, demapper; in this order
STAGES = ("kmeans", "demap", "metric", "bp")
STEP_LIMIT = 540
CHUNK = 4096  # frames per call of the pairing count (even: the pairs stay together)


def workload_args(steps, warmup):
    return argparse.Namespace(snr=SNR, batch=16384, blind=False, is5g=True, max_iter=MAX_ITER,
                              matrix="5GLDPCBG2a3_R12_K960.txt", modem="4bit_16QAM_Gray.txt", seed=17,
                              steps=steps, warmup=warmup)


def pairing_cost(K, d, args, alpha, y, th):
    """Own sweeps against the pairs' sweeps on the known-H decodes of frames y, th, per front end."""
    import numpy as np
    ctx = K.Context(matrix_file=os.path.join(d, args.matrix), modem_file=os.path.join(d, args.modem), is5g=True,
                    max_iter=2 * MAX_ITER, device=0)
    ctx.set_algorithm("nms", alpha)
    ctx.set_schedule("layered")
    ctx.set_messages("f16")
    var = 10.0 ** (-0.1 * SNR)
    out = {}
    for fe in ("exact", "maxlog"):
        its = []
        for a in range(0, y.shape[0], CHUNK):
            if fe == "exact":
                r = ctx.bp_decode(ctx.demap(y[a:a + CHUNK], th[a:a + CHUNK], var), MAX_ITER)
            else:
                r = ctx.llr_decode(ctx.demap_llr(y[a:a + CHUNK], th[a:a + CHUNK], var), MAX_ITER)
            its.append(r["ret"].astype(np.int64) - 1)
        it = np.concatenate(its)
        own = int(it.sum())
        paired = 2 * int(np.maximum(it[0::2], it[1::2]).sum())
        out[fe] = {"sweeps_own": own, "sweeps_paired": paired, "ratio": round(paired / own, 4),
                   "pairs_with_equal_counts": int((it[0::2] == it[1::2]).sum()), "pairs": int(it.size // 2)}
    ctx.close()
    return out


def step_timing(steps, warmup, alpha):
    """ms per step of configuration x format, alternating the formats, then the counters and the stage profile."""
    import kmldpc_amd as K
    d = bench.data_dir()
    args = workload_args(steps, warmup)
    ctx = K.Context(bench.write_config(d, args), data_dir=d, device=0)
    ctx.sim_generate(args.snr, args.batch, seed=args.seed, first_cw=0)
    ctx.set_algorithm("nms", alpha)
    ctx.set_schedule("layered")
    out = {"alpha": ctx.algorithm[1], "metric_iter": ctx.run_config()["metric_iter"]}
    for name, blind, fe in CONFIGS:
        ctx.set_demapper(fe)
        ms = {f: [] for f in FORMATS}
        for _ in range(REPEATS):
            for f in FORMATS:
                ctx.set_messages(f)
                for _ in range(warmup):
                    ctx.sim_decode(SNR, blind=blind, sync=False)
                ctx.sync()
                t0 = time.perf_counter()
                for _ in range(steps):
                    ctx.sim_decode(SNR, blind=blind, sync=False)
                ctx.sync()
                ms[f].append((time.perf_counter() - t0) / steps * 1e3)
        res = {"ms_per_step": {f: [round(v, 4) for v in ms[f]] for f in FORMATS}}
        for f in FORMATS:
            ctx.set_messages(f)
            _, _, c = ctx.sim_decode_ex(SNR, blind=blind)
            res[f] = {"err_bit": c["err_bit"], "err_blk": c["err_blk"], "converged": c["converged"],
                      "tot_bit": c["tot_bit"], "tot_blk": c["tot_blk"], "ber": c["err_bit"] / c["tot_bit"],
                      "fer": c["err_blk"] / c["tot_blk"], "vn_phases": c["vn_phases"], "sweeps": c["cn_phases"],
                      "redone": c["redone"], "kernel": ctx.bp_kernel()}
            ctx.prof_enable(True)

            def stages_of(run):
                ctx.prof_reset()
                run()
                got = {st: ctx.prof_read(st) for st in STAGES}
                return {st: {"launches": p["launches"], "ms": round(p["ms"], 4)} for st, p in got.items()}

            res[f]["stage_ms"] = stages_of(lambda: ctx.sim_decode(SNR, blind=blind))
            if blind:  # the "bp" stage holds the metric decodes and the final decode: histogram mode runs the first alone
                res[f]["stage_ms_metrics_only"] = stages_of(lambda: ctx.sim_decode_ex(SNR, blind=True, histogram=True))
            ctx.prof_enable(False)
            ctx.prof_reset()
        out[name] = res
    _, y, th = ctx.sim_frames(args.batch)
    ctx.close()
    out["pairing"] = pairing_cost(K, d, args, alpha, y, th)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--alpha", type=float, default=0.75)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "h16_bench.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(step_timing(a.steps, a.warmup, a.alpha)), flush=True)
        return 0
    res = {"workload": "5GLDPCBG2a3_R12_K960 + 4bit_16QAM_Gray, Es/N0 5.01 dB, B = 16384, seed 17; min-sum, layered, "
                       "max_iter 25; f32 against binary16 messages; known H and blind (metric_iter 5), exact and "
                       "max-log front end",
           "steps": a.steps, "warmup": a.warmup, "repeats": REPEATS, "src_sha": bench.src_sha(),
           "box": socket.gethostname()}
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--steps", str(a.steps), "--warmup", str(a.warmup),
           "--alpha", str(a.alpha)]
    try:  # a fresh process for the GPU step, under its own time limit
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=STEP_LIMIT)
    except subprocess.TimeoutExpired:
        print(f"bench_messages: the timing step exceeded {STEP_LIMIT} s", file=sys.stderr)
        return 124
    if p.returncode != 0:
        print(f"bench_messages: the timing step failed ({p.returncode})", file=sys.stderr)
        return p.returncode if p.returncode > 0 else 1
    res.update(json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    for name, _, _ in CONFIGS:
        t = res[name]["ms_per_step"]
        med = {f: sorted(t[f])[len(t[f]) // 2] for f in FORMATS}
        res[name]["ms_per_step_median"] = {f: round(med[f], 4) for f in FORMATS}
        res[name]["spread_ms"] = {f: round(max(t[f]) - min(t[f]), 4) for f in FORMATS}
        res[name]["ratio_f16_over_f32"] = round(med["f16"] / med["f32"], 4)
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
