#!/usr/bin/env python3
"""fp64 against the opt-in f32 BP mode on the headline workload, in one process.

    python tools/bench_precision.py [--steps 10] [--warmup 2] [--out profiles/f32_bench.json]

The workload and the timed region are bench.py's (PEG2304 + QPSK, known H, 20
iterations, B = 32,768 resident frames; warm-up, then `steps` asynchronous
kml_sim_decode calls and one sync).  Both precisions run on the same context
and the same frames, alternating, three repeats each.  A second step decodes
the reference's own seed-17 stream (kml_ref_frames) in f32 and compares its BER
with the reference's counters (tests/golden/bench/), the z-score computed as
bench.py computes it for fp64.

Each GPU step is a child process under its own time limit; a failure ends the
script with that step's status.  One JSON line goes to --out and to stdout.
"""
import argparse
import json
import math
import os
import socket
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402  (the workload's config, fixtures, src_sha and BER error model)

REPEATS = 3
PRECISIONS = ("f64", "f32")


def workload_args(steps, warmup):
    return argparse.Namespace(snr=2.0, batch=32768, blind=False, is5g=False, max_iter=20,
                              matrix="PEG2304regular0.5.txt", modem="2bits_QPSK.txt", seed=17,
                              steps=steps, warmup=warmup)


def make_context(args):
    import kmldpc_amd as K
    d = bench.data_dir()
    return K, K.Context(bench.write_config(d, args), data_dir=d, device=0)


def step_timing(args):
    """ms per step of both precisions, alternating, and the counters of one more (untimed) step of each."""
    import numpy as np
    K, ctx = make_context(args)
    ctx.sim_generate(args.snr, args.batch, seed=args.seed, first_cw=0)
    ms = {p: [] for p in PRECISIONS}
    for _ in range(REPEATS):
        for p in PRECISIONS:
            ctx.set_precision(p)
            for _ in range(args.warmup):
                ctx.sim_decode(args.snr, sync=False)
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                ctx.sim_decode(args.snr, sync=False)
            ctx.sync()
            ms[p].append((time.perf_counter() - t0) / args.steps * 1e3)
    out = {"ms_per_step": {p: [round(v, 4) for v in ms[p]] for p in PRECISIONS}}
    errs = {}
    for p in PRECISIONS:
        ctx.set_precision(p)
        e, _, c = ctx.sim_decode_ex(args.snr)
        errs[p] = e.astype(np.int64)
        out[p] = {"err_bit": c["err_bit"], "err_blk": c["err_blk"], "tot_blk": c["tot_blk"], "redone": c["redone"],
                  "kernel": ctx.bp_kernel()}
    out["codewords_whose_error_count_differs"] = int(np.sum(errs["f64"] != errs["f32"]))
    ctx.close()
    return out


def step_ber(args):
    """f32 on the reference's own seed-17 stream against the reference's counters (bench.py's BER match)."""
    import numpy as np
    fx = bench.bench_fixture(args)
    if fx is None:
        raise SystemExit("no tests/golden/bench fixture for the workload")
    fn, hdr, ref_errs = fx
    n_ref = int(hdr["n"])
    K, ctx = make_context(args)
    uu, th, y = ctx.ref_frames(K.CLCRandNum(hdr.get("seed", 17)), args.snr, n_ref)
    ctx.sim_load(args.snr, uu, y, th)
    ctx.set_precision("f32")
    g, _, c = ctx.sim_decode_ex(args.snr)
    ctx.close()
    g = g.astype(np.float64)
    r = ref_errs.astype(np.float64)
    Kb = hdr["K"]
    ber, ber_ref = g.sum() / (n_ref * Kb), r.sum() / (n_ref * Kb)
    sig = math.hypot(bench.ber_sigma(g.sum(), (g * g).sum(), n_ref, Kb), bench.ber_sigma(r.sum(), (r * r).sum(), n_ref, Kb))
    return {"ber_line": {
        "frames": f"reference stream CLCRandNum seed {hdr.get('seed', 17)}, first {n_ref} codewords (kml_ref_frames)",
        "reference": f"tests/golden/bench/{fn}",
        "f32_ber": ber, "ref_ber": ber_ref, "ber_sigma_combined": sig, "ber_z": (ber - ber_ref) / sig if sig > 0 else None,
        "f32_err_bit": int(c["err_bit"]), "ref_err_bit": int(r.sum()),
        "f32_err_blk": int(c["err_blk"]), "ref_err_blk": int((ref_errs > 0).sum()),
        "codewords_whose_error_count_differs": int(np.sum(g != r)),
    }}


STEPS = {"timing": (step_timing, 300), "ber": (step_ber, 300)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "f32_bench.json"))
    ap.add_argument("--child", choices=sorted(STEPS), help=argparse.SUPPRESS)
    a = ap.parse_args()
    args = workload_args(a.steps, a.warmup)
    if a.child:
        print("RESULT " + json.dumps(STEPS[a.child][0](args)), flush=True)
        return 0
    res = {"workload": "PEG2304regular0.5 + 2bits_QPSK, Es/N0 2.0 dB, known H, 20 BP iterations, B = 32768",
           "steps": a.steps, "warmup": a.warmup, "repeats": REPEATS, "src_sha": bench.src_sha(),
           "box": socket.gethostname()}
    for name in ("timing", "ber"):  # a fresh process per GPU step, each under its own time limit
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--steps", str(a.steps), "--warmup",
               str(a.warmup)]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=STEPS[name][1])
        except subprocess.TimeoutExpired:
            print(f"bench_precision: step {name} exceeded {STEPS[name][1]} s", file=sys.stderr)
            return 124
        if p.returncode != 0:
            print(f"bench_precision: step {name} failed ({p.returncode})", file=sys.stderr)
            return p.returncode if p.returncode > 0 else 1
        res.update(json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    t = res["ms_per_step"]
    med = {p: sorted(t[p])[len(t[p]) // 2] for p in PRECISIONS}
    spread = {p: max(t[p]) - min(t[p]) for p in PRECISIONS}
    res["ms_per_step_median"] = {p: round(med[p], 4) for p in PRECISIONS}
    res["spread_ms"] = {p: round(spread[p], 4) for p in PRECISIONS}
    res["ratio_f64_over_f32"] = round(med["f64"] / med["f32"], 4)
    # f32 counts as faster when its slowest repeat beats fp64's fastest: a gap beyond the repeats' spread
    res["f32_faster_beyond_spread"] = bool(max(t["f32"]) < min(t["f64"]))
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
