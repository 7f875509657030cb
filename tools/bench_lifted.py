#!/usr/bin/env python3
"""The layered min-sum decoders on the lifted BG2 codes against the K960 yardstick, in one process.

    python tools/bench_lifted.py [--steps 5] [--warmup 1] [--batch 8192] [--out profiles/lifted_bench.json]

Workload per code: 16QAM, Es/N0 5.01 dB, known H, the max-log front end, the
layered schedule at max_iter 25, alpha 0.75, B resident frames (seed 17); the
timed region is bench.py's (warm-up, then `steps` asynchronous kml_sim_decode
calls and one sync).  The two message formats (f32, binary16) run on the same
frames, alternating, three repeats each; one more untimed step of each gives the
sweeps run (the CN-phase counter), FER and the kernel family.

Codes: 5G BG2 K960 (Z = 96, the yardstick: LDS tables, two workgroups a CU),
and tests/golden/make_codes_lifted.py's Z = 128 (LDS tables, two workgroups),
Z = 256 (LDS tables, one workgroup), Z = 288 and Z = 384 (global tables, one
workgroup).  A second child process with KML_LNMS_TABLES=global runs K960,
Z = 128 and Z = 256 on the global-table instances: the same code, frames and
occupancy, so the difference is what the tables' placement costs.

Reported per code and format: ms per step, sweeps, edge-sweeps per second
(E x sweeps / time) and its ratio to K960's in the same process, FER.
Each GPU step is a child process under its own time limit; a failure ends the
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
sys.path.insert(0, os.path.join(REPO, "tests", "golden"))

import bench  # noqa: E402  (the workload's config, fixtures and src_sha)

REPEATS = 3
MAX_ITER = 25
SNR = 5.01
FORMATS = ("f32", "f16")
K960 = "5GLDPCBG2a3_R12_K960.txt"
CODES = {"default": ("k960", 128, 256, 288, 384), "global": ("k960", 128, 256)}
STEP_LIMIT = 540


def one_code(K, d, code, a):
    import make_codes_lifted
    matrix = K960 if code == "k960" else os.path.basename(make_codes_lifted.write(code, d))
    args = argparse.Namespace(snr=SNR, batch=a.batch, blind=False, is5g=True, max_iter=MAX_ITER, matrix=matrix,
                              modem="4bit_16QAM_Gray.txt", seed=17, steps=a.steps, warmup=a.warmup)
    ctx = K.Context(bench.write_config(d, args), data_dir=d, device=0)
    ctx.sim_generate(SNR, a.batch, seed=17, first_cw=0)
    ctx.set_algorithm("nms", 0.75)
    ctx.set_schedule("layered")
    ctx.set_demapper("maxlog")
    ms = {f: [] for f in FORMATS}
    for _ in range(REPEATS):
        for f in FORMATS:
            ctx.set_messages(f)
            for _ in range(a.warmup):
                ctx.sim_decode(SNR, sync=False)
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                ctx.sim_decode(SNR, sync=False)
            ctx.sync()
            ms[f].append((time.perf_counter() - t0) / a.steps * 1e3)
    lp = ctx.layers()
    res = {"Z": ctx.Z, "N": ctx.Ncol, "M": ctx.M, "E": ctx.E,
           "passes": int(sum(-(-int(b - a) // 96) for a, b in zip(lp[:-1], lp[1:])))}
    for f in FORMATS:
        ctx.set_messages(f)
        _, _, c = ctx.sim_decode_ex(SNR)
        med = sorted(ms[f])[len(ms[f]) // 2]
        res[f] = {"ms_per_step": [round(v, 4) for v in ms[f]], "ms_per_step_median": round(med, 4),
                  "sweeps": c["cn_phases"], "fer": c["err_blk"] / c["tot_blk"], "converged": c["converged"],
                  "edge_sweeps_per_s": round(ctx.E * c["cn_phases"] / (med * 1e-3), 1), "kernel": ctx.bp_kernel()}
    ctx.close()
    return res


def child(a):
    import kmldpc_amd as K
    d = bench.data_dir()
    out = {}
    for code in CODES[a.child]:
        out[str(code)] = one_code(K, d, code, a)
    for code, r in out.items():
        for f in FORMATS:
            r[f]["rate_vs_k960"] = round(r[f]["edge_sweeps_per_s"] / out["k960"][f]["edge_sweeps_per_s"], 4)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lifted_bench.json"))
    ap.add_argument("--child", choices=list(CODES), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(child(a)), flush=True)
        return 0
    res = {"workload": "16QAM Gray, Es/N0 5.01 dB, known H, max-log front end, layered min-sum, max_iter 25, alpha "
                       "0.75, seed 17; K960 and the lifted BG2 codes; f32 against binary16 messages",
           "batch": a.batch, "steps": a.steps, "warmup": a.warmup, "repeats": REPEATS, "src_sha": bench.src_sha(),
           "box": socket.gethostname()}
    for which in CODES:
        env = dict(os.environ)
        env.pop("KML_LNMS_TABLES", None)
        if which == "global":
            env["KML_LNMS_TABLES"] = "global"
        cmd = [sys.executable, os.path.abspath(__file__), "--child", which, "--steps", str(a.steps), "--warmup",
               str(a.warmup), "--batch", str(a.batch)]
        try:  # a fresh process for each GPU step, under its own time limit
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=STEP_LIMIT, env=env)
        except subprocess.TimeoutExpired:
            print(f"bench_lifted: the {which} step exceeded {STEP_LIMIT} s", file=sys.stderr)
            return 124
        if p.returncode != 0:
            print(f"bench_lifted: the {which} step failed ({p.returncode})", file=sys.stderr)
            return p.returncode if p.returncode > 0 else 1
        res["tables_" + which] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
