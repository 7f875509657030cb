#!/usr/bin/env python3
"""BER / FER against the BP iteration budget from one decode per frame.

    python tools/iter_profile.py config.toml [--snr S] [--codewords N] [--batch B] [--seed s] [--blind] [--json]

Generates N frames on the GPU (sim_generate, in batches of B) at one SNR,
receives every batch once with the config's [ldpc] max_iter = P
(Context.sim_decode_profile) and prints, for every budget k = 1..P, what a run
configured with max_iter = k counts on the same frames: budget, BER, FER and
the share of converged codewords, in the simulator's number format.  A fixed
codeword count: the sweep driver's stop rule is not applied.

--json adds one JSON line with the raw sums and the timing: ms per batch in
profile mode against the plain sim_decode of the same resident frames
(alternating, median of --repeats).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import kmldpc_amd as K  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("config")
    ap.add_argument("--data-dir", default=None, help="directory the config's relative paths resolve against")
    ap.add_argument("--snr", type=float, default=None, help="Es/N0 in dB (default: the config's minimum_snr)")
    ap.add_argument("--codewords", type=int, default=32768)
    ap.add_argument("--batch", type=int, default=32768)
    ap.add_argument("--seed", type=int, default=17)
    ap.add_argument("--blind", action="store_true")
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--repeats", type=int, default=5, help="timed repeats per batch and mode (--json)")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)

    ctx = K.Context(a.config, data_dir=a.data_dir, device=a.device)
    snr = ctx.run_config()["minimum_snr"] if a.snr is None else a.snr
    P = ctx.max_iter
    prof = np.zeros((P, 3), np.uint64)
    tot_blk = tot_bit = 0
    t_prof, t_plain = [], []
    first = 0
    while first < a.codewords:
        B = min(a.batch, a.codewords - first)
        ctx.sim_generate(snr, B, seed=a.seed, first_cw=first)
        p, _, cnt = ctx.sim_decode_profile(snr, blind=a.blind, cw_prof=False)
        prof += p
        tot_blk += cnt["tot_blk"]
        tot_bit += cnt["tot_bit"]
        if a.json:  # the same resident frames, alternating
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                plain = ctx.sim_decode(snr, blind=a.blind)
                t1 = time.perf_counter()
                p2, _, cnt2 = ctx.sim_decode_profile(snr, blind=a.blind, cw_prof=False)
                t2 = time.perf_counter()
                assert plain == cnt2 == cnt and np.array_equal(p2, p), "the profile call changed the plain counters"
                t_plain.append((t1 - t0) * 1e3)
                t_prof.append((t2 - t1) * 1e3)
        first += B

    print(f"SNR = {snr:03.3f}  codewords = {tot_blk}  max_iter = {P}")
    print("budget BER FER converged")
    for k in range(P):
        ber = int(prof[k, 0]) / max(tot_bit, 1)
        fer = int(prof[k, 1]) / max(tot_blk, 1)
        conv = int(prof[k, 2]) / max(tot_blk, 1)
        print(f"{k + 1:3d} {ber:.14f} {fer:.14f} {conv:.14f}")
    if a.json:
        print(json.dumps(dict(snr=snr, codewords=tot_blk, batch=a.batch, max_iter=P, blind=bool(a.blind),
                              kernel=ctx.bp_kernel(), tot_bit=tot_bit, prof=prof.tolist(),
                              profile_ms_per_batch=statistics.median(t_prof),
                              plain_ms_per_batch=statistics.median(t_plain),
                              profile_ms_all=[round(t, 4) for t in t_prof],
                              plain_ms_all=[round(t, 4) for t in t_plain])))
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
