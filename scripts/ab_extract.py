#!/usr/bin/env python3
"""Timing of TRLWE sample extraction (Engine.trlwe_extract_batch_dev), legs alternating round by round in one process: the call runs twice per
round (extract, extract_again: their difference is the spread a figure is read against) beside the lvl1 form of the same shape (the extract
kernel alone, storing natural rows).  rtfhe_timer_end_detail splits the call's device time: the key switch's share, and the remainder -- the
extract kernel(s) and the clearing of the output rows the key switch adds into.  The remainder is stated against two yardsticks: the key switch
of the same samples in the same run, and the bandwidth floor -- 4 (N + 1) bytes written per sample plus the source bytes read (per row the
a-polynomial once and the b words the call reads: rows shared by many samples come from the L2 after that) over the HBM peak, 8.0 TB/s by
specification (6.29 TB/s measured for a float4 copy).
Shapes at N = 1024, default n: 1,024, 8,192 and 65,536 samples as P = 1 over many rows and as P = 1024 over few; at N = 2048: 8,192 samples
both ways.  Rows and keys are random words: the arithmetic does not depend on them.  There is no parent to compare with and no pass mark.
usage: ab_extract.py [--steps 10] [--warmup 2] [--rounds 5] [--N 1024 2048]"""
import argparse, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import rustfhe_amd as R

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--N", type=int, nargs="+", default=[1024, 2048])
args = ap.parse_args()
per_round = max(1, args.steps // args.rounds)
st = torch.cuda.current_stream()
HBM_PEAK = 8.0e12


def words(rng, shape):
    return rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)


def timed(e, legs):
    """median over the rounds of (total ms, key-switch ms) per call, device events of the library's timer on the stream"""
    for f in legs.values():
        for _ in range(args.warmup): f()
    e.sync(st.cuda_stream)
    times = {k: [] for k in legs}
    for r in range(args.rounds):
        for name, f in legs.items():
            e.timer_begin(st.cuda_stream)
            for _ in range(per_round): f()
            ms, ks, _ = e.timer_end_detail(st.cuda_stream)
            times[name].append((ms / per_round, ks / per_round))
    return {k: tuple(float(np.median([t[i] for t in v])) for i in range(2)) for k, v in times.items()}


SAMPLES = {1024: [1024, 8192, 65536], 2048: [8192]}

for N in args.N:
    P_ = R.Params(N=N)
    rng = np.random.default_rng(N)
    e = R.Engine(P_, 0)
    e.load_ksk(words(rng, P_.ksk_words))
    for M in SAMPLES[N]:
        for P in (1, N):
            count = M // P
            d_in = torch.from_numpy(words(rng, (count, 2, N)).view(np.int32)).cuda()
            d_out = torch.zeros((M, P_.n + 1), dtype=torch.int32, device="cuda")
            d_lvl1 = torch.zeros((M, N + 1), dtype=torch.int32, device="cuda")
            coef = [N // 2] if P == 1 else None
            extract = lambda: e.trlwe_extract_batch_dev(d_in, P, d_out, count, coef, 1, st.cuda_stream)  # noqa: E731
            med = timed(e, {"extract": extract, "lvl1": lambda: e.trlwe_extract_lvl1_batch_dev(d_in, P, d_lvl1, count, coef, 1, st.cuda_stream),
                            "extract_again": extract})
            total, ks = med["extract"]
            rest = total - ks
            floor = (M * 4 * (N + 1) + count * (4 * N + 4 * P)) / HBM_PEAK * 1e3
            res = {"N": N, "count": count, "P": P, "samples": M, "extract_ms": round(total, 4), "key_switch_ms": round(ks, 4),
                   "extract_kernel_ms": round(rest, 4), "lvl1_ms": round(med["lvl1"][0], 4), "extract_again_ms": round(med["extract_again"][0], 4),
                   "spread_pct": round(abs(med["extract_again"][0] / total - 1) * 100, 2),
                   "kernel_vs_key_switch_pct": round(rest / ks * 100, 2) if ks > 0 else None,
                   "bandwidth_floor_ms": round(floor, 5), "kernel_over_floor": round(rest / floor, 2), "lvl1_over_floor": round(med["lvl1"][0] / floor, 2)}
            print(json.dumps(res), flush=True)
            del d_in, d_out, d_lvl1
    e.close()
