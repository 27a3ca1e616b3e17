#!/usr/bin/env python3
"""Timing of the packing key switch (Engine.pack_batch_dev), legs alternating round by round in one process: the pack runs twice per round
(pack, pack_again: their difference is the spread a figure is read against) beside pbs_batch_dev of the same number of samples as a scale.
Shapes at N = 1024: (count 1, P 1024, rep 1), (count 1,024, P 4, rep 256: the table layout) and (count 8, P 1024, rep 1); at N = 2048:
(count 1, P 2048, rep 1).  Keys, tables and samples are random words: the arithmetic does not depend on them.  Device events around each
leg.  There is no parent to compare with and no pass mark.
usage: ab_pack.py [--steps 10] [--warmup 2] [--rounds 5] [--N 1024 2048]"""
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


def words(rng, shape):
    return rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)


def timed(legs):
    for f in legs.values():
        for _ in range(args.warmup): f()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for r in range(args.rounds):
        for name, f in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            for _ in range(per_round): f()
            b.record(st)
            b.synchronize()
            times[name].append(a.elapsed_time(b) / per_round)
    return {k: float(np.median(v)) for k, v in times.items()}


SHAPES = {1024: [(1, 1024, 1, None), (1024, 4, 256, "table"), (8, 1024, 1, None)], 2048: [(1, 2048, 1, None)]}

for N in args.N:
    P_ = R.Params(N=N)
    rng = np.random.default_rng(N)
    e = R.Engine(P_, 0)
    e.load_bk_torus(words(rng, P_.bk_words))
    e.load_ksk(words(rng, P_.ksk_words))
    key = e.packing_key(words(rng, (P_.n, 8, 3, 2, N)))
    lut = e.lut(words(rng, (1, N)))
    for count, P, rep, layout in SHAPES[N]:
        pos = R.lut_pack_layout(N, 2)[0] if layout == "table" else None
        M = count * P
        d_in = torch.from_numpy(words(rng, (M, P_.n + 1)).view(np.int32)).cuda()
        d_out = torch.zeros((count, 2, N), dtype=torch.int32, device="cuda")
        d_pbs = torch.zeros((M, P_.n + 1), dtype=torch.int32, device="cuda")
        pack = lambda: e.pack_batch_dev(key, d_in, P, d_out, count, rep, pos, st.cuda_stream)  # noqa: E731
        med = timed({"pack": pack, "pbs": lambda: e.pbs_batch_dev(lut, d_in, d_pbs, M, None, st.cuda_stream), "pack_again": pack})
        e.sync(st.cuda_stream)
        res = {"N": N, "count": count, "P": P, "rep": rep, "samples": M}
        for name, ms in med.items():
            res[name + "_ms"] = round(ms, 4)
        res["spread_pct"] = round(abs(med["pack_again"] / med["pack"] - 1) * 100, 2)
        res["pack_us_per_sample"] = round(med["pack"] / M * 1e3, 3)
        res["pack_vs_pbs_pct"] = round(med["pack"] / med["pbs"] * 100, 2)
        print(json.dumps(res), flush=True)
    lut.close()
    key.close()
    e.close()
