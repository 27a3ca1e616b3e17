#!/usr/bin/env python3
"""Same-process A/B of the CMUX demultiplexer against the CMUX tree (device buffers): legs alternate round by round -- demux_tree_batch_dev
(k_demux_tree: one external product and TWO 2N-word stores per node) and cmux_tree_batch_dev on an encrypted table (k_cmux_tree: one product
and one store per node) at the same depth and count, 2^d - 1 products per lookup each -- in external products per second.  Then a 1,024-write
histogram update (depth 4 at 1,024 lookups, then rtfhe_lut_accumulate_dev of the 1,024 x 16 leaves into 16 rows): k_trlwe_accumulate's share of
it.  Selectors, inputs and rows are random words: the arithmetic does not depend on them.  Device events around each leg.
usage: ab_demux_tree.py [--steps 20] [--warmup 3]     (shapes: depth 10 at 64 lookups, depth 4 at 8,192 lookups)"""
import argparse, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import rustfhe_amd as R

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--rounds", type=int, default=5)
args = ap.parse_args()
per_round = max(1, args.steps // args.rounds)
st = torch.cuda.current_stream()
SHAPES = ((10, 64), (4, 8192))
N_SEL = 16


def words(rng, shape):
    return rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


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


for N in (1024, 2048):
    P = R.Params(N=N)
    rng = np.random.default_rng(N)
    e = R.Engine(P, 0)                     # no key is loaded: neither call needs one
    sel = e.selectors(words(rng, (N_SEL, 2, 2 * P.l, N)))
    for depth, count in SHAPES:
        rows = 1 << depth
        lut = e.lut_encrypted(words(rng, (rows, 2, N)))
        d_idx = torch.from_numpy(rng.integers(0, N_SEL, (count, depth)).astype(np.int32)).cuda()
        d_x = dev(words(rng, (count, 2, N)))
        d_leaves = torch.zeros((count, rows, 2, N), dtype=torch.int32, device="cuda")
        d_row = torch.zeros((count, 2, N), dtype=torch.int32, device="cuda")
        med = timed({"demux": lambda: e.demux_tree_batch_dev(sel, d_x, depth, d_leaves, count, d_idx, st.cuda_stream),
                     "tree_enc": lambda: e.cmux_tree_batch_dev(sel, lut, depth, d_row, count, d_idx, None, st.cuda_stream)})
        e.sync(st.cuda_stream)
        products = count * (rows - 1)
        res = {"N": N, "depth": depth, "lookups": count, "products": products, "steps_per_leg": per_round * args.rounds}
        for name, ms in med.items():
            res[name + "_ms"] = round(ms, 4)
            res[name + "_products_per_s"] = round(products / ms * 1e3, 1)
        res["demux_vs_tree"] = round(med["tree_enc"] / med["demux"], 3)
        print(json.dumps(res), flush=True)
        lut.close()
        del d_leaves, d_row, d_x
    # the histogram update: 1,024 writes of depth 4, then one accumulation into 16 rows
    depth, count = 4, 1024
    table = e.lut_encrypted(words(rng, (16, 2, N)))
    d_idx = torch.from_numpy(rng.integers(0, N_SEL, (count, depth)).astype(np.int32)).cuda()
    d_x = dev(words(rng, (count, 2, N)))
    d_leaves = torch.zeros((count, 16, 2, N), dtype=torch.int32, device="cuda")
    med = timed({"demux": lambda: e.demux_tree_batch_dev(sel, d_x, depth, d_leaves, count, d_idx, st.cuda_stream),
                 "accumulate": lambda: table.accumulate_dev(d_leaves, 0, 16, count, st.cuda_stream)})
    e.sync(st.cuda_stream)
    total = med["demux"] + med["accumulate"]
    print(json.dumps({"N": N, "histogram_writes": count, "rows": 16, "demux_ms": round(med["demux"], 4), "accumulate_ms": round(med["accumulate"], 4),
                      "accumulate_share_pct": round(100 * med["accumulate"] / total, 2), "accumulate_GB_per_s": round(count * 16 * 2 * N * 4 / med["accumulate"] / 1e6, 1),
                      "steps_per_leg": per_round * args.rounds}), flush=True)
    table.close()
    sel.close()
    e.close()
