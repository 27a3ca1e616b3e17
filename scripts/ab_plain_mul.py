#!/usr/bin/env python3
"""Timing of the exact TRLWE x plain-polynomial product (Engine.trlwe_mul_plain_batch_dev), legs alternating round by round in one process: the
product runs twice per round (product, product_again: their difference is the spread a figure is read against) beside the closest existing
call, Engine.cmux_tree_batch_dev at depth 1 over as many lookups -- one external product per lookup, also eight 512-point transforms per
polynomial pair at N = 1024 (six forward and two inverse; the product at K = 1: four forward and four inverse).  Device events of the library's
timer on the stream.  The product is stated against the tree's CMUX rate of the same process and against its traffic floor:
(K + 1 + accumulate) * 8 N bytes per sample (K rows read, one written, the old one read when accumulating; the weights' spectra stay in the
L2) over the HBM peak, 8.0 TB/s by specification.
Shapes at both N: K = 1 at 1,024 / 8,192 / 65,536 samples and K = 8 at 8,192, accumulate off; K = 1 at 8,192 with accumulate on.  Rows, weights
and selectors are random words: the arithmetic does not depend on them.  There is no parent to compare with and no pass mark.
usage: ab_plain_mul.py [--steps 50] [--warmup 3] [--rounds 5] [--N 1024 2048]"""
import argparse, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import rustfhe_amd as R

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--N", type=int, nargs="+", default=[1024, 2048])
args = ap.parse_args()
per_round = max(1, args.steps // args.rounds)
st = torch.cuda.current_stream()
HBM_PEAK = 8.0e12


def words(rng, shape):
    return rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)


def device_words(shape):
    return torch.randint(-2 ** 31, 2 ** 31 - 1, shape, dtype=torch.int32, device="cuda")


def timed(e, legs):
    """per leg: (median, min, max) over the rounds of ms per call"""
    for f in legs.values():
        for _ in range(args.warmup): f()
    e.sync(st.cuda_stream)
    times = {k: [] for k in legs}
    for r in range(args.rounds):
        for name, f in legs.items():
            e.timer_begin(st.cuda_stream)
            for _ in range(per_round): f()
            ms, launches = e.timer_end(st.cuda_stream)
            assert launches == per_round, (name, launches)
            times[name].append(ms / per_round)
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in times.items()}


SHAPES = [(1024, 1, False), (8192, 1, False), (65536, 1, False), (8192, 8, False), (8192, 1, True)]

for N in args.N:
    P_ = R.Params(N=N)
    rng = np.random.default_rng(N)
    e = R.Engine(P_, 0)          # no key: neither call reads one
    l1 = 192 * N // 8            # every polynomial at the K = 8 limit
    w = np.zeros((8, N), np.int64)
    for k in range(8):
        w[k] = (l1 // N) * rng.choice([-1, 1], N)
    pp = e.plain_polys(w.astype(np.int32))
    sel = e.selectors(words(rng, (1, 2 * 2 * P_.l * N)))
    lut = e.lut(words(rng, (2, N)))
    for count, K, acc in SHAPES:
        d_x = device_words((count * K, 2, N))
        d_out = device_words((count, 2, N))
        d_tree = torch.zeros((count, 2, N), dtype=torch.int32, device="cuda")
        d_sel_idx = torch.zeros((count, 1), dtype=torch.int32, device="cuda")
        product = lambda: e.trlwe_mul_plain_batch_dev(pp, d_x, count * K, d_out, count, K, None, None, acc, st.cuda_stream)  # noqa: E731
        med = timed(e, {"product": product, "tree": lambda: e.cmux_tree_batch_dev(sel, lut, 1, d_tree, count, d_sel_idx, None, st.cuda_stream),
                        "product_again": product})
        ms, lo, hi = med["product"]
        tree = med["tree"][0]
        floor = count * (K + 1 + int(acc)) * 8 * N / HBM_PEAK * 1e3
        res = {"N": N, "samples": count, "K": K, "accumulate": int(acc), "product_ms": round(ms, 4), "product_min_ms": round(lo, 4), "product_max_ms": round(hi, 4),
               "product_again_ms": round(med["product_again"][0], 4), "spread_pct": round(abs(med["product_again"][0] / ms - 1) * 100, 2),
               "products_per_s": round(count * K / ms * 1e3), "tree_depth1_ms": round(tree, 4), "cmux_per_s": round(count / tree * 1e3),
               "product_rate_over_cmux_rate": round((count * K / ms) / (count / tree), 2),
               "traffic_floor_ms": round(floor, 5), "product_over_floor": round(ms / floor, 2)}
        print(json.dumps(res), flush=True)
        del d_x, d_out, d_tree, d_sel_idx
    pp.close(); sel.close(); lut.close()
    e.close()
