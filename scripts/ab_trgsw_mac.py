#!/usr/bin/env python3
"""Timing of the TRLWE x TRGSW multiply-accumulate (Engine.trlwe_mul_trgsw_batch_dev), legs alternating round by round in one process: the
product runs twice per round (product, product_again: their difference is the spread a figure is read against) beside the closest existing
call over as many samples --
    K = 1   Engine.cmux_tree_batch_dev at depth 1: one external product per lookup, the same six forward and two inverse transforms;
    K = 8   Engine.trgsw_rotate_batch_dev at depth 8: eight external products with eight pairs of inverse transforms and eight truncations,
            where the sum has one: by transform count the product is expected near (6 K + 2) / (8 K) = 0.78 of the rotation's time.
Device events of the library's timer on the stream.  Shapes at both N: 1,024 and 8,192 samples, accumulate off.  Rows and selectors are random
words: the arithmetic does not depend on them.  Every sample reads its own K rows; the eight selectors are shared.  There is no parent to
compare with and no pass mark.
usage: ab_trgsw_mac.py [--steps 50] [--warmup 3] [--rounds 5] [--N 1024 2048]"""
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


def words(rng, shape):
    return rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)


def device_words(shape):
    return torch.randint(-2 ** 31, 2 ** 31 - 1, shape, dtype=torch.int32, device="cuda")


def timed(e, legs, launches_per_call):
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
            assert launches == per_round * launches_per_call[name], (name, launches)
            times[name].append(ms / per_round)
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in times.items()}


SHAPES = [(1024, 1), (8192, 1), (1024, 8), (8192, 8)]

for N in args.N:
    P_ = R.Params(N=N)
    rng = np.random.default_rng(N)
    e = R.Engine(P_, 0)          # no key: none of the calls reads one
    sel = e.selectors(words(rng, (8, 2 * 2 * P_.l * N)))
    lut = e.lut(words(rng, (2, N)))
    for count, K in SHAPES:
        d_x = device_words((count * K, 2, N))
        d_out = device_words((count, 2, N))
        d_other = torch.zeros((count, 2, N), dtype=torch.int32, device="cuda")
        d_idx = torch.arange(K, dtype=torch.int32, device="cuda").repeat(count, 1).contiguous()      # [count][K]: selectors 0 .. K-1 for every sample
        product = lambda: e.trlwe_mul_trgsw_batch_dev(sel, d_x, count * K, d_out, count, K, d_idx, None, False, st.cuda_stream)  # noqa: E731
        if K == 1:
            other_name = "tree_depth1"
            other = lambda: e.cmux_tree_batch_dev(sel, lut, 1, d_other, count, d_idx, None, st.cuda_stream)  # noqa: E731
        else:
            other_name = "rotate_depth8"
            other = lambda: e.trgsw_rotate_batch_dev(sel, d_x, K, d_other, count, d_idx, None, st.cuda_stream)  # noqa: E731
        med = timed(e, {"product": product, "other": other, "product_again": product}, {"product": 1, "other": 1, "product_again": 1})
        ms, lo, hi = med["product"]
        oth = med["other"][0]
        res = {"N": N, "samples": count, "K": K, "product_ms": round(ms, 4), "product_min_ms": round(lo, 4), "product_max_ms": round(hi, 4),
               "product_again_ms": round(med["product_again"][0], 4), "spread_pct": round(abs(med["product_again"][0] / ms - 1) * 100, 2),
               "products_per_s": round(count * K / ms * 1e3), other_name + "_ms": round(oth, 4), "product_over_" + other_name: round(ms / oth, 3),
               "by_transform_count": round((6 * K + 2) / (8.0 * K), 3)}
        print(json.dumps(res), flush=True)
        del d_x, d_out, d_other, d_idx
    sel.close(); lut.close()
    e.close()
