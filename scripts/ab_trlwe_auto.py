#!/usr/bin/env python3
"""Timing of the TRLWE key switch (Engine.trlwe_auto_batch_dev), legs alternating round by round in one process: the call runs twice per round
(switch, switch_again: their difference is the spread a figure is read against) beside Engine.trgsw_rotate_batch_dev of the same depth over
as many rows -- a rotation step is a whole CMUX, 2l forward and 2 inverse transforms, where a switch step has l forward and 2 inverse: by
transform count the switch is expected near (l + 2) / (2l + 2) = 0.625 of the rotation's time.
Device events of the library's timer on the stream.  Shapes at both N: depths 1 and 8, 1,024 and 8,192 rows, out of place.  Rows, keys and
selectors are random words: the arithmetic does not depend on them.  There is no parent to compare with and no pass mark.
usage: ab_trlwe_auto.py [--steps 50] [--warmup 3] [--rounds 5] [--N 1024 2048]"""
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


def timed(e, legs):
    """per leg: (median, min, max) over the rounds of ms per call; every leg is one launch per call"""
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


SHAPES = [(1024, 1), (8192, 1), (1024, 8), (8192, 8)]

for N in args.N:
    P_ = R.Params(N=N)
    rng = np.random.default_rng(N)
    e = R.Engine(P_, 0)          # no key: neither call reads one
    t = [3, 5, N // 2 + 1, N + 1, 2 * N - 1, 7, 9, 11]
    key = e.trlwe_switch_key(words(rng, (len(t), P_.l, 2, N)), t)
    sel = e.selectors(words(rng, (8, 2 * 2 * P_.l * N)))
    for count, depth in SHAPES:
        d_x = device_words((count, 2, N))
        d_out = torch.zeros((count, 2, N), dtype=torch.int32, device="cuda")
        d_other = torch.zeros((count, 2, N), dtype=torch.int32, device="cuda")
        d_idx = torch.arange(depth, dtype=torch.int32, device="cuda").repeat(count, 1).contiguous()      # [count][depth]: selectors 0 .. depth-1 for every row
        entry = list(range(depth))
        switch = lambda: e.trlwe_auto_batch_dev(key, d_x, d_out, count, entry, None, st.cuda_stream)  # noqa: E731
        rotate = lambda: e.trgsw_rotate_batch_dev(sel, d_x, depth, d_other, count, d_idx, None, st.cuda_stream)  # noqa: E731
        med = timed(e, {"switch": switch, "rotate": rotate, "switch_again": switch})
        ms, lo, hi = med["switch"]
        oth = med["rotate"][0]
        res = {"N": N, "rows": count, "depth": depth, "switch_ms": round(ms, 4), "switch_min_ms": round(lo, 4), "switch_max_ms": round(hi, 4),
               "switch_again_ms": round(med["switch_again"][0], 4), "spread_pct": round(abs(med["switch_again"][0] / ms - 1) * 100, 2),
               "steps_per_s": round(count * depth / ms * 1e3), "rotate_ms": round(oth, 4), "switch_over_rotate": round(ms / oth, 3),
               "by_transform_count": round((P_.l + 2) / (2.0 * P_.l + 2), 3)}
        print(json.dumps(res), flush=True)
        del d_x, d_out, d_other, d_idx
    key.close(); sel.close()
    e.close()
