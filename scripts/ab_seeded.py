#!/usr/bin/env python3
"""Timing of the seeded ciphertexts, legs alternating round by round in one process (one box, one run):
  (a) Engine.seeded_expand_dev alone, group 2l, at 1,024 and 8,192 selectors and both N: device events of the library's timer; the ratio to the
      traffic floor (bytes written plus the b halves read, at 8 TB/s).  A recorded figure, not a threshold.
  (b) Engine.selectors_seeded against Engine.selectors of the same set, both from ordinary (pageable) host arrays, at 1,024 and 8,192 selectors:
      host wall time of the whole synchronous call, handle creation and release included.  The unseeded call is the yardstick and runs twice per
      round (unseeded, unseeded_again): their difference is the spread the seeded figure is read against.
  (c) the same for Engine.load_bk_seeded against Engine.load_bk_torus at the default n.
Words are random: neither the copies nor the kernels depend on them.  There is no pass mark.
usage: ab_seeded.py [--steps 20] [--warmup 2] [--rounds 5] [--N 1024 2048]"""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import rustfhe_amd as R

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--N", type=int, nargs="+", default=[1024, 2048])
args = ap.parse_args()
per_round = max(1, args.steps // args.rounds)
st = torch.cuda.current_stream()
HBM = 8e12      # bytes / s: the floor the README's traffic figures use


def words(rng, shape):
    return rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)


def stats(v):
    return float(np.median(v)), float(min(v)), float(max(v))


def device_timed(e, f):
    """(median, min, max) over the rounds of device ms per call, one launch each"""
    for _ in range(args.warmup): f()
    e.sync(st.cuda_stream)
    t = []
    for _ in range(args.rounds):
        e.timer_begin(st.cuda_stream)
        for _ in range(per_round): f()
        ms, launches = e.timer_end(st.cuda_stream)
        assert launches == per_round, launches
        t.append(ms / per_round)
    return stats(t)


def wall_timed(e, legs, calls):
    """per leg: (median, min, max) over the rounds of host ms per synchronous call"""
    for f in legs.values():
        f()
    e.sync()
    times = {k: [] for k in legs}
    for _ in range(args.rounds):
        for name, f in legs.items():
            t0 = time.perf_counter()
            for _ in range(calls): f()
            e.sync()
            times[name].append((time.perf_counter() - t0) * 1e3 / calls)
    return {k: stats(v) for k, v in times.items()}


def upload_row(what, N, extra, med, full_bytes, kernel_ms):
    u, s, u2 = med["unseeded"][0], med["seeded"][0], med["unseeded_again"][0]
    res = dict({"leg": what, "N": N}, **extra)
    res.update({"unseeded_ms": round(u, 3), "unseeded_min_ms": round(med["unseeded"][1], 3), "unseeded_max_ms": round(med["unseeded"][2], 3),
                "unseeded_again_ms": round(u2, 3), "spread_pct": round(abs(u2 / u - 1) * 100, 2), "seeded_ms": round(s, 3),
                "seeded_min_ms": round(med["seeded"][1], 3), "seeded_max_ms": round(med["seeded"][2], 3), "seeded_over_unseeded": round(s / u, 3),
                "full_bytes": full_bytes, "seeded_bytes": full_bytes // 2 + 32, "expand_kernel_ms": kernel_ms,
                "kernel_share_of_seeded_call_pct": None if kernel_ms is None else round(kernel_ms / s * 100, 2)})
    print(json.dumps(res), flush=True)


seed = words(np.random.default_rng(1), 8)
for N in args.N:
    P_ = R.Params(N=N)
    group = 2 * P_.l
    rng = np.random.default_rng(N)
    e = R.Engine(P_, 0)
    kernel_ms = {}
    for n_sel in (1024, 8192):
        rows = n_sel * group
        d_b = torch.randint(-2 ** 31, 2 ** 31 - 1, (rows, N), dtype=torch.int32, device="cuda")
        d_out = torch.empty((2 * rows, N), dtype=torch.int32, device="cuda")
        ms, lo, hi = device_timed(e, lambda: e.seeded_expand_dev(seed, d_b, group, d_out, rows, 0, st.cuda_stream))
        traffic = 3 * rows * N * 4
        floor_ms = traffic / HBM * 1e3
        kernel_ms[n_sel] = round(ms, 4)
        print(json.dumps({"leg": "expand_dev", "N": N, "selectors": n_sel, "rows": rows, "ms": round(ms, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4),
                          "bytes_written_plus_b_read": traffic, "floor_ms_at_8TBps": round(floor_ms, 4), "over_floor": round(ms / floor_ms, 2),
                          "output_TBps": round(2 * rows * N * 4 / ms / 1e9, 3)}), flush=True)
        del d_b, d_out
    if N == 1024:
        for n_sel in (1024, 8192):
            full = words(rng, (n_sel, 2, group, N))
            b = np.ascontiguousarray(full[:, 0])
            med = wall_timed(e, {"unseeded": lambda: e.selectors(full).close(), "seeded": lambda: e.selectors_seeded(seed, b).close(),
                                 "unseeded_again": lambda: e.selectors(full).close()}, 1 if n_sel > 1024 else 4)
            upload_row("trgsw_create", N, {"selectors": n_sel}, med, full.nbytes, kernel_ms[n_sel])
            del full, b
        bk = words(rng, (P_.n, 2, group, N))
        bk_b = np.ascontiguousarray(bk[:, 0])
        med = wall_timed(e, {"unseeded": lambda: e.load_bk_torus(bk), "seeded": lambda: e.load_bk_seeded(seed, bk_b), "unseeded_again": lambda: e.load_bk_torus(bk)}, 2)
        d_b = torch.zeros((P_.n * group, N), dtype=torch.int32, device="cuda")
        d_out = torch.empty((2 * P_.n * group, N), dtype=torch.int32, device="cuda")
        k_ms = device_timed(e, lambda: e.seeded_expand_dev(seed, d_b, group, d_out, P_.n * group, 0, st.cuda_stream))[0]
        upload_row("load_bk", N, {"n": P_.n}, med, bk.nbytes, round(k_ms, 4))
    e.close()
