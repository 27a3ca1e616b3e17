#!/usr/bin/env python3
"""Timing of the seeded lvl0 ciphertexts, legs alternating round by round in one process (one box, one run):
  (a) Engine.tlwe_seeded_expand_dev alone at n = 635 and 2,048 / 131,072 rows, and the key's 24,576 rows: device events of the library's timer; the
      ratio to the traffic floor (bytes written plus b read, at 8 TB/s).  A recorded figure, not a threshold.
  (b) Engine.upload_tlwe_seeded against the plain host-to-device copy of the same full rows, both from ordinary (pageable) host arrays, at 2,048 and
      131,072 rows: host wall time of the synchronous call.  The plain copy is the yardstick and runs twice per round (unseeded, unseeded_again):
      their difference is the spread the seeded figure is read against.
  (c) the same for Engine.load_ksk_seeded against Engine.load_ksk at the default parameters.
Words are random: neither the copies nor the kernels depend on them.  There is no pass mark.
usage: ab_tlwe_seeded.py [--steps 20] [--warmup 2] [--rounds 5]"""
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
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.rounds):
        for name, f in legs.items():
            t0 = time.perf_counter()
            for _ in range(calls): f()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / calls)
    return {k: stats(v) for k, v in times.items()}


def upload_row(what, extra, med, full_bytes, seeded_bytes, kernel_ms):
    u, s, u2 = med["unseeded"][0], med["seeded"][0], med["unseeded_again"][0]
    res = dict({"leg": what}, **extra)
    res.update({"unseeded_ms": round(u, 3), "unseeded_min_ms": round(med["unseeded"][1], 3), "unseeded_max_ms": round(med["unseeded"][2], 3),
                "unseeded_again_ms": round(u2, 3), "spread_pct": round(abs(u2 / u - 1) * 100, 2), "seeded_ms": round(s, 3),
                "seeded_min_ms": round(med["seeded"][1], 3), "seeded_max_ms": round(med["seeded"][2], 3), "seeded_over_unseeded": round(s / u, 3),
                "full_bytes": full_bytes, "seeded_bytes": seeded_bytes, "expand_kernel_ms": kernel_ms,
                "kernel_share_of_seeded_call_pct": round(kernel_ms / s * 100, 2)})
    print(json.dumps(res), flush=True)


seed = words(np.random.default_rng(1), 8)
P_ = R.Params()
n, w = P_.n, P_.n + 1
ksk_rows = P_.ksk_words // w
rng = np.random.default_rng(n)
e = R.Engine(P_, 0)
kernel_ms = {}
for rows in (2048, ksk_rows, 131072):
    d_b = torch.randint(-2 ** 31, 2 ** 31 - 1, (rows,), dtype=torch.int32, device="cuda")
    d_out = torch.empty((rows, w), dtype=torch.int32, device="cuda")
    ms, lo, hi = device_timed(e, lambda: e.tlwe_seeded_expand_dev(seed, d_b, d_out, rows, 0, st.cuda_stream))
    traffic = rows * (w + 1) * 4
    floor_ms = traffic / HBM * 1e3
    kernel_ms[rows] = round(ms, 4)
    print(json.dumps({"leg": "tlwe_expand_dev", "n": n, "rows": rows, "ms": round(ms, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4),
                      "bytes_written_plus_b_read": traffic, "floor_ms_at_8TBps": round(floor_ms, 5), "over_floor": round(ms / floor_ms, 2),
                      "output_TBps": round(rows * w * 4 / ms / 1e9, 3)}), flush=True)
    del d_b, d_out
for rows in (2048, 131072):
    full = words(rng, (rows, w))
    b = np.ascontiguousarray(full[:, n])
    plain = lambda: torch.from_numpy(full.view(np.int32)).cuda()
    med = wall_timed(e, {"unseeded": plain, "seeded": lambda: e.upload_tlwe_seeded(seed, b), "unseeded_again": plain}, 1 if rows > 2048 else 8)
    upload_row("upload_tlwe", {"n": n, "rows": rows}, med, full.nbytes, b.nbytes + 32, kernel_ms[rows])
    del full, b
ksk = words(rng, (ksk_rows, w))
ksk_b = np.ascontiguousarray(ksk[:, n])
med = wall_timed(e, {"unseeded": lambda: e.load_ksk(ksk), "seeded": lambda: e.load_ksk_seeded(seed, ksk_b), "unseeded_again": lambda: e.load_ksk(ksk)}, 2)
upload_row("load_ksk", {"n": n, "rows": ksk_rows}, med, ksk.nbytes, ksk_b.nbytes + 32, kernel_ms[ksk_rows])
e.close()
