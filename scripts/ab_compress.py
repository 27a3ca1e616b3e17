#!/usr/bin/env python3
"""Timing of compressed results, legs alternating round by round in one process (one box, one run):
  (a) k_compress_rows alone -- 8,192 and 131,072 lvl0 rows at n = 635 (k = 10, 16); 64 and 8,192 TRLWE rows at N = 1024 and 2,048 (P = N, k = 12,
      16) -- in device time, as a multiple of its traffic floor (the bytes it reads once plus the bytes it writes, at 8 TB/s), beside a
      hipMemcpyAsync device-to-device copy of the same input in the same process.  A recorded figure, not a threshold.
  (b) end to end: compress + device-to-pinned-host copy of the compressed buffer against the device-to-pinned-host copy of the full rows (the
      only way results left the GPU before), host wall time of the synchronous sequence.  The full copy runs twice per round (full, full_again):
      their difference is the spread the compressed figure is read against.  8,192 lvl0 rows and 64 packed rows, and two small shapes where a
      launch costs more than the bytes saved.
Words are random: neither the copies nor the kernel depend on them.  There is no pass mark.
usage: ab_compress.py [--steps 40] [--warmup 3] [--rounds 5]"""
import argparse, ctypes as C, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import rustfhe_amd as R

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--rounds", type=int, default=5)
args = ap.parse_args()
per_round = max(1, args.steps // args.rounds)
st = torch.cuda.current_stream()
HBM = 8e12      # bytes / s: the floor the README's traffic figures use

# the HIP runtime the library itself is bound to (dlsym through the library's handle searches its dependencies)
hip_memcpy_async = R.load().hipMemcpyAsync
hip_memcpy_async.restype = C.c_int
hip_memcpy_async.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
D2H, D2D = 2, 3


def memcpy(dst, src, nbytes, kind):
    rc = hip_memcpy_async(dst, src, nbytes, kind, st.cuda_stream)
    assert rc == 0, "hipMemcpyAsync: %d" % rc


def stats(v):
    return float(np.median(v)), float(min(v)), float(max(v))


def device_timed(legs):
    """per leg: (median, min, max) over the rounds of device ms per call, by events on the stream, the legs alternating"""
    for f in legs.values():
        for _ in range(args.warmup): f()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.rounds):
        for name, f in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            for _ in range(per_round): f()
            b.record(st)
            b.synchronize()
            times[name].append(a.elapsed_time(b) / per_round)
    return {k: stats(v) for k, v in times.items()}


def wall_timed(legs):
    """per leg: (median, min, max) over the rounds of host ms per synchronous sequence"""
    for f in legs.values():
        for _ in range(args.warmup): f()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.rounds):
        for name, f in legs.items():
            t0 = time.perf_counter()
            for _ in range(per_round):
                f()
                torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / per_round)
    return {k: stats(v) for k, v in times.items()}


def rand_words(shape):
    return torch.randint(-2 ** 31, 2 ** 31 - 1, shape, dtype=torch.int32, device="cuda")


def kernel_row(what, extra, d_in, read_bytes, W, rows, call):
    d_out = torch.empty((rows, W), dtype=torch.int32, device="cuda")
    d_copy = torch.empty_like(d_in)
    med = device_timed({"compress": lambda: call(d_out), "d2d_copy": lambda: memcpy(d_copy.data_ptr(), d_in.data_ptr(), d_in.numel() * 4, D2D)})
    ms, copy_ms = med["compress"][0], med["d2d_copy"][0]
    traffic = read_bytes + rows * W * 4
    floor_ms = traffic / HBM * 1e3
    res = dict({"leg": what}, **extra)
    res.update({"rows": rows, "ms": round(ms, 4), "min_ms": round(med["compress"][1], 4), "max_ms": round(med["compress"][2], 4),
                "bytes_read_once_plus_written": traffic, "floor_ms_at_8TBps": round(floor_ms, 5), "over_floor": round(ms / floor_ms, 2),
                "d2d_copy_of_input_ms": round(copy_ms, 4), "d2d_copy_over_its_floor": round(copy_ms / (2 * d_in.numel() * 4 / HBM * 1e3), 2),
                "compress_over_d2d_copy": round(ms / copy_ms, 3)})
    print(json.dumps(res), flush=True)


def end_to_end_row(what, extra, d_in, W, rows, call):
    full_bytes, packed_bytes = d_in.numel() * 4, rows * W * 4
    h_full, h_packed = R.pinned_empty((full_bytes // 4,)), R.pinned_empty((packed_bytes // 4,))
    d_out = torch.empty((rows, W), dtype=torch.int32, device="cuda")
    full = lambda: memcpy(h_full.ctypes.data, d_in.data_ptr(), full_bytes, D2H)

    def compressed():
        call(d_out)
        memcpy(h_packed.ctypes.data, d_out.data_ptr(), packed_bytes, D2H)
    med = wall_timed({"full": full, "compressed": compressed, "full_again": full})
    u, s, u2 = med["full"][0], med["compressed"][0], med["full_again"][0]
    res = dict({"leg": what}, **extra)
    res.update({"rows": rows, "full_ms": round(u, 4), "full_min_ms": round(med["full"][1], 4), "full_max_ms": round(med["full"][2], 4),
                "full_again_ms": round(u2, 4), "spread_pct": round(abs(u2 / u - 1) * 100, 2), "compressed_ms": round(s, 4),
                "compressed_min_ms": round(med["compressed"][1], 4), "compressed_max_ms": round(med["compressed"][2], 4),
                "compressed_over_full": round(s / u, 3), "full_bytes": full_bytes, "compressed_bytes": packed_bytes,
                "byte_ratio": round(packed_bytes / full_bytes, 3)})
    print(json.dumps(res), flush=True)


for N in (1024, 2048):
    p = R.Params(N=N)
    n, n1 = p.n, p.n + 1
    e = R.Engine(p, 0)
    if N == 1024:
        for rows in (8192, 131072):
            d_in = rand_words((rows, n1))
            for k in (10, 16):
                kernel_row("tlwe_compress_dev", {"n": n, "k": k}, d_in, rows * n1 * 4, R.compressed_words(n1, k), rows,
                           lambda d_out, k=k, d_in=d_in, rows=rows: e.tlwe_compress_dev(d_in, k, d_out, rows, st.cuda_stream))
            del d_in
    for rows in (64, 8192):
        d_in = rand_words((rows, 2, N))
        for k in (12, 16):
            kernel_row("trlwe_compress_dev", {"N": N, "P": N, "k": k, "launches": N // 512}, d_in, rows * 2 * N * 4, R.compressed_words(2 * N, k), rows,
                       lambda d_out, k=k, d_in=d_in, rows=rows: e.trlwe_compress_dev(d_in, k, N, d_out, rows, None, 1, st.cuda_stream))
        del d_in
    if N == 1024:
        for rows in (16, 8192):
            d_in = rand_words((rows, n1))
            end_to_end_row("tlwe_results_to_pinned_host", {"n": n, "k": 10}, d_in, R.compressed_words(n1, 10), rows,
                           lambda d_out, d_in=d_in, rows=rows: e.tlwe_compress_dev(d_in, 10, d_out, rows, st.cuda_stream))
            del d_in
        for rows in (1, 64):
            d_in = rand_words((rows, 2, N))
            end_to_end_row("packed_rows_to_pinned_host", {"N": N, "P": N, "k": 12}, d_in, R.compressed_words(2 * N, 12), rows,
                           lambda d_out, d_in=d_in, rows=rows: e.trlwe_compress_dev(d_in, 12, N, d_out, rows, None, 1, st.cuda_stream))
            del d_in
    e.close()
