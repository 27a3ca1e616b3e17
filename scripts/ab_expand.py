#!/usr/bin/env python3
"""Timing of the device-side expansion of compressed rows, legs alternating round by round in one process (one box, one run):
  (a) k_expand_rows alone -- 8,192 and 131,072 lvl0 rows at n = 635, k = 10; 64 and 8,192 TRLWE rows at N = 1024 and 8,192 at N = 2048 (P = N,
      k = 12; a NULL list, and the same coefficients as a list, which is two launches at N = 2048) -- in device time, as a multiple of its traffic
      floor (the bytes it reads once plus the bytes it writes, at 8 TB/s), beside k_compress_rows on the same shape in the same rounds.  A recorded
      figure, not a threshold.
  (b) what the user gains: from pinned host memory to a ready device buffer of full rows -- the copy of the packed words followed by the
      expansion, against a plain hipMemcpyAsync of the full rows (the only way before) -- host wall time of the synchronous sequence.  The full
      copy runs twice per round (full, full_again): their difference is the spread the compressed figure is read against.  The shapes of (a) and
      two small ones where a launch costs more than the bytes saved.
Words are random: neither the copies nor the kernels depend on them.  There is no pass mark.
usage: ab_expand.py [--steps 40] [--warmup 3] [--rounds 5]"""
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
H2D = 1


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


def kernel_row(what, extra, rows, full_words, W, expand, compress):
    """expand(d_packed, d_full) and compress(d_full, d_packed) on `rows` rows of full_words / W words"""
    d_packed, d_full = rand_words((rows, W)), rand_words((rows, full_words))
    d_packed2 = torch.empty_like(d_packed)
    med = device_timed({"expand": lambda: expand(d_packed, d_full), "compress": lambda: compress(d_full, d_packed2)})
    traffic = rows * (W + full_words) * 4      # the same bytes either way: one side read once, the other written
    floor_ms = traffic / HBM * 1e3
    ms, cms = med["expand"][0], med["compress"][0]
    res = dict({"leg": what}, **extra)
    res.update({"rows": rows, "ms": round(ms, 4), "min_ms": round(med["expand"][1], 4), "max_ms": round(med["expand"][2], 4),
                "bytes_read_once_plus_written": traffic, "floor_ms_at_8TBps": round(floor_ms, 5), "over_floor": round(ms / floor_ms, 2),
                "compress_ms": round(cms, 4), "compress_min_ms": round(med["compress"][1], 4), "compress_max_ms": round(med["compress"][2], 4),
                "compress_over_floor": round(cms / floor_ms, 2), "expand_over_compress": round(ms / cms, 3)})
    print(json.dumps(res), flush=True)


def upload_row(what, extra, rows, full_words, W, expand):
    full_bytes, packed_bytes = rows * full_words * 4, rows * W * 4
    h_full, h_packed = R.pinned_empty((full_bytes // 4,)), R.pinned_empty((packed_bytes // 4,))
    h_full[:] = 1
    h_packed[:] = 1
    d_full, d_packed = torch.empty((rows, full_words), dtype=torch.int32, device="cuda"), torch.empty((rows, W), dtype=torch.int32, device="cuda")
    full = lambda: memcpy(d_full.data_ptr(), h_full.ctypes.data, full_bytes, H2D)

    def compressed():
        memcpy(d_packed.data_ptr(), h_packed.ctypes.data, packed_bytes, H2D)
        expand(d_packed, d_full)
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
    s = st.cuda_stream
    W0, W1 = R.compressed_words(n1, 10), R.compressed_words(2 * N, 12)
    coef = np.arange(N, dtype=np.int32)
    tl_exp = lambda rows: (lambda d_w, d_f: e.tlwe_expand_dev(d_w, 10, d_f, rows, s))                               # noqa: E731
    tl_cmp = lambda rows: (lambda d_f, d_w: e.tlwe_compress_dev(d_f, 10, d_w, rows, s))                             # noqa: E731
    tr_exp = lambda rows, c: (lambda d_w, d_f: e.trlwe_expand_dev(d_w, 12, N, d_f, rows, c, 1, s))                  # noqa: E731
    tr_cmp = lambda rows, c: (lambda d_f, d_w: e.trlwe_compress_dev(d_f, 12, N, d_w, rows, c, 1, s))                # noqa: E731
    if N == 1024:
        for rows in (8192, 131072):
            kernel_row("tlwe_expand_dev", {"n": n, "k": 10}, rows, n1, W0, tl_exp(rows), tl_cmp(rows))
    for rows in ((64, 8192) if N == 1024 else (8192,)):
        for name, c, launches in (("null", None, 1), ("list", coef, N // 1024)):
            kernel_row("trlwe_expand_dev", {"N": N, "P": N, "k": 12, "coef": name, "launches": launches}, rows, 2 * N, W1, tr_exp(rows, c), tr_cmp(rows, c))
    if N == 1024:
        for rows in (16, 8192, 131072):
            upload_row("tlwe_rows_from_pinned_host", {"n": n, "k": 10}, rows, n1, W0, tl_exp(rows))
        for rows in (1, 64, 8192):
            upload_row("trlwe_rows_from_pinned_host", {"N": N, "P": N, "k": 12}, rows, 2 * N, W1, tr_exp(rows, None))
    else:
        upload_row("trlwe_rows_from_pinned_host", {"N": N, "P": N, "k": 12}, 8192, 2 * N, W1, tr_exp(8192, None))
    e.close()
