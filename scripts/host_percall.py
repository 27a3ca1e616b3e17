#!/usr/bin/env python3
"""Per-call host time of two leveled entry points, on the checkout given as argv[1] (its own rustfhe_amd package and library; A/B: run it once
per checkout, alternating, RTFHE_LIB pointing at that checkout's library so that nothing is rebuilt): 1,000 back-to-back
rtfhe_trlwe_mul_trgsw_batch_dev calls (count = 1, K = 1, one sync at the end) and 1,000 rtfhe_tlwe_dense_batch host-form calls at 1 x 1, wall
clock, five rounds each after a warm-up.  Also prints what rtfhe_ctx_memory_bytes reports afterwards and the pack entry point's refusals."""
import json
import os
import sys
import time

root = os.path.abspath(sys.argv[1])
sys.path.insert(0, root)
import numpy as np
import torch
import rustfhe_amd as R

assert os.path.abspath(R.__file__).startswith(root), R.__file__
CALLS, ROUNDS = 1000, 5
p = R.Params()
eng = R.Engine(p, 0)
L = eng.L
rng = np.random.default_rng(5)
N = p.N
sel = eng.selectors(rng.integers(0, 1 << 32, (1, 2, 2 * p.l, N), dtype=np.uint64).astype(np.uint32))
d_x = torch.zeros((1, 2, N), dtype=torch.int32, device="cuda")
d_out = torch.zeros((1, 2, N), dtype=torch.int32, device="cuda")
xp, op = d_x.data_ptr(), d_out.data_ptr()


def mac_round(n):
    t = time.perf_counter()
    for _ in range(n):
        rc = L.rtfhe_trlwe_mul_trgsw_batch_dev(eng.h, sel.h, None, xp, 1, None, 1, 0, op, 1, None)
    eng.sync()
    dt = time.perf_counter() - t
    assert rc == 0
    return dt / n * 1e6


dense = eng.dense(np.ones((1, 1), np.int32))
x = rng.integers(0, 1 << 32, (1, 1, p.n + 1), dtype=np.uint64).astype(np.uint32)
out = np.zeros((1, 1, p.n + 1), np.uint32)
hx, ho = x.ctypes.data, out.ctypes.data


def dense_round(n):
    t = time.perf_counter()
    for _ in range(n):
        rc = L.rtfhe_tlwe_dense_batch(eng.h, dense.h, hx, None, 0, ho, 1)
    dt = time.perf_counter() - t
    assert rc == 0
    return dt / n * 1e6


mac_round(300)
dense_round(300)
mac = [round(mac_round(CALLS), 3) for _ in range(ROUNDS)]
den = [round(dense_round(CALLS), 3) for _ in range(ROUNDS)]
assert np.array_equal(out, x), "1 x 1 dense layer with W = 1 returns its input"
# the other host forms once each at small shapes, then what the staging buffers hold
row = rng.integers(0, 1 << 32, (2, 2, N), dtype=np.uint64).astype(np.uint32)
eng.trlwe_mul_trgsw_batch(sel, row[:1], K=1)
pp = eng.plain_polys(np.eye(1, N, dtype=np.int32))
eng.trlwe_mul_plain_batch(pp, row, K=1, w_idx=[0, 0], x_idx=[1, 0], acc=row)
mem = eng.memory_bytes()
print(json.dumps({"tree": root, "mac_dev_us_per_call": mac, "mac_dev_median": float(np.median(mac)), "dense_host_us_per_call": den,
                  "dense_host_median": float(np.median(den)), "memory_bytes_after": mem}), flush=True)
pp.close()
dense.close()
sel.close()
eng.close()

# the pack entry point's refusals (before any device work), full text
small = R.Params(n=8, N=1024)
e2 = R.Engine(small, 0)
pk = e2.packing_key(rng.integers(0, 1 << 32, R.engine.packing_key_words(small), dtype=np.uint64).astype(np.uint32))
tl = np.zeros((4, small.n + 1), np.uint32)
o2 = np.zeros((1, 2, 1024), np.uint32)
for P, pos, rep, count in [(0, None, 1, 1), (1025, None, 1, 1), (1, None, 0, 1), (1, None, 1025, 1), (1, None, 1, 1 << 31), (3, [0, -1, 5], 1, 1), (3, [0, 1, 2048], 1, 1),
                           (4, None, 1024, 1)]:
    a = None if pos is None else np.ascontiguousarray(pos, np.int32)
    rc = e2.L.rtfhe_pack_batch(e2.h, pk.h, tl.ctypes.data, P, None if a is None else a.ctypes.data, rep, o2.ctypes.data, count)
    print("pack", (P, pos, rep, count), "->", rc, repr(e2.L.rtfhe_last_error(e2.h).decode()), flush=True)
rc = e2.L.rtfhe_pack_batch(e2.h, pk.h, None, 1, None, 1, o2.ctypes.data, 1)
print("pack null in ->", rc, repr(e2.L.rtfhe_last_error(e2.h).decode()), flush=True)
pk.close()
e2.close()
