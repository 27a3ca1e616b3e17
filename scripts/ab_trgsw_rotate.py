#!/usr/bin/env python3
"""Same-process A/B of the TRGSW blind rotation (device buffers): legs alternate round by round -- k_trgsw_rotate (four waves, one lookup each,
per workgroup; no other shape is built) at depth 10 on 1,024 and on 8,192 lookups, out of place -- and beside them the two-waves-per-gate pair
kernel's rate count * n / ms from bootstrap_batch_dev at 1,024 gates.  Selectors and rows are random words: the arithmetic does not depend on
them.  Device events around each leg.  There is no pass mark.
usage: ab_trgsw_rotate.py [--steps 20] [--warmup 3]"""
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
DEPTH = 10
COUNTS = (1024, 8192)
N_SEL = 16


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


for N in (1024, 2048):
    P = R.Params(N=N)
    rng = np.random.default_rng(N)
    e = R.Engine(P, 0)
    pair_rate = None
    if N == 1024:      # the pair kernel beside the rotation, same process: 1,024 gates of n CMUX steps each
        key0, key1, bk, ksk = R.keygen(P, 20261018)
        e.load_bk_torus(bk); e.load_ksk(ksk)
        d_in = torch.from_numpy(R.encrypt_bits(P, key0, rng.integers(0, 2, 1024).astype(np.uint8), 1).view(np.int32)).cuda()
        d_o = torch.empty_like(d_in)
        ms = timed({"bootstrap": lambda: e.bootstrap_batch_dev(d_in, d_o, 1024, st.cuda_stream)})["bootstrap"]
        pair_rate = 1024 * P.n / ms * 1e3
        print(json.dumps({"N": N, "pair_kernel_gates": 1024, "bootstrap_ms": round(ms, 4), "pair_cmux_per_s": round(pair_rate, 1)}), flush=True)
    sel = e.selectors(words(rng, (N_SEL, 2, 2 * P.l, N)))
    rot = rng.integers(0, 2 * N, DEPTH).astype(np.int32)
    bufs = {c: (torch.from_numpy(words(rng, (c, 2, N)).view(np.int32)).cuda(), torch.zeros((c, 2, N), dtype=torch.int32, device="cuda"),
                torch.from_numpy(rng.integers(0, N_SEL, (c, DEPTH)).astype(np.int32)).cuda()) for c in COUNTS}
    legs = {"lookups_%d" % c: (lambda c=c: e.trgsw_rotate_batch_dev(sel, bufs[c][0], DEPTH, bufs[c][1], c, bufs[c][2], rot, st.cuda_stream)) for c in COUNTS}
    med = timed(legs)
    e.sync(st.cuda_stream)
    for c in COUNTS:
        ms = med["lookups_%d" % c]
        res = {"N": N, "depth": DEPTH, "lookups": c, "cmuxes": c * DEPTH, "steps_per_leg": per_round * args.rounds, "ms": round(ms, 4),
               "cmux_per_s": round(c * DEPTH / ms * 1e3, 1)}
        if pair_rate: res["vs_pair"] = round(c * DEPTH / ms * 1e3 / pair_rate, 3)
        print(json.dumps(res), flush=True)
    sel.close()
    e.close()
