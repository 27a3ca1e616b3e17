#!/usr/bin/env python3
"""Same-process A/B of the CMUX-tree lookup (device buffers): legs alternate round by round -- k_cmux_tree (four waves, one node each, per
workgroup; an 8-wave shape is not built) on a plain and on an encrypted table (a plain table's level 0 has zero a-halves; no kernel skips
their transforms, so the two legs show what such a skip could at most be worth: level 0 is half of all CMUXes) -- and beside them the two-waves-per-gate pair kernel's rate count * n / ms from bootstrap_batch_dev at 1,024
gates.  Selectors and rows are random words: the arithmetic does not depend on them.  Device events around each leg.
usage: ab_cmux_tree.py [--steps 20] [--warmup 3]     (shapes: depth 10 at 64 lookups, depth 4 at 8,192 lookups)"""
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
    engs = {4: R.Engine(P, 0)}
    pair_rate = None
    if N == 1024:      # the pair kernel beside the tree, same process: 1,024 gates of n CMUX steps each
        key0, key1, bk, ksk = R.keygen(P, 20261018)
        e = engs[4]
        e.load_bk_torus(bk); e.load_ksk(ksk)
        d_in = torch.from_numpy(R.encrypt_bits(P, key0, rng.integers(0, 2, 1024).astype(np.uint8), 1).view(np.int32)).cuda()
        d_o = torch.empty_like(d_in)
        ms = timed({"bootstrap": lambda: e.bootstrap_batch_dev(d_in, d_o, 1024, st.cuda_stream)})["bootstrap"]
        pair_rate = 1024 * P.n / ms * 1e3
        print(json.dumps({"N": N, "pair_kernel_gates": 1024, "bootstrap_ms": round(ms, 4), "pair_cmux_per_s": round(pair_rate, 1)}), flush=True)
    sel_t = words(rng, (N_SEL, 2, 2 * P.l, N))
    sels = {w: e.selectors(sel_t) for w, e in engs.items()}
    for depth, count in SHAPES:
        rows = 1 << depth
        plain, enc = words(rng, (rows, N)), words(rng, (rows, 2, N))
        luts = {(w, k): (e.lut(plain) if k == "plain" else e.lut_encrypted(enc)) for w, e in engs.items() for k in ("plain", "enc")}
        d_idx = torch.from_numpy(rng.integers(0, N_SEL, (count, depth)).astype(np.int32)).cuda()
        outs = {key: torch.zeros((count, 2, N), dtype=torch.int32, device="cuda") for key in luts}
        legs = {"w%d_%s" % key: (lambda key=key: engs[key[0]].cmux_tree_batch_dev(sels[key[0]], luts[key], depth, outs[key], count, d_idx, None, st.cuda_stream))
                for key in luts}
        med = timed(legs)
        for e in engs.values(): e.sync(st.cuda_stream)
        cmuxes = count * (rows - 1)
        res = {"N": N, "depth": depth, "lookups": count, "cmuxes": cmuxes, "steps_per_leg": per_round * args.rounds}
        for name, ms in med.items():
            res[name + "_ms"] = round(ms, 4)
            res[name + "_cmux_per_s"] = round(cmuxes / ms * 1e3, 1)
            if pair_rate: res[name + "_vs_pair"] = round(cmuxes / ms * 1e3 / pair_rate, 3)
        res["plain_vs_enc_pct_w4"] = round((med["w4_plain"] / med["w4_enc"] - 1) * 100, 2)
        res["zero_half_skip"] = "not implemented"
        print(json.dumps(res), flush=True)
        for l in luts.values(): l.close()
    for s in sels.values(): s.close()
    for e in engs.values(): e.close()
