#!/usr/bin/env python3
"""Same-process A/B of the many-LUT PBS in rounded decomposition mode against reference mode, which is the yardstick (device buffers, one engine
per N, four random tables picked by random indices, n_out = 4).  Legs alternate round by round: reference, reference again (against itself: the
noise floor and the spread) and rounded.  Device events around each leg; medians and the min .. max of the per-round means.
usage: ab_pbs_round.py [--steps 20] [--warmup 3] [--rounds 5]     (shapes: 1,024 / 8,192 gates at N = 1024, 1,024 at N = 2048)"""
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
N_OUT = 4

for N, counts in ((1024, (1024, 8192)), (2048, (1024,))):
    P = R.Params(N=N)
    key0, key1, bk, ksk = R.keygen(P, 20261018)
    e = R.Engine(P, 0)
    e.load_bk_torus(bk); e.load_ksk(ksk)
    rng = np.random.default_rng(N)
    G = max(counts)
    d_in = torch.from_numpy(R.encrypt_bits(P, key0, rng.integers(0, 2, G).astype(np.uint8), 1).view(np.int32)).cuda()
    d_idx = torch.from_numpy(rng.integers(0, 4, G).astype(np.int32)).cuda()
    lut4 = e.lut(rng.integers(0, 1 << 32, (4, N), dtype=np.uint64).astype(np.uint32))
    for c in counts:
        legs = {"reference": R._ffi.DECOMP_REFERENCE, "reference_again": R._ffi.DECOMP_REFERENCE, "rounded": R._ffi.DECOMP_ROUNDED}
        outs = {k: torch.empty((G, N_OUT, P.n + 1), dtype=torch.int32, device="cuda") for k in legs}

        def run(name):
            e.set_decomposition(legs[name])
            e.pbs_many_batch_dev(lut4, d_in, outs[name], c, N_OUT, d_idx, st.cuda_stream)
        for name in legs:
            for _ in range(args.warmup): run(name)
        e.sync(st.cuda_stream)
        times = {k: [] for k in legs}
        for r in range(args.rounds):
            for name in legs:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(st)
                for _ in range(per_round): run(name)
                b.record(st)
                b.synchronize()
                times[name].append(a.elapsed_time(b) / per_round)
        e.sync(st.cuda_stream)
        e.set_decomposition(R._ffi.DECOMP_REFERENCE)
        med = {k: float(np.median(v)) for k, v in times.items()}
        print(json.dumps({"N": N, "gates": c, "n_out": N_OUT, "steps_per_leg": per_round * args.rounds,
                          **{k + "_ms": round(v, 4) for k, v in med.items()},
                          **{k + "_min_max_ms": [round(min(v), 4), round(max(v), 4)] for k, v in times.items()},
                          "reference_vs_itself_pct": round((med["reference_again"] / med["reference"] - 1) * 100, 2),
                          "rounded_vs_reference_pct": round((med["rounded"] / med["reference"] - 1) * 100, 2),
                          "reference_legs_words_equal": bool(torch.equal(outs["reference"][:c], outs["reference_again"][:c])),
                          "rounded_words_differ": not bool(torch.equal(outs["rounded"][:c], outs["reference"][:c]))}), flush=True)
    lut4.close()
    e.close()
