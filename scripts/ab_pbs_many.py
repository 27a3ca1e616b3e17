#!/usr/bin/env python3
"""Same-process A/B of the many-LUT PBS against the single-output PBS (device buffers, one engine per N): legs alternate round by round --
pbs_batch_dev twice (against itself: the noise floor) and pbs_many_batch_dev with 1, 2 and 4 outputs per gate, all on four random tables
picked by random indices (n_out = 1: words compared with pbs_batch_dev's).  Device events around each leg.
usage: ab_pbs_many.py [--steps 20] [--warmup 3]     (shapes: 1,024 / 8,192 gates at N = 1024, 1,024 at N = 2048)"""
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

for N, counts in ((1024, (1024, 8192)), (2048, (1024,))):
    P = R.Params(N=N)
    key0, key1, bk, ksk = R.keygen(P, 20261016)
    e = R.Engine(P, 0)
    e.load_bk_torus(bk); e.load_ksk(ksk)
    rng = np.random.default_rng(N)
    G = max(counts)
    d_in = torch.from_numpy(R.encrypt_bits(P, key0, rng.integers(0, 2, G).astype(np.uint8), 1).view(np.int32)).cuda()
    d_idx = torch.from_numpy(rng.integers(0, 4, G).astype(np.int32)).cuda()
    lut4 = e.lut(rng.integers(0, 1 << 32, (4, N), dtype=np.uint64).astype(np.uint32))
    for c in counts:
        outs = {"pbs": torch.empty_like(d_in), "pbs_again": torch.empty_like(d_in)}
        for k in (1, 2, 4):
            outs["many%d" % k] = torch.empty((G, k, P.n + 1), dtype=torch.int32, device="cuda")
        legs = {
            "pbs": lambda o: e.pbs_batch_dev(lut4, d_in, o, c, d_idx, st.cuda_stream),
            "pbs_again": lambda o: e.pbs_batch_dev(lut4, d_in, o, c, d_idx, st.cuda_stream),
            "many1": lambda o: e.pbs_many_batch_dev(lut4, d_in, o, c, 1, d_idx, st.cuda_stream),
            "many2": lambda o: e.pbs_many_batch_dev(lut4, d_in, o, c, 2, d_idx, st.cuda_stream),
            "many4": lambda o: e.pbs_many_batch_dev(lut4, d_in, o, c, 4, d_idx, st.cuda_stream),
        }
        for name, f in legs.items():
            for _ in range(args.warmup): f(outs[name])
        e.sync(st.cuda_stream)
        times = {k: [] for k in legs}
        for r in range(args.rounds):
            for name, f in legs.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(st)
                for _ in range(per_round): f(outs[name])
                b.record(st)
                b.synchronize()
                times[name].append(a.elapsed_time(b) / per_round)
        e.sync(st.cuda_stream)
        med = {k: float(np.median(v)) for k, v in times.items()}
        print(json.dumps({"N": N, "gates": c, "steps_per_leg": per_round * args.rounds, **{k + "_ms": round(v, 4) for k, v in med.items()},
                          "pbs_vs_itself_pct": round((med["pbs_again"] / med["pbs"] - 1) * 100, 2),
                          **{"many%d_vs_pbs_pct" % k: round((med["many%d" % k] / med["pbs"] - 1) * 100, 2) for k in (1, 2, 4)},
                          "many4_outputs_per_s": round(4 * c / med["many4"] * 1e3, 1),
                          "many1_words_equal_pbs": bool(torch.equal(outs["many1"][:c, 0], outs["pbs"][:c]))}), flush=True)
    lut4.close(); e.close()
