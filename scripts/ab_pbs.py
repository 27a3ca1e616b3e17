#!/usr/bin/env python3
"""Same-process A/B of the programmable bootstrap against the gate path's bootstrap (device buffers, one engine per N): legs alternate
round by round -- bootstrap_batch_dev twice (the gate path against itself: the noise floor), pbs_batch_dev with the constant 1/8 table
(words compared with the gate path's) and with four random tables picked by random indices.  Device events around each leg.
usage: ab_pbs.py [--steps 20] [--warmup 3]     (shapes: 1,024 / 1,280 / 8,192 gates at N = 1024, 1,024 at N = 2048)"""
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

for N, counts in ((1024, (1024, 1280, 8192)), (2048, (1024,))):
    P = R.Params(N=N)
    key0, key1, bk, ksk = R.keygen(P, 20261016)
    e = R.Engine(P, 0)
    e.load_bk_torus(bk); e.load_ksk(ksk)
    rng = np.random.default_rng(N)
    G = max(counts)
    d_in = torch.from_numpy(R.encrypt_bits(P, key0, rng.integers(0, 2, G).astype(np.uint8), 1).view(np.int32)).cuda()
    d_idx = torch.from_numpy(rng.integers(0, 4, G).astype(np.int32)).cuda()
    lut1 = e.lut(np.full(N, 0x20000000, np.uint32))
    lut4 = e.lut(rng.integers(0, 1 << 32, (4, N), dtype=np.uint64).astype(np.uint32))
    for c in counts:
        outs = {k: torch.empty_like(d_in) for k in ("gate", "gate_again", "pbs_1_table", "pbs_4_tables")}
        legs = {
            "gate": lambda o: e.bootstrap_batch_dev(d_in, o, c, st.cuda_stream),
            "gate_again": lambda o: e.bootstrap_batch_dev(d_in, o, c, st.cuda_stream),
            "pbs_1_table": lambda o: e.pbs_batch_dev(lut1, d_in, o, c, None, st.cuda_stream),
            "pbs_4_tables": lambda o: e.pbs_batch_dev(lut4, d_in, o, c, d_idx, st.cuda_stream),
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
                          "gate_vs_itself_pct": round((med["gate_again"] / med["gate"] - 1) * 100, 2),
                          "pbs_1_table_vs_gate_pct": round((med["pbs_1_table"] / med["gate"] - 1) * 100, 2),
                          "pbs_4_tables_vs_gate_pct": round((med["pbs_4_tables"] / med["gate"] - 1) * 100, 2),
                          "pbs_gates_per_s": round(c / med["pbs_4_tables"] * 1e3, 1),
                          "constant_table_words_equal_gate": bool(torch.equal(outs["pbs_1_table"][:c], outs["gate"][:c]))}), flush=True)
    lut1.close(); lut4.close(); e.close()
