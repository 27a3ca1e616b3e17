#!/usr/bin/env python3
"""Same-process A/B of the 8-bit adder: the eager device path of examples/pbs_adder.py (add_dev: torch adds, pbs_many_batch_dev, slice copies
per bit) against the same netlist as ONE replayed LUT circuit (rustfhe_amd.lut_ripple_adder + LutCircuitRunner).  Legs alternate round by round
-- eager twice (against itself: the noise floor of the run) and the circuit -- with device events around each leg; the outputs of both paths
are compared word for word.
usage: ab_lut_circuit.py [--steps 20] [--warmup 3] [--rounds 5] [--replicas 1024,8192]
       ab_lut_circuit.py --profile      # one recording and ONE replay at 1,024 replicas and nothing else (for rocprofv3 --kernel-trace --stats)"""
import argparse, importlib.util, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import rustfhe_amd as R

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--replicas", default="1024,8192")
ap.add_argument("--profile", action="store_true")
args = ap.parse_args()
per_round = max(1, args.steps // args.rounds)
spec = importlib.util.spec_from_file_location("pbs_adder", os.path.join(ROOT, "examples", "pbs_adder.py"))
ex = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ex)

P = R.Params()
key0, key1, bk, ksk = R.keygen(P, 20261016)
e = R.Engine(P, 0)
e.load_bk_torus(bk); e.load_ksk(ksk)
st = torch.cuda.current_stream()
net = R.lut_ripple_adder(8)

for reps in ([1024] if args.profile else [int(x) for x in args.replicas.split(",")]):
    rng = np.random.default_rng(reps)
    a, b = rng.integers(0, 256, reps), rng.integers(0, 256, reps)
    ca, cb = ex.encrypt_operands(P, key0, a, seed=1), ex.encrypt_operands(P, key0, b, seed=2)
    run = R.LutCircuitRunner(e, net, reps)
    run.set_inputs(np.concatenate([ca, cb], axis=1))
    if args.profile:
        run.run()
        print(json.dumps({"replicas": reps, "profile_replays": 1, "right": int((ex.decode(P, key0, run.outputs()) == a + b).sum())}), flush=True)
        run.close()
        break
    lut = ex.adder_lut(e)
    d_a = torch.from_numpy(ca.view(np.int32)).cuda()
    d_b = torch.from_numpy(cb.view(np.int32)).cuda()
    outs = {k: torch.empty((reps, 9, P.n + 1), dtype=torch.int32, device="cuda") for k in ("eager", "eager_again")}
    legs = {
        "eager": lambda: ex.add_dev(e, lut, d_a, d_b, outs["eager"], st.cuda_stream),
        "eager_again": lambda: ex.add_dev(e, lut, d_a, d_b, outs["eager_again"], st.cuda_stream),
        "circuit": lambda: run.launch(st.cuda_stream),
    }
    for f in legs.values():
        for _ in range(args.warmup): f()
    e.sync(st.cuda_stream)
    times = {k: [] for k in legs}
    for r in range(args.rounds):
        for name, f in legs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(st)
            for _ in range(per_round): f()
            t1.record(st)
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1) / per_round)
    e.sync(st.cuda_stream)
    med = {k: float(np.median(v)) for k, v in times.items()}
    got = run.outputs()
    print(json.dumps({"replicas": reps, "steps_per_leg": per_round * args.rounds, **{k + "_ms": round(v, 4) for k, v in med.items()},
                      **{k + "_ms_per_addition": round(v / reps, 5) for k, v in med.items()},
                      "eager_vs_itself_pct": round((med["eager_again"] / med["eager"] - 1) * 100, 2),
                      "circuit_vs_eager_pct": round((med["circuit"] / med["eager"] - 1) * 100, 2),
                      "spread_pct": {k: round((max(v) / min(v) - 1) * 100, 2) for k, v in times.items()},
                      "circuit_words_equal_eager": bool(np.array_equal(got, outs["eager"].cpu().numpy().view(np.uint32))),
                      "right": int((ex.decode(P, key0, got) == a + b).sum())}), flush=True)
    run.close(); lut.close()
e.close()
