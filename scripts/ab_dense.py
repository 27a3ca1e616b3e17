#!/usr/bin/env python3
"""Timing of the lvl0 dense layer (Engine.tlwe_dense_batch_dev) at the default n = 635, one process: per shape (I, O, count) the layer runs twice
per round (layer, layer_again: their difference is the spread a figure is read against) beside the bootstrap that follows it in a network,
Engine.pbs_batch_dev of the same count * O samples.  Device events of the library's timer on the stream.  The layer is stated against its
traffic floor -- x read once and out written once, count * (I + O) * (n + 1) * 4 bytes, over the HBM peak, 8.0 TB/s by specification -- and as
a share of the bootstrap's time, the number a user cares about.
Shapes: (784, 32, 1024), (784, 512, 256), (32, 16, 8192), (8, 8, 8192).  Rows, weights and tables are random words: no timing depends on them.
For (8, 8, 8192) the parent's only way to the same sums is a recorded LUT circuit of one wave at fan-in 8; `--circuit STEPS` replays just that
circuit STEPS times, for a kernel trace of its own (rocprofv3 --kernel-trace --stats -- python scripts/ab_dense.py --circuit 20), whose
k_lut_gather line is the figure to compare with.  There is no parent to compare the layer itself with and no pass mark.
usage: ab_dense.py [--steps 20] [--pbs-steps 3] [--warmup 2] [--rounds 5] [--circuit STEPS]"""
import argparse, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import rustfhe_amd as R

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--pbs-steps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--circuit", type=int, default=0)
args = ap.parse_args()
st = torch.cuda.current_stream()
HBM_PEAK = 8.0e12
SHAPES = [(784, 32, 1024), (784, 512, 256), (32, 16, 8192), (8, 8, 8192)]


def words(rng, shape):
    return rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)


def device_words(shape):
    return torch.randint(-2 ** 31, 2 ** 31 - 1, shape, dtype=torch.int32, device="cuda")


def timed(e, legs, per_round):
    """per leg: (median, min, max) over the rounds of ms per call; per_round[name] calls per timed window"""
    for name, f in legs.items():
        for _ in range(args.warmup if per_round[name] > 1 else 1): f()
    e.sync(st.cuda_stream)
    times = {k: [] for k in legs}
    for r in range(args.rounds):
        for name, f in legs.items():
            e.timer_begin(st.cuda_stream)
            for _ in range(per_round[name]): f()
            ms, _ = e.timer_end(st.cuda_stream)
            times[name].append(ms / per_round[name])
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in times.items()}


P_ = R.Params()
n1 = P_.n + 1
rng = np.random.default_rng(28)
key0, key1, bk, ksk = R.keygen(P_, 28)
e = R.Engine(P_, 0)
e.load_bk_torus(bk)
e.load_ksk(ksk)
lut = e.lut(words(rng, (1, P_.N)))

if args.circuit:
    I, O, count = SHAPES[3]
    per = I + O
    W = rng.integers(-128, 128, (O, I)).astype(np.int32)
    in_idx = np.array([[g * per + i for i in range(I)] for g in range(count) for _ in range(O)], np.int32)
    out_idx = np.array([g * per + I + o for g in range(count) for o in range(O)], np.int32)
    d_wires = device_words((count * per, n1))
    c = e.lut_circuit_create(lut, I, in_idx, np.tile(W, (count, 1)), None, None, np.array([0, count * O], np.int32), np.array([1], np.int32), out_idx,
                             d_wires, count * per)
    for _ in range(args.circuit):
        e.circuit_launch(c, st.cuda_stream)
    e.sync(st.cuda_stream)
    e.circuit_destroy(c)
    print(json.dumps({"circuit_replays": args.circuit, "nodes": count * O, "fan_in": I}), flush=True)
else:
    for I, O, count in SHAPES:
        W = rng.integers(-128, 128, (O, I)).astype(np.int32)
        dense = e.dense(W)
        d_x = device_words((count, I, n1))
        d_out = device_words((count, O, n1))
        d_pbs = torch.empty((count * O, n1), dtype=torch.int32, device="cuda")
        layer = lambda: e.tlwe_dense_batch_dev(dense, d_x, d_out, count, None, False, st.cuda_stream)  # noqa: E731
        per_round = {"layer": max(1, args.steps // args.rounds), "pbs": max(1, args.pbs_steps // args.rounds), "layer_again": max(1, args.steps // args.rounds)}
        med = timed(e, {"layer": layer, "pbs": lambda: e.pbs_batch_dev(lut, d_out, d_pbs, count * O, None, st.cuda_stream), "layer_again": layer}, per_round)
        ms, lo, hi = med["layer"]
        pbs = med["pbs"][0]
        floor = count * (I + O) * n1 * 4 / HBM_PEAK * 1e3
        print(json.dumps({"n": P_.n, "I": I, "O": O, "count": count, "layer_ms": round(ms, 4), "layer_min_ms": round(lo, 4), "layer_max_ms": round(hi, 4),
                          "layer_again_ms": round(med["layer_again"][0], 4), "spread_pct": round(abs(med["layer_again"][0] / ms - 1) * 100, 2),
                          "traffic_floor_ms": round(floor, 5), "layer_over_floor": round(ms / floor, 2),
                          "limb_macs_per_s": round(4.0 * count * O * I * n1 / ms * 1e3), "pbs_samples": count * O, "pbs_ms": round(pbs, 3),
                          "layer_share_of_pbs_pct": round(ms / pbs * 100, 3)}), flush=True)
        dense.close()
        del d_x, d_out, d_pbs
lut.close()
e.close()
