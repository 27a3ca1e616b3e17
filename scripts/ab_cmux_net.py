#!/usr/bin/env python3
"""Same-process A/B of CMUX netlists (Engine.cmux_circuit) against the two entry points they generalise, legs alternating round by round:
cmux_tree_netlist(4) at 8,192 replicas and cmux_tree_netlist(10) at 64 against cmux_tree_batch_dev on the same tables and selectors;
trgsw_rotate_netlist(10) at 1,024 replicas against trgsw_rotate_batch_dev; and the 8-bit comparator (a < b, 23 nodes on 16 levels) at 1,024
and 8,192 replicas in CMUX/s.  Every reference leg runs twice (ref, ref_again): their difference is the spread a netlist leg is read against.
Selectors and rows are random words: the arithmetic does not depend on them.  Device events around each leg.
usage: ab_cmux_net.py [--steps 10] [--warmup 2] [--rounds 5] [--N 1024 2048]"""
import argparse, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import rustfhe_amd as R

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--N", type=int, nargs="+", default=[1024, 2048])
args = ap.parse_args()
per_round = max(1, args.steps // args.rounds)
st = torch.cuda.current_stream()
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


def report(res, med, cmuxes):
    for name, ms in med.items():
        res[name + "_ms"] = round(ms, 4)
        res[name + "_cmux_per_s"] = round(cmuxes / ms * 1e3, 1)
    if "ref" in med:
        res["spread_pct"] = round(abs(med["ref_again"] / med["ref"] - 1) * 100, 2)
        res["net_vs_ref_pct"] = round((med["net"] / med["ref"] - 1) * 100, 2)
    print(json.dumps(res), flush=True)


def comparator(bits):
    order = [v for i in reversed(range(bits)) for v in (i, bits + i)]
    less = lambda b: int(sum(b[i] << i for i in range(bits)) < sum(b[bits + i] << i for i in range(bits)))  # noqa: E731
    return R.bdd_netlist(2 * bits, less, order)


for N in args.N:
    P = R.Params(N=N)
    rng = np.random.default_rng(N)
    e = R.Engine(P, 0)
    sel = e.selectors(words(rng, (N_SEL, 2, 2 * P.l, N)))
    for depth, count in ((4, 8192), (10, 64)):
        rows = 1 << depth
        d_idx = torch.from_numpy(rng.integers(0, N_SEL, (count, depth)).astype(np.int32)).cuda()
        d_ref = torch.zeros((count, 2, N), dtype=torch.int32, device="cuda")
        d_net = torch.zeros((count, 1, 2, N), dtype=torch.int32, device="cuda")
        with e.lut_encrypted(words(rng, (rows, 2, N))) as lut, e.cmux_circuit(R.cmux_tree_netlist(depth), sel, lut, d_net, count, d_idx) as c:
            ref = lambda: e.cmux_tree_batch_dev(sel, lut, depth, d_ref, count, d_idx, None, st.cuda_stream)  # noqa: E731
            med = timed({"ref": ref, "net": lambda: c.launch(st.cuda_stream), "ref_again": ref})
            e.sync(st.cuda_stream)
            assert torch.equal(d_ref, d_net[:, 0]), "the netlist's tree and the tree entry disagree"
        report({"N": N, "shape": "tree", "depth": depth, "replicas": count, "nodes": rows - 1, "levels": depth}, med, count * (rows - 1))
    depth, count = 10, 1024
    d_idx = torch.from_numpy(rng.integers(0, N_SEL, (count, depth)).astype(np.int32)).cuda()
    d_row0 = torch.arange(count, dtype=torch.int32, device="cuda")
    trlwe = words(rng, (count, 2, N))
    d_in = torch.from_numpy(trlwe.view(np.int32)).cuda()
    d_ref = torch.zeros((count, 2, N), dtype=torch.int32, device="cuda")
    d_net = torch.zeros((count, 1, 2, N), dtype=torch.int32, device="cuda")
    with e.lut_encrypted(trlwe) as lut, e.cmux_circuit(R.trgsw_rotate_netlist(depth), sel, lut, d_net, count, d_idx, d_row0) as c:
        ref = lambda: e.trgsw_rotate_batch_dev(sel, d_in, depth, d_ref, count, d_idx, None, st.cuda_stream)  # noqa: E731
        med = timed({"ref": ref, "net": lambda: c.launch(st.cuda_stream), "ref_again": ref})
        e.sync(st.cuda_stream)
        assert torch.equal(d_ref, d_net[:, 0]), "the netlist's chain and the rotation entry disagree"
    report({"N": N, "shape": "rotate", "depth": depth, "replicas": count, "nodes": depth, "levels": depth}, med, count * depth)
    net = comparator(8)
    sel16 = e.selectors(words(rng, (16, 2, 2 * P.l, N)))
    for count in (1024, 8192):
        d_idx = torch.from_numpy(np.tile(np.arange(16, dtype=np.int32), (count, 1))).cuda()
        d_net = torch.zeros((count, 1, 2, N), dtype=torch.int32, device="cuda")
        with e.lut(words(rng, (2, N))) as lut, e.cmux_circuit(net, sel16, lut, d_net, count, d_idx) as c:
            med = timed({"net": lambda: c.launch(st.cuda_stream)})
            e.sync(st.cuda_stream)
        report({"N": N, "shape": "compare8", "replicas": count, "nodes": net.n_nodes, "levels": len(net.levels())}, med, count * net.n_nodes)
    sel16.close()
    sel.close()
    e.close()
