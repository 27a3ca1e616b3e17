#!/usr/bin/env python3
"""Same-process A/B of the leveled entry points in rounded decomposition mode (Engine.set_leveled_decomposition) against reference mode, which
is the yardstick.  Legs alternate round by round: reference, reference again (against itself: the noise floor and the spread) and rounded.
Shapes: cmux_tree_batch_dev at depth 10 x 64 lookups and depth 4 x 8,192; trgsw_rotate_batch_dev at depth 10 x 1,024 and x 8,192; the 8-bit
comparator of examples/bdd_compare.py (a < b, 23 nodes on 16 levels) as a CMUX circuit at 1,024 replicas, one circuit recorded per leg.
Selectors and rows are random words: the arithmetic does not depend on them.  Device events around each leg; medians and the min .. max of the
per-round means.
usage: ab_leveled_round.py [--steps 10] [--warmup 2] [--rounds 5] [--N 1024 2048]"""
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
MODES = {"reference": R._ffi.DECOMP_REFERENCE, "reference_again": R._ffi.DECOMP_REFERENCE, "rounded": R._ffi.DECOMP_ROUNDED}


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
    return times


def report(res, times, cmuxes, outs):
    med = {k: float(np.median(v)) for k, v in times.items()}
    print(json.dumps({**res, "cmuxes": cmuxes, "steps_per_leg": per_round * args.rounds,
                      **{k + "_ms": round(v, 4) for k, v in med.items()},
                      **{k + "_min_max_ms": [round(min(v), 4), round(max(v), 4)] for k, v in times.items()},
                      "reference_cmux_per_s": round(cmuxes / med["reference"] * 1e3, 1),
                      "reference_vs_itself_pct": round((med["reference_again"] / med["reference"] - 1) * 100, 2),
                      "rounded_vs_reference_pct": round((med["rounded"] / med["reference"] - 1) * 100, 2),
                      "reference_legs_words_equal": bool(torch.equal(outs["reference"], outs["reference_again"])),
                      "rounded_words_differ": not bool(torch.equal(outs["rounded"], outs["reference"]))}), flush=True)


def comparator(bits):
    order = [v for i in reversed(range(bits)) for v in (i, bits + i)]
    less = lambda b: int(sum(b[i] << i for i in range(bits)) < sum(b[bits + i] << i for i in range(bits)))  # noqa: E731
    return R.bdd_netlist(2 * bits, less, order)


for N in args.N:
    P = R.Params(N=N)
    rng = np.random.default_rng(N)
    e = R.Engine(P, 0)
    sel = e.selectors(words(rng, (N_SEL, 2, 2 * P.l, N)))

    def in_mode(name, call):
        def leg():
            e.set_leveled_decomposition(MODES[name])
            call(name)
        return leg

    for depth, count in ((10, 64), (4, 8192)):
        rows = 1 << depth
        d_idx = torch.from_numpy(rng.integers(0, N_SEL, (count, depth)).astype(np.int32)).cuda()
        outs = {k: torch.zeros((count, 2, N), dtype=torch.int32, device="cuda") for k in MODES}
        with e.lut_encrypted(words(rng, (rows, 2, N))) as lut:
            times = timed({k: in_mode(k, lambda k: e.cmux_tree_batch_dev(sel, lut, depth, outs[k], count, d_idx, None, st.cuda_stream)) for k in MODES})
            e.sync(st.cuda_stream)
        report({"N": N, "shape": "tree", "depth": depth, "lookups": count}, times, count * (rows - 1), outs)
    depth = 10
    for count in (1024, 8192):
        d_idx = torch.from_numpy(rng.integers(0, N_SEL, (count, depth)).astype(np.int32)).cuda()
        d_in = torch.from_numpy(words(rng, (count, 2, N)).view(np.int32)).cuda()
        outs = {k: torch.zeros((count, 2, N), dtype=torch.int32, device="cuda") for k in MODES}
        times = timed({k: in_mode(k, lambda k: e.trgsw_rotate_batch_dev(sel, d_in, depth, outs[k], count, d_idx, None, st.cuda_stream)) for k in MODES})
        e.sync(st.cuda_stream)
        report({"N": N, "shape": "rotate", "depth": depth, "lookups": count}, times, count * depth, outs)
    net = comparator(8)
    count = 1024
    d_idx = torch.from_numpy(np.tile(np.arange(16, dtype=np.int32), (count, 1))).cuda()
    outs = {k: torch.zeros((count, 1, 2, N), dtype=torch.int32, device="cuda") for k in MODES}
    with e.lut(words(rng, (2, N))) as lut:
        circ = {k: e.cmux_circuit(net, sel, lut, outs[k], count, d_idx, rounded=MODES[k] == R._ffi.DECOMP_ROUNDED) for k in MODES}
        times = timed({k: (lambda k=k: circ[k].launch(st.cuda_stream)) for k in MODES})
        e.sync(st.cuda_stream)
        for c in circ.values():
            c.close()
    report({"N": N, "shape": "compare8", "replicas": count, "nodes": net.n_nodes, "levels": len(net.levels())}, times, count * net.n_nodes, outs)
    e.set_leveled_decomposition(R._ffi.DECOMP_REFERENCE)
    sel.close()
    e.close()
