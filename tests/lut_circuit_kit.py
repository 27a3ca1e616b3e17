"""TEST INFRASTRUCTURE: what the tests of LUT circuits share (rtfhe_lut_circuit_create; tests/test_gpu_lut_circuit.py, and the tests that
replay a circuit in another decomposition mode, at another mask length or from an encrypted table): the circuit's semantics composed on the
host, creation from a description, one replay, random circuits, and the adder's inputs and decoding."""
import numpy as np


def host_compose(e, lut, d, wires):
    """rtfhe.h's LUT-circuit semantics on the host: per wave the weighted sums in numpy (wrapping u32), then Engine.pbs_many_batch."""
    w = np.array(wires, np.uint32, copy=True)
    F = d["fan_in"]
    idx, wt = np.asarray(d["in_idx"]).reshape(-1, F), np.asarray(d["weights"]).reshape(-1, F)
    cst = np.zeros(idx.shape[0], np.uint32) if d["cst"] is None else np.asarray(d["cst"], np.uint32)
    offs, n_out, out_idx = d["wave_offsets"], d["wave_n_out"], np.asarray(d["out_idx"])
    row = 0
    for v in range(len(n_out)):
        lo, hi, th = int(offs[v]), int(offs[v + 1]), int(n_out[v])
        t = np.zeros((hi - lo, w.shape[1]), np.uint32)
        for k in range(F):
            used = idx[lo:hi, k] >= 0
            t[used] += wt[lo:hi, k][used].astype(np.uint32)[:, None] * w[idx[lo:hi, k][used]]
        t[:, -1] += cst[lo:hi]
        li = None if d["lut_idx"] is None else np.asarray(d["lut_idx"])[lo:hi]
        out = e.pbs_many_batch(lut, t, th, li).reshape(-1, w.shape[1])
        w[out_idx[row:row + out.shape[0]]] = out
        row += out.shape[0]
    return w


def create(e, lut, d, wires):
    return e.lut_circuit_create(lut, d["fan_in"], d["in_idx"], d["weights"], d["cst"], d["lut_idx"], d["wave_offsets"], d["wave_n_out"],
                                d["out_idx"], wires, d["num_wires"])


def replay(e, c, wires):
    e.circuit_launch(c)
    e.sync()
    return wires.cpu().numpy().view(np.uint32).copy()


def random_circuit(rng, fan_in, replicas, n_tables=3):
    """Per replica: 6 input wires, then waves (level 1: n_out 1, then 4; level 2: 2, then 8; level 3: a pair of n_out = 1 nodes that swap two
    wires in place) with one node per replica each, except the swap.  Random weights, constants, table indices and used slots."""
    inputs = 6
    plan = [(1, 1), (4, 1), (2, 1), (8, 1), (1, 2)]        # (n_out, nodes per replica)
    W = inputs + sum(th * k for th, k in plan[:-1])
    in_idx, wts, cst, lut_idx, out_idx, offs, n_out = [], [], [], [], [], [0], []
    avail = list(range(inputs))
    nxt = inputs
    level_new = []
    for v, (th, k) in enumerate(plan):
        if v in (2, 4):                                      # a new level: what the previous one wrote becomes readable
            avail += level_new
            level_new = []
        swap = v == len(plan) - 1
        outs = [[nxt + j * th + i for i in range(th)] for j in range(k)] if not swap else [[avail[-1]], [avail[-2]]]
        srcs = [None] * k if not swap else [[avail[-2]], [avail[-1]]]
        for r in range(replicas):
            for j in range(k):
                used = rng.integers(1, fan_in + 1)
                ws = list(rng.choice(avail, used)) if srcs[j] is None else srcs[j] * used
                in_idx.append([r * W + x for x in ws] + [-1] * (fan_in - used))
                wts.append(list(rng.integers(-(1 << 31), 1 << 31, used)) + list(rng.integers(-5, 5, fan_in - used)))
                cst.append(int(rng.integers(0, 1 << 32)))
                lut_idx.append(int(rng.integers(0, n_tables)))
                out_idx.extend(r * W + o for o in outs[j])
        if not swap:
            level_new += [o for oo in outs for o in oo]
            nxt += th * k
        offs.append(offs[-1] + replicas * k)
        n_out.append(th)
    perm = rng.permutation(fan_in)                          # unused slots anywhere, not only at the end
    in_idx = np.array(in_idx, np.int64)[:, perm]
    wts = np.array(wts, np.int64)[:, perm]
    return {"fan_in": fan_in, "in_idx": in_idx.astype(np.int32), "weights": wts.astype(np.int32), "cst": np.array(cst, np.uint32),
            "lut_idx": np.array(lut_idx, np.int32), "wave_offsets": np.array(offs, np.int32), "wave_n_out": np.array(n_out, np.int32),
            "out_idx": np.array(out_idx, np.int32), "num_wires": replicas * W}


def adder_inputs(R, p, key0, reps, seed):
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, 256, reps), rng.integers(0, 256, reps)
    bits = np.concatenate([(a[:, None] >> np.arange(8)) & 1, (b[:, None] >> np.arange(8)) & 1], axis=1)
    return a, b, R.encrypt_torus(p, key0, R.encode_msgs(bits.reshape(-1), 2), seed=seed).reshape(reps, 16, p.n + 1)


def decode(R, p, key0, out):
    bits = R.decode_msgs(R.phases(p, key0, out.reshape(-1, p.n + 1)), 2).reshape(out.shape[0], -1)
    return (bits << np.arange(bits.shape[1])).sum(axis=1)
