#!/usr/bin/env python3
"""a < b on encrypted 8-bit numbers in TFHE's leveled mode, no bootstrap in the comparison (include/rtfhe.h: rtfhe_cmux_circuit_create).
The client sends the sixteen bits of a and b as TRGSW ciphertexts (rustfhe_amd.encrypt_selectors).  The server evaluates the reduced decision
diagram of a < b under the interleaved order a7 b7 a6 b6 ... (rustfhe_amd.bdd_netlist): 23 CMUXes on 16 levels where the full tree over sixteen
bits would take 65,535, recorded once as one graph for all replicas and replayed.  The terminals are +-1/8 at coefficient 0 of two plain rows;
the extract form returns one lvl0 ciphertext per comparison, an ordinary encrypted bit that the gates (Engine.gate_batch) accept.

    python examples/bdd_compare.py [replicas]      # random a and b, checked against the plaintext comparison
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rustfhe_amd as R  # noqa: E402

BITS = 8


def less_than_netlist(bits=BITS):
    """Variables 0 .. bits-1 are a (LSB first), bits .. 2 bits-1 are b; one output, coefficient 0 in the extract form."""
    order = [v for i in reversed(range(bits)) for v in (i, bits + i)]
    less = lambda x: int(sum(x[i] << i for i in range(bits)) < sum(x[bits + i] << i for i in range(bits)))  # noqa: E731
    bdd = R.bdd_netlist(2 * bits, less, order)
    net = R.CmuxNetlist(2 * bits)
    for var, hi, lo, rot in bdd.nodes:
        net.node(var, hi, lo, rot)
    net.output(bdd.outputs[0][0], coef=0)
    return net


def terminals(N):
    """rows 0 (true) and 1 (false): +1/8 and -1/8 at coefficient 0"""
    rows = np.zeros((2, N), np.uint32)
    rows[0, 0], rows[1, 0] = 0x20000000, 0xE0000000
    return rows


def client_query(p, key1, a, b, seed=None):
    """-> TRGSW selectors u32[len * 16][2][2l][N]: per replica the bits of a, then of b, least significant first"""
    v = np.stack([np.asarray(a, np.int64), np.asarray(b, np.int64)], axis=1)                     # [count][2]
    bits = ((v[:, :, None] >> np.arange(BITS)) & 1).astype(np.uint8).reshape(-1)
    return R.encrypt_selectors(p, key1, bits, seed=seed)


def server_compare(engine, selectors, count, replays=3):
    """What the server runs: the circuit recorded once, replayed `replays` times.  Returns (lvl0 ciphertexts u32[count][n+1], the netlist,
    device milliseconds of the last replay)."""
    import torch
    net = less_than_netlist()
    st = torch.cuda.current_stream()
    d_out = torch.zeros((count, 1, engine.p.n + 1), dtype=torch.int32, device="cuda")
    with engine.selectors(selectors) as sel, engine.lut(terminals(engine.p.N)) as lut, engine.cmux_circuit(net, sel, lut, d_out, count) as c:
        for _ in range(replays):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(st)
            c.launch(st.cuda_stream)
            t1.record(st)
            engine.sync(st.cuda_stream)
            ms = t0.elapsed_time(t1)
    return d_out.cpu().numpy().view(np.uint32)[:, 0], net, ms


def run(engine, key0, key1, count, seed=None):
    """`count` random pairs.  Returns (a, b, decrypted a < b, decrypted NAND of it with itself, the netlist, milliseconds)."""
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, 1 << BITS, count), rng.integers(0, 1 << BITS, count)
    y, net, ms = server_compare(engine, client_query(engine.p, key1, a, b, seed=seed), count)
    dec = lambda ct: R.decrypt_bits(engine.p, key0, ct).astype(bool)  # noqa: E731
    return a, b, dec(y), dec(engine.gate_batch(R.NAND, y, y)), net, ms


def main():
    count = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    p = R.Params()
    key0, key1, bk, ksk = R.keygen(p)
    eng = R.Engine(p, 0)
    eng.load_bk_torus(bk)                               # for the NAND behind the comparison only
    eng.load_ksk(ksk)
    a, b, got, neg, net, ms = run(eng, key0, key1, count)
    ok = np.array_equal(got, a < b) and np.array_equal(neg, ~(a < b))
    print("%d nodes on %d levels; %d / %d comparisons right; %.3f ms per replay, %.2f us per comparison, %.3g CMUX/s"
          % (net.n_nodes, len(net.levels()), int((got == (a < b)).sum()), count, ms, ms * 1e3 / count, count * net.n_nodes / ms * 1e3))
    eng.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
