#!/usr/bin/env python3
"""The encrypted 8-bit ripple-carry adder of examples/pbs_adder.py as ONE recorded LUT circuit (rustfhe_amd.lut_circuit; include/rtfhe.h:
rtfhe_lut_circuit_create).  The netlist (lut_ripple_adder) has 8 nodes, one per bit: a_i + b_i + c_i, then one many-LUT PBS with two functions,
the sum bit and the carry.  Recorded once, every addition of a batch of replicas is one rtfhe_circuit_launch.

    python examples/lut_circuit_adder.py [replicas]      # random pairs, checked against a + b, and the device time per addition
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rustfhe_amd as R  # noqa: E402

BITS = 8
MSG_BITS = 2


def encrypt_inputs(p, key0, a, b, seed=None):
    """ints a, b in [0, 2^BITS) -> u32[len(a)][2 BITS][n+1]: the bits of a then of b (LSB first), each a 2-bit message"""
    bits = np.concatenate([(np.asarray(x, np.int64)[:, None] >> np.arange(BITS)) & 1 for x in (a, b)], axis=1)
    ct = R.encrypt_torus(p, key0, R.encode_msgs(bits.reshape(-1), MSG_BITS), seed=seed)
    return ct.reshape(len(a), 2 * BITS, p.n + 1)


def decode(p, key0, out):
    """u32[count][BITS + 1][n+1] -> the integers"""
    bits = R.decode_msgs(R.phases(p, key0, out.reshape(-1, p.n + 1)), MSG_BITS).reshape(out.shape[0], BITS + 1)
    return (bits << np.arange(BITS + 1)).sum(axis=1)


def run(engine, key0, replicas, seed=None, timed=5):
    """Adds `replicas` random pairs with one replay; then `timed` more replays under the device timer.  Returns (a, b, sums, ms per replay)."""
    import torch
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << BITS, replicas)
    b = rng.integers(0, 1 << BITS, replicas)
    runner = R.LutCircuitRunner(engine, R.lut_ripple_adder(BITS), replicas)
    try:
        runner.set_inputs(encrypt_inputs(engine.p, key0, a, b, seed=seed))
        runner.run()                                    # records the circuit, then replays it once
        got = decode(engine.p, key0, runner.outputs())
        st = torch.cuda.current_stream().cuda_stream
        times = []
        for _ in range(timed):
            engine.timer_begin(st)
            runner.launch(st)
            times.append(engine.timer_end(st)[0])
        engine.sync(st)
    finally:
        runner.close()
    return a, b, got, float(np.median(times)) if times else None


def main():
    replicas = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    p = R.Params()
    key0, key1, bk, ksk = R.keygen(p)
    eng = R.Engine(p, 0)
    eng.load_bk_torus(bk)
    eng.load_ksk(ksk)
    a, b, got, ms = run(eng, key0, replicas)
    print("%d / %d additions right; %.3f ms per replay of %d additions (median of 5), %.4f ms per addition, 8 bootstraps each"
          % (int((got == a + b).sum()), replicas, ms, replicas, ms / replicas))
    eng.close()


if __name__ == "__main__":
    main()
