#!/usr/bin/env python3
"""An encrypted 8-bit ripple-carry adder on many-LUT programmable bootstrapping (Engine.pbs_many_batch, include/rtfhe.h).

Every bit is a 2-bit message (m * 2^29, rustfhe_amd.encode_msgs).  Level i adds the words of a_i, b_i and the carry c_i -- a plain
wrapping sum of ciphertexts, no bootstrap: its message s = a_i + b_i + c_i lies in [0, 3] -- and ONE many-LUT PBS with two interleaved
functions gives sum_i = s & 1 and c_{i+1} = s >> 1, both again 2-bit messages, so the carry feeds the next level.  8 bootstraps per
addition, against the 72 NAND gates of the NAND-only ripple-carry netlist (BASELINE config 4).  Only the carry is ever a bootstrapped
input; a_i and b_i are fresh encryptions (DESIGN.md 5.5 has the noise budget).

    python examples/pbs_adder.py [replicas]      # random pairs, checked against a + b, and the device time per addition
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rustfhe_amd as R  # noqa: E402

BITS = 8
MSG_BITS = 2


def adder_lut(engine):
    """The one table of the adder: (s & 1, s >> 1) of a 2-bit message s, 2-bit outputs."""
    return engine.lut(R.many_lut_polynomial([lambda s: s & 1, lambda s: s >> 1], engine.p.N, MSG_BITS, out_bits=MSG_BITS))


def encrypt_operands(p, key0, x, seed=None):
    """x: ints in [0, 2^BITS) -> u32[len(x)][BITS][n+1], bit i of x as a 2-bit message (LSB first)."""
    bits = (np.asarray(x, np.int64)[:, None] >> np.arange(BITS)) & 1
    ct = R.encrypt_torus(p, key0, R.encode_msgs(bits.reshape(-1), MSG_BITS), seed=seed)
    return ct.reshape(len(x), BITS, p.n + 1)


def add(engine, lut, ca, cb):
    """Ripple-carry addition of ciphertext arrays u32[count][BITS][n+1] (host buffers): u32[count][BITS + 1][n+1], bit BITS = the carry out."""
    count, n1 = ca.shape[0], ca.shape[2]
    out = np.empty((count, BITS + 1, n1), np.uint32)
    carry = np.zeros((count, n1), np.uint32)          # a trivial encryption of 0
    for i in range(BITS):
        s = ca[:, i] + cb[:, i] + carry                # wrapping u32 sum of the three ciphertexts: message a_i + b_i + c_i
        r = engine.pbs_many_batch(lut, s, 2)
        out[:, i] = r[:, 0]
        carry = r[:, 1]
    out[:, BITS] = carry
    return out


def add_dev(engine, lut, d_a, d_b, d_out, stream=None):
    """The same on the device: torch int32 tensors d_a, d_b [count][BITS][n+1], d_out [count][BITS + 1][n+1]; asynchronous on `stream`.
    Scratch: a sum and a [count][2][n+1] output per level (torch's allocator, so a warm call allocates nothing new)."""
    import torch
    count, n1 = d_a.shape[0], d_a.shape[2]
    carry = torch.zeros((count, n1), dtype=torch.int32, device=d_a.device)
    r = torch.empty((count, 2, n1), dtype=torch.int32, device=d_a.device)
    for i in range(BITS):
        s = (d_a[:, i] + d_b[:, i] + carry).contiguous()      # int32 addition wraps like u32
        engine.pbs_many_batch_dev(lut, s, r, count, 2, stream=stream)
        d_out[:, i] = r[:, 0]
        carry = r[:, 1].clone()
    d_out[:, BITS] = carry


def decode(p, key0, out):
    """u32[count][BITS + 1][n+1] -> the integers"""
    bits = R.decode_msgs(R.phases(p, key0, out.reshape(-1, p.n + 1)), MSG_BITS).reshape(out.shape[0], BITS + 1)
    return (bits << np.arange(BITS + 1)).sum(axis=1)


def main():
    import torch
    replicas = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    p = R.Params()
    key0, key1, bk, ksk = R.keygen(p)
    eng = R.Engine(p, 0)
    eng.load_bk_torus(bk)
    eng.load_ksk(ksk)
    rng = np.random.default_rng()
    a = rng.integers(0, 1 << BITS, replicas)
    b = rng.integers(0, 1 << BITS, replicas)
    ca, cb = encrypt_operands(p, key0, a), encrypt_operands(p, key0, b)
    with adder_lut(eng) as lut:
        got = decode(p, key0, add(eng, lut, ca, cb))
        print("host path: %d / %d additions right" % (int((got == a + b).sum()), replicas))
        d_a = torch.from_numpy(ca.view(np.int32)).cuda()
        d_b = torch.from_numpy(cb.view(np.int32)).cuda()
        d_out = torch.empty((replicas, BITS + 1, p.n + 1), dtype=torch.int32, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        add_dev(eng, lut, d_a, d_b, d_out, st)       # warm-up
        eng.sync(st)
        times = []
        for _ in range(5):
            eng.timer_begin(st)
            add_dev(eng, lut, d_a, d_b, d_out, st)
            times.append(eng.timer_end(st)[0])
        eng.sync(st)
        got = decode(p, key0, d_out.cpu().numpy().view(np.uint32))
        ms = float(np.median(times))
        print("device path: %d / %d right; %.3f ms per batch of %d additions (median of 5), %.4f ms per addition, 8 bootstraps each"
              % (int((got == a + b).sum()), replicas, ms, replicas, ms / replicas))
    eng.close()


if __name__ == "__main__":
    main()
