#!/usr/bin/env python3
"""A private histogram in TFHE's leveled mode: encrypted-address WRITES (include/rtfhe.h: rtfhe_demux_tree_batch, rtfhe_lut_accumulate_dev;
DESIGN.md 5.14).  1,024 clients each hold a bucket number in [0, 16) and send its four bits as TRGSW ciphertexts.  The server holds a 16-row
encrypted table of counters.  For client c it demultiplexes the trivial TRLWE of ONE COUNTING UNIT, (u X^slot(c), 0), through a depth-4 CMUX
demultiplexer in the rounded leveled mode -- leaf `bucket` is a TRLWE of the unit, the other fifteen are TRLWEs of 0 -- and adds all sixteen
leaves into the sixteen rows: it never learns which row counted.  The key holder decrypts the rows and reads the 16 counts.

Counter width.  Every write adds one leaf to EVERY row, so a row collects the noise of all writes.  A leaf has passed d = 4 external products:
its noise is at most r(d, N) = sqrt(d (2 l N 18.5^2 2^-50 + (N/2 + 1) 2^-38 / 3)), the rounded leveled mode's bound (noise_bound of
tests/leveled_round_oracle.py; restated below), 1.0e-4 of the torus at d = 4, N = 1024.  After W writes a row's noise is
r sqrt(W): 3.2e-3 at W = 1,024.  The counting unit is u = 2^-B for the largest B whose half unit keeps SIX such deviations,
2^-(B+1) >= 6 r sqrt(W): B = 4 at 1,024 writes (half a unit is 0.031 = 9.8 deviations; B = 5 would leave 4.9), B = 6 at 64 writes.
A B-bit counter wraps at 2^B, and sixteen would be a poor histogram of 1,024 clients; so the row's N coefficients are used as slots: client c
counts at slot c mod S with S = ceil(clients / (2^B - 1)), no coefficient ever receives more than 2^B - 1 units, and the key holder adds the
S decoded slots of a row.  The slot is the client's public index, not its data.

Where the slots sit.  r sqrt(W) holds around coefficient N/2 only.  The selector rows' noise comes from the reference's f32 sampler, whose
mean is about +10 * 2^-32 (include/rtfhe.h, the packing key's note), and the balanced digits -32 .. 31 have a mean of -1/2: their product does
not average out over the writes.  In output coefficient c of a negacyclic product c + 1 terms carry a plus sign and N - 1 - c a minus sign, so
the leftover is proportional to 2 (c + 1) - N: nothing at c = N/2 - 1, largest at both ends, and linear in W.  The restatement on the CPU gives,
after 1,024 writes, an error of rms 2.9e-3 in coefficients 384 .. 639 and 1.3e-2 in the first and the last 128.  The S slots are therefore
the coefficients N/2 - S/2 .. N/2 + S/2 (69 at 1,024 clients: at most 7 % of the ends' leftover).

    python examples/private_histogram.py [clients]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rustfhe_amd as R  # noqa: E402

ADDR_BITS = 4       # 16 buckets
DEVIATIONS = 6.0    # half a counting unit keeps this many standard deviations of a row's noise


def noise_bound(depth, N, l=3):
    """r(d, N) of the rounded leveled mode: per level, the selector rows' 2^-25 noise through 2 l N balanced 6-bit digits (rms
    18.5) plus the rounding error, uniform in +-2^-19, times the binary key."""
    return float(np.sqrt(depth * (2 * l * N * 18.5 ** 2 * 2.0 ** -50 + (N / 2 + 1) * 2.0 ** -38 / 3)))


def counter_bits(writes, N, depth=ADDR_BITS):
    """The largest B with 2^-(B+1) >= DEVIATIONS * noise_bound(depth, N) * sqrt(writes); and the margin it leaves, in deviations."""
    sigma = noise_bound(depth, N) * np.sqrt(writes)
    bits = int(np.floor(-np.log2(DEVIATIONS * sigma))) - 1
    assert bits >= 1, "too many writes for one table: the rows' noise passes half of a one-bit counter's unit"
    return bits, 2.0 ** -(bits + 1) / sigma


def slots_for(clients, bits):
    return -(-clients // ((1 << bits) - 1))


def slot_coefficients(p, clients, bits):
    """The coefficients that hold the slots: slots_for(clients, bits) of them around N/2, where the writes' systematic error vanishes"""
    S = slots_for(clients, bits)
    assert S <= p.N, "more clients than the slots of one table hold"
    return p.N // 2 - S // 2 + np.arange(S)


def client_query(p, key1, buckets, seed=None):
    """bucket numbers in [0, 16) -> TRGSW selectors u32[len * 4][2][2l][N], per client the four address bits, least significant first"""
    buckets = np.asarray(buckets, np.int64)
    bits = ((buckets[:, None] >> np.arange(ADDR_BITS)) & 1).astype(np.uint8).reshape(-1)
    return R.encrypt_selectors(p, key1, bits, seed=seed)


def counting_units(p, clients, bits):
    """What the server demultiplexes, u32[clients][2][N]: for client c the trivial TRLWE of 2^-bits at the coefficient of slot c mod slots"""
    coef = slot_coefficients(p, clients, bits)
    x = np.zeros((clients, 2, p.N), np.uint32)
    x[np.arange(clients), 0, coef[np.arange(clients) % coef.size]] = 1 << (32 - bits)
    return x


def server_update(engine, table, selectors, clients, bits):
    """What the server runs, on device buffers and one stream, in the rounded leveled mode (restored afterwards): the demultiplexer of every
    client's counting unit, then one accumulation of all leaves into the table's 16 rows."""
    import torch
    p = engine.p
    st = torch.cuda.current_stream().cuda_stream
    d_x = torch.from_numpy(counting_units(p, clients, bits).view(np.int32)).cuda()
    d_leaves = torch.zeros((clients, 1 << ADDR_BITS, 2, p.N), dtype=torch.int32, device="cuda")
    before = engine.leveled_decomposition()
    engine.set_leveled_decomposition(R._ffi.DECOMP_ROUNDED)
    try:
        with engine.selectors(selectors) as sel:
            engine.demux_tree_batch_dev(sel, d_x, ADDR_BITS, d_leaves, clients, None, st)       # sel_idx NULL: client c uses selectors 4c .. 4c + 3
            table.accumulate_dev(d_leaves, 0, 1 << ADDR_BITS, clients, st)
            engine.sync(st)
    finally:
        engine.set_leveled_decomposition(before)


def read_counts(p, key1, rows, clients, bits):
    """The key holder: decrypt the 16 rows, round every slot to the nearest multiple of 2^-bits (the whole torus holds the counter: nothing is
    bootstrapped afterwards, so there is no padding bit) and add the slots up."""
    ph = R.trlwe_phase(p, key1, rows)[:, slot_coefficients(p, clients, bits)].astype(np.int64)
    return (((ph + (1 << (31 - bits))) >> (32 - bits)) & ((1 << bits) - 1)).sum(axis=1)


def run(engine, key1, clients, seed=None):
    """`clients` random bucket numbers through the whole protocol.  Returns (the clear histogram, the decoded counts, counter bits)."""
    import torch
    rng = np.random.default_rng(seed)
    p = engine.p
    buckets = rng.integers(0, 1 << ADDR_BITS, clients)
    bits, _ = counter_bits(clients, p.N)
    zeros = R.encrypt_lut(p, key1, np.zeros((1 << ADDR_BITS, p.N), np.uint32), seed=seed)         # the key holder's empty table
    selectors = client_query(p, key1, buckets, seed=seed)
    d_rows = torch.zeros((1 << ADDR_BITS, 2, p.N), dtype=torch.int32, device="cuda")
    with engine.lut_encrypted(zeros) as table:
        server_update(engine, table, selectors, clients, bits)
        table.read_dev(d_rows, 0, 1 << ADDR_BITS)                                                  # the rows leave for the key holder
        engine.sync()
    rows = d_rows.cpu().numpy().view(np.uint32)
    return np.bincount(buckets, minlength=1 << ADDR_BITS), read_counts(p, key1, rows, clients, bits), bits


def main():
    clients = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    p = R.Params()
    _, key1, _, _ = R.keygen(p, want_bk=False, want_ksk=False)
    eng = R.Engine(p, 0)                                # no key is ever loaded: the leveled path needs none
    bits, margin = counter_bits(clients, p.N)
    want, got, _ = run(eng, key1, clients)
    print("%d clients, 16 buckets: %d-bit counters in %d slots per row (half a unit = %.1f deviations of a row's noise), %d external products" %
          (clients, bits, slots_for(clients, bits), margin, clients * ((1 << ADDR_BITS) - 1)))
    print("clear histogram  ", want.tolist())
    print("decoded histogram", got.tolist())
    eng.close()
    sys.exit(0 if np.array_equal(got, want) else 1)


if __name__ == "__main__":
    main()
