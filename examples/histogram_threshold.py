#!/usr/bin/env python3
"""A private histogram the SERVER goes on computing with: examples/private_histogram.py stops where "the rows leave for the key holder",
because a count exists only as a coefficient of a TRLWE.  TRLWE sample extraction (include/rtfhe.h: rtfhe_trlwe_extract_batch_dev; DESIGN.md
5.15) takes that coefficient back to the bootstrapped mode: here the server thresholds every count with one programmable bootstrap and the
key holder receives 16 encrypted flags "bucket b has at least t votes" -- never the counts.

The election is small enough for ONE slot per row: at most 15 voters, at most 7 votes per bucket.  The counting unit is encode_msgs(1, 3) =
2^-4, so a count is a 3-bit PBS message with its padding bit clear, and the slot sits at coefficient N/2 (where the writes' systematic error
vanishes, private_histogram.py).  After private_histogram's accumulation the server runs, on one stream and without leaving the device,

    Lut.read_dev                                   the 16 rows of the table
    trlwe_extract_batch_dev(P = 1, coef = [N/2])   16 lvl0 ciphertexts of the counts
    pbs_batch_dev, table m -> [m >= t]             16 lvl0 ciphertexts of the flags (1-bit outputs), rounded decomposition mode

and the key holder decrypts the flags with key0.

Noise budget at the default parameters (n = 635, N = 1024), from the figures the project already has.  What the PBS's mod switch sees is the
count plus
    the rows' noise     r(4, N) sqrt(W) = 1.0e-4 sqrt(15) = 3.9e-4 after W <= 15 writes (the demultiplexer bound of DESIGN.md 5.13 / 5.14),
    the key switch      rms 2.3e-3 with a mean of -1.8e-3 (measured),
    the mod switch      sqrt((n/2 + 1) / 12) / 2N = 2.5e-3,
3.4e-3 in quadrature.  Half a 3-bit box is 2^-5 = 3.1e-2: less the key switch's mean, 8.6 deviations -- above the 6 this project asks for, so
the message width stays at 3 bits.  The flag is a 1-bit output (half a box 1/8) behind a rounded-mode PBS whose output noise is 3.0e-3
(DESIGN.md 5.12): 40 deviations.

    python examples/histogram_threshold.py [voters] [threshold]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rustfhe_amd as R  # noqa: E402
from private_histogram import ADDR_BITS, client_query, noise_bound, server_update, slot_coefficients  # noqa: E402

MSG_BITS = 3                        # a count is a 3-bit message: at most 2^3 - 1 = 7 votes per bucket
UNIT_BITS = MSG_BITS + 1            # the counting unit 2^-4 = encode_msgs(1, 3): private_histogram's `bits`
MAX_VOTERS = (1 << UNIT_BITS) - 1   # one slot per row holds that many writes (private_histogram.slots_for)
KEY_SWITCH_RMS, KEY_SWITCH_MEAN = 2.3e-3, 1.8e-3      # DESIGN.md 5.12, measured at n = 635, N = 1024
DEVIATIONS = 6.0


def noise_budget(n, N, writes):
    """(sigma of the phase the PBS mod-switches, the margin of half a MSG_BITS box in deviations) from the three figures of the docstring"""
    rows = noise_bound(ADDR_BITS, N) * np.sqrt(writes)
    mod_switch = np.sqrt((n / 2 + 1) / 12.0) / (2 * N)
    sigma = float(np.sqrt(rows ** 2 + KEY_SWITCH_RMS ** 2 + mod_switch ** 2))
    return sigma, (2.0 ** -(MSG_BITS + 2) - KEY_SWITCH_MEAN) / sigma


def draw_votes(rng, voters):
    """bucket numbers of `voters` voters, a few buckets favoured, no bucket above 2^MSG_BITS - 1 votes"""
    assert 1 <= voters <= MAX_VOTERS, "one slot per row holds at most %d writes" % MAX_VOTERS
    weights = np.ones(1 << ADDR_BITS)
    weights[rng.choice(1 << ADDR_BITS, 3, replace=False)] = 8.0
    while True:
        votes = rng.choice(1 << ADDR_BITS, voters, p=weights / weights.sum())
        if np.bincount(votes).max() < (1 << MSG_BITS):
            return votes


def server_threshold(engine, table, threshold):
    """What the server adds to private_histogram.server_update: rows -> counts at lvl0 -> flags, on device buffers and one stream; the
    decomposition mode of the PBS family is set to rounded around the bootstrap and restored.  Returns the 16 flag ciphertexts u32[16][n+1]."""
    import torch
    p = engine.p
    rows_n = 1 << ADDR_BITS
    st = torch.cuda.current_stream().cuda_stream
    d_rows = torch.zeros((rows_n, 2, p.N), dtype=torch.int32, device="cuda")
    d_counts = torch.zeros((rows_n, p.n + 1), dtype=torch.int32, device="cuda")
    d_flags = torch.zeros((rows_n, p.n + 1), dtype=torch.int32, device="cuda")
    tv = R.lut_polynomial(lambda m: int(m >= threshold), p.N, MSG_BITS, out_bits=1)
    before = engine.decomposition()
    engine.set_decomposition(R._ffi.DECOMP_ROUNDED)
    try:
        with engine.lut(tv) as lut:
            table.read_dev(d_rows, 0, rows_n, st)
            engine.trlwe_extract_batch_dev(d_rows, 1, d_counts, rows_n, coef=[p.N // 2], stream=st)
            engine.pbs_batch_dev(lut, d_counts, d_flags, rows_n, None, st)
            engine.sync(st)
    finally:
        engine.set_decomposition(before)
    return d_flags.cpu().numpy().view(np.uint32)


def run(engine, key0, key1, voters=12, threshold=2, seed=None):
    """`voters` votes through the whole protocol on an engine that holds the bootstrapping and the key-switching key of (key0, key1).
    Returns (the clear flags [count >= threshold], the decrypted flags, the clear histogram)."""
    rng = np.random.default_rng(seed)
    p = engine.p
    _, margin = noise_budget(p.n, p.N, voters)
    assert margin >= DEVIATIONS, "half a %d-bit box keeps only %.1f deviations at these parameters: lower MSG_BITS" % (MSG_BITS, margin)
    assert slot_coefficients(p, voters, UNIT_BITS).tolist() == [p.N // 2]
    votes = draw_votes(rng, voters)
    zeros = R.encrypt_lut(p, key1, np.zeros((1 << ADDR_BITS, p.N), np.uint32), seed=seed)         # the key holder's empty table
    selectors = client_query(p, key1, votes, seed=seed)
    with engine.lut_encrypted(zeros) as table:
        server_update(engine, table, selectors, voters, UNIT_BITS)
        flags_ct = server_threshold(engine, table, threshold)
    hist = np.bincount(votes, minlength=1 << ADDR_BITS)
    return (hist >= threshold).astype(np.int64), R.decode_msgs(R.phases(p, key0, flags_ct), 1), hist


def main():
    voters = int(sys.argv[1]) if len(sys.argv) > 1 else 12
    threshold = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    p = R.Params()
    key0, key1, bk, ksk = R.keygen(p)
    eng = R.Engine(p, 0)
    eng.load_bk_torus(bk)
    eng.load_ksk(ksk)
    sigma, margin = noise_budget(p.n, p.N, voters)
    want, got, hist = run(eng, key0, key1, voters, threshold)
    print("%d voters, 16 buckets, threshold %d: counts as %d-bit messages (sigma %.1e, half a box = %.1f deviations)" % (voters, threshold, MSG_BITS, sigma, margin))
    print("clear histogram ", hist.tolist())
    print("clear flags     ", want.tolist())
    print("decrypted flags ", got.tolist())
    eng.close()
    sys.exit(0 if np.array_equal(got, want) else 1)


if __name__ == "__main__":
    main()
