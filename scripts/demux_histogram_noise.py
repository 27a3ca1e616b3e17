#!/usr/bin/env python3
"""CPU only: the noise of accumulated demultiplexer writes.  examples/private_histogram.py's server side restated with
tests/leveled_oracle.py's oracle_demux_tree in rounded leveled mode (bit-exact with k_demux_tree), the accumulation as a numpy sum:
`writes` clients, 16 rows, full parameter set.  Prints the error of the accumulated rows against the clear counts -- over all coefficients, by
bands of 128 coefficients (the part that does not average out grows with the distance from N/2) and in the example's slots -- beside
r(4, N) sqrt(writes) and half a counting unit.
usage: demux_histogram_noise.py [writes = 1024]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "examples")):
    sys.path.insert(0, d)
import numpy as np
import orc, round_oracle as ro
import rustfhe_amd as R
import private_histogram as ex
from leveled_oracle import oracle_demux_tree
from pbs_oracle import bk_fft

orc.build()
writes = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
rp, p = R.Params(), orc.Params()
plan = orc.Plan(p.N)
_, key1, _, _ = R.keygen(rp, 5, want_bk=False, want_ksk=False)
buckets = np.random.default_rng(1).integers(0, 16, writes)
bits, margin = ex.counter_bits(writes, rp.N)
x = ex.counting_units(rp, writes, bits)
rows = R.encrypt_lut(rp, key1, np.zeros((16, rp.N), np.uint32), seed=3).copy()
for c in range(writes):
    sel_f = bk_fft(orc, p, plan, ex.client_query(rp, key1, buckets[c:c + 1], seed=100 + c).reshape(-1))
    rows += oracle_demux_tree(orc, p, plan, sel_f, range(4), x[c], ro.ROUNDED)
got, want = ex.read_counts(rp, key1, rows, writes, bits), np.bincount(buckets, minlength=16)
coef = ex.slot_coefficients(rp, writes, bits)
clear = np.zeros((16, rp.N), np.int64)
np.add.at(clear, (buckets, coef[np.arange(writes) % coef.size]), 1 << (32 - bits))
err = ((R.trlwe_phase(rp, key1, rows).astype(np.int64) - clear + 2 ** 31) % 2 ** 32 - 2 ** 31) / 2.0 ** 32
print("writes %d  N %d  counter bits %d  slots %d (coefficients %d .. %d)  histogram decoded %s" %
      (writes, rp.N, bits, coef.size, coef[0], coef[-1], "right" if np.array_equal(got, want) else "WRONG"))
print("r(4, N) sqrt(writes) = %.3e   half a unit = %.3e (%.1f deviations)" % (ex.noise_bound(4, rp.N) * np.sqrt(writes), 2.0 ** -(bits + 1), margin))
print("all coefficients: rms %.3e  max %.3e" % (err.std(), np.abs(err).max()))
for lo in range(0, rp.N, 128):
    print("coefficients %4d .. %4d: rms %.3e" % (lo, lo + 127, err[:, lo:lo + 128].std()))
print("the slots: rms %.3e  max %.3e" % (err[:, coef].std(), np.abs(err[:, coef]).max()))
