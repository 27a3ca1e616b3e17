"""TEST INFRASTRUCTURE: what the mask-length modules share (tests/test_gpu_mask_lengths.py, tests/test_gpu_mask_lengths_mb.py,
tests/test_gpu_mask_lengths_round.py): the TLWE dimensions n at which every family's LDS carve, step count and dispatch change, the gates
of a batch the oracle is asked about, and one key set with its default engine per (N, n).  rustfhe_amd is imported inside the functions, as in
gpu_kit.py.

Mask lengths: 1, 2 (fewer steps than any prefetch depth); 63 / 639 / 703 / 767 (n + 1 == npad, npad = n + 1 rounded up to 64: the body word is
the last word of its LDS row); 64 / 640 / 704 (one word into a new 64-block, n + 1 odd); 639 -> 640 (six -> five gates per CU time-sliced);
703 -> 704 (four -> three gates per CU at N = 2048); 767 (the maximum rtfhe_ctx_create accepts)."""
import numpy as np

import gpu_kit as gk

MASKS = {1024: (1, 2, 63, 64, 639, 640, 767), 2048: (1, 63, 64, 703, 704, 767)}
ALL = [(N, n) for N in (1024, 2048) for n in MASKS[N]]
# small first: a carve or ring defect shows at n = 63 / 64 before the degenerate step counts and the long masks run
ORDER = sorted(ALL, key=lambda m: (m[1] in (1, 2), m[1] > 64, m[0], m[1]))
RANDOM_PICKS = 8
# the launch shapes an engine can be forced into at creation, and the mask lengths they run at: 1, 63, 64 and the largest of the ring plus the
# first n past the change of the dispatch (640: five gates per CU time-sliced; 704: three gates per CU in the N = 2048 whole rounds)
FORCED = {1024: [{"RTFHE_FORCE_WAVES": "1"}, {"RTFHE_FORCE_WAVES": "2"}, {"RTFHE_FORCE_WAVES": "4"}, {"RTFHE_FORCE_WAVES": "8"},
                 {"RTFHE_PAIR4": "0"}, {"RTFHE_PAIR_RR": "0"}, {"RTFHE_KS_MM_MIN": "0"}],
          2048: [{"RTFHE_FORCE_WAVES": "4"}, {"RTFHE_N2048_EO4": "0"}]}
FORCED_MASKS = {1024: (1, 63, 64, 640, 767), 2048: (1, 63, 64, 704, 767)}


def boundary_picks(count, N, C):
    """first and last gate, the last gate before and the first after every segment boundary the dispatch can make at this size (multiples of
    4C: whole rounds, and where the time-sliced launch starts; N = 2048 also multiples of 3C: the whole rounds of the longest masks)"""
    s = {0, count - 1}
    for per in ((4,) if N == 1024 else (3, 4)):
        for b in range(per * C, count, per * C):
            s |= {b - 1, b}
    return sorted(s)


def _picks(count, N, C, rng):
    """boundary_picks and RANDOM_PICKS more drawn at random"""
    s = set(boundary_picks(count, N, C))
    rest = np.setdiff1d(np.arange(count), sorted(s))
    s |= set(rng.choice(rest, min(RANDOM_PICKS, rest.size), replace=False).tolist())
    return sorted(s)


class Mask:
    def __init__(self, orc, N, n):
        import rustfhe_amd as R
        self.orc, self.N, self.n = orc, N, n
        self.P = orc.Params(n=n, N=N)
        self.K = orc.Keys(self.P, 7000 + N + n)
        self.p = R.Params(n=n, N=N)
        self.C = gk.cus()
        self.e = gk.engine(R, self.p, self.K.bk_t, self.K.ksk)

    def engine(self, monkeypatch=None, env=None):
        import rustfhe_amd as R
        return gk.engine(R, self.p, self.K.bk_t, self.K.ksk, monkeypatch, env)

    def gates(self, op, c0, c1, backend=None):
        orc, K = self.orc, self.K
        if backend is None:
            return orc.gate_batch_mt(self.P, op, K.bk_f, None, K.ksk, c0, c1, nthreads=gk.THREADS)[0]
        return orc.gate_batch_mt(self.P, op, None, K.bk_t, K.ksk, c0, c1, nthreads=gk.THREADS, backend=backend)[0]
