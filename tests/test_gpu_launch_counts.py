"""GPU: how many kernels a batch enqueues, on every backend and ring -- the ladder of rtfhe_dispatch_fft.hip / _ntt.hip / _xfft.hip counted rung
by rung with the counter rtfhe_timer_end returns (every bootstrap launch and every batch key switch adds one).

A batch of G gates on a device of C CUs is cut into whole rounds of R gates per CU and a remainder; the expected counts below restate only that
arithmetic and the knobs that change the NUMBER of launches, read off the dispatch code:

  every default shape   a MODE_GATE batch takes the split path: the ladder in MODE_EXTRACT, then ONE k_key_switch_mm (KS = 1); a many-LUT PBS, an
                        encrypted table and the rounded decomposition run the same ladder in MODE_EXTRACT and one key switch of count * n_out rows
  whole rounds          one launch for all of them (full = G // (R C) * R C gates), R = 4 except N = 2048: the mirror backend's eo_round (4 at
                        n = 635: three only from n = 704), the split-FFT backend's 2
  the remainder         one launch, whichever kernel serves it (wg / pair<2|3|4> / pair4 / eo / eo4 / ntt_wg / ntt_pair / ntt_halves / xpair / xquad)
  time-sliced (RR)      N = 1024, mirror and split-FFT: behind at least one whole round a remainder of up to (RR - 4) C gates rides with the LAST
                        whole round in one launch (k_bootstrap_pair_rr / k_bootstrap_xpair_rr); RR = 6 by default and never below 5 at any mask
                        length, and no batch here needs more than five gates per CU
  RTFHE_FORCE_WAVES=4   one fused launch for the whole batch (mirror, NTT at N = 1024); the NTT backend at N = 2048 ignores it

One batch per backend and ring is also compared word for word with a forced single-shape engine (the mirror backend with itself, the two exact
backends with the NTT backend's forced shape at N = 1024 and with each other at N = 2048: their words are equal by construction)."""
import numpy as np
import pytest

import gpu_kit as gk
from kit import keys_2048, random_words

pytestmark = pytest.mark.gpu

KS = 1           # the batch key switch behind the ladder (k_key_switch_mm, one launch up to 2 GiB of samples)
RR = 5           # gates per CU the time-sliced launch is sure to take (the default is 6; 5 fits at every mask length)
BACKENDS = ("mirror", "ntt", "xfft")


def _sizes(C):
    return [1, C, C + 1, 2 * C + 1, 3 * C + 1, 4 * C, 4 * C + 1, 5 * C, 8 * C + 1]


def _ladder(G, C, R, rr=0):
    """launches of the ladder: whole rounds of R gates per CU + the remainder; rr: gates per CU of a time-sliced launch (0: none)"""
    round_ = R * C
    full, rem = G // round_ * round_, G % round_
    if rr > R and full and rem and round_ + rem <= rr * C:
        return (1 if full > round_ else 0) + 1
    return (1 if full else 0) + (1 if rem else 0)


def _expected(N, backend, G, C):
    if N == 1024:
        return _ladder(G, C, 4, RR if backend in ("mirror", "xfft") else 0) + KS
    return _ladder(G, C, 2 if backend == "xfft" else 4) + KS


def test_expected_counts_at_256_cus():
    """the formulas, spelled out once for the 256 CUs of an MI355X (no device needed for this one, but it lives with the tests it explains)"""
    C = 256
    assert [_expected(1024, "mirror", G, C) for G in _sizes(C)] == [2, 2, 2, 2, 2, 2, 2, 2, 3]
    assert [_expected(1024, "xfft", G, C) for G in _sizes(C)] == [2, 2, 2, 2, 2, 2, 2, 2, 3]
    assert [_expected(1024, "ntt", G, C) for G in _sizes(C)] == [2, 2, 2, 2, 2, 2, 3, 3, 3]
    assert [_expected(2048, "mirror", G, C) for G in _sizes(C)] == [2, 2, 2, 2, 2, 2, 3, 3, 3]
    assert [_expected(2048, "ntt", G, C) for G in _sizes(C)] == [2, 2, 2, 2, 2, 2, 3, 3, 3]
    assert [_expected(2048, "xfft", G, C) for G in _sizes(C)] == [2, 2, 2, 3, 3, 2, 3, 3, 3]


class World:
    """the default engine of a ring, a forced single-shape engine beside it and one block of random input words shared by every case"""
    def __init__(self, R, N, default, forced, keys):
        self.R, self.N, self.e, self.forced, self.keys = R, N, default, forced, keys
        self.C = gk.cus()
        rng = np.random.default_rng(N)
        self.c0 = random_words(rng, (8 * self.C + 1, default.p.n + 1))
        self.c1 = random_words(rng, (8 * self.C + 1, default.p.n + 1))
        self.forced_out = {}

    def counted(self, e, fn):
        e.timer_begin()
        out = fn()
        return e.timer_end()[1], out

    def on(self, e, backend):
        f = self.R._ffi
        e.set_backend({"mirror": f.BACKEND_FFT64_MIRROR, "ntt": f.BACKEND_NTT_EXACT, "xfft": f.BACKEND_FFT_SPLIT_EXACT}[backend])


@pytest.fixture(scope="module")
def worlds(orc, params, keys, engine):
    import rustfhe_amd as R
    mp = pytest.MonkeyPatch()
    made, engines = {}, []

    def get(N):
        if N not in made:
            if N == 1024:
                K, default = keys, engine
                p = R.Params(n=params.n, N=params.N)
            else:
                K = keys_2048(orc)[1]
                p = R.Params(N=2048)
                default = gk.engine(R, p, K.bk_t, K.ksk)
                engines.append(default)
            forced = gk.engine(R, p, K.bk_t, K.ksk, mp, {"RTFHE_FORCE_WAVES": "4"})
            engines.append(forced)
            made[N] = World(R, N, default, forced, K)
        return made[N]
    yield get
    engine.set_backend(R._ffi.BACKEND_FFT64_MIRROR)
    for e in engines:
        e.close()
    mp.undo()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("N", (1024, 2048))
def test_gate_batches_launch_counts_and_words(worlds, N, backend):
    w = worlds(N)
    R, C, e = w.R, w.C, w.e
    w.on(e, backend)
    try:
        outs = {}
        for G in _sizes(C):
            k, outs[G] = w.counted(e, lambda: e.gate_batch(R.NAND, w.c0[:G], w.c1[:G]))
            print("N = %d %s: %d gates, %d launches" % (N, backend, G, k))
            assert k == _expected(N, backend, G, C), (N, backend, G, k)
        # against one kernel shape for the whole of the largest batch (two whole rounds and a one-gate tail)
        G = 8 * C + 1
        ref_backend = "mirror" if backend == "mirror" else "ntt"
        if ref_backend not in w.forced_out:
            w.on(w.forced, ref_backend)
            k, w.forced_out[ref_backend] = w.counted(w.forced, lambda: w.forced.gate_batch(R.NAND, w.c0, w.c1))
            # (one fused launch; the NTT backend at N = 2048 has no forced shape and walks its ladder)
            assert k == (_expected(N, "ntt", G, C) if (N, ref_backend) == (2048, "ntt") else 1), (N, ref_backend, k)
        # (smaller batches are prefixes of it: every rung's words against the same forced result)
        for G in _sizes(C):
            assert np.array_equal(outs[G], w.forced_out[ref_backend][:G]), (N, backend, G)
    finally:
        w.on(e, "mirror")


@pytest.mark.parametrize("N", (1024, 2048))
def test_pbs_family_launch_counts_on_the_mirror_backend(worlds, N):
    """a many-LUT PBS of 4C + 1 gates (four outputs), an encrypted table on 2C + 1 and the rounded decomposition on 2C + 1: the ladder in
    MODE_EXTRACT (no split path: the ladder is not walked twice) and one key switch over all output rows"""
    w = worlds(N)
    R, C, e = w.R, w.C, w.e
    rng = np.random.default_rng(N + 1)
    w.on(e, "mirror")
    rr = RR if N == 1024 else 0
    with e.lut(random_words(rng, (2, N))) as lut, e.lut_encrypted(random_words(rng, (2, 2, N))) as enc:
        G = 4 * C + 1
        k, many = w.counted(e, lambda: e.pbs_many_batch(lut, w.c0[:G], 4))
        print("N = %d many-LUT: %d gates, %d launches" % (N, G, k))
        assert k == _ladder(G, C, 4, rr) + KS, (N, "many", k)
        G = 2 * C + 1
        k, _ = w.counted(e, lambda: e.pbs_many_batch(enc, w.c0[:G], 2))
        print("N = %d encrypted table: %d gates, %d launches" % (N, G, k))
        assert k == _ladder(G, C, 4, rr) + KS, (N, "enc", k)
        e.set_decomposition(R._ffi.DECOMP_ROUNDED)
        try:
            k, _ = w.counted(e, lambda: e.pbs_many_batch(lut, w.c0[:G], 2))
        finally:
            e.set_decomposition(R._ffi.DECOMP_REFERENCE)
        print("N = %d rounded: %d gates, %d launches" % (N, G, k))
        assert k == _ladder(G, C, 4, rr) + KS, (N, "rounded", k)
        # the many-LUT words once more from the forced single-shape engine (its own table: a table belongs to one context)
        w.on(w.forced, "mirror")
        with w.forced.lut(random_words(np.random.default_rng(N + 1), (2, N))) as flut:
            k, want = w.counted(w.forced, lambda: w.forced.pbs_many_batch(flut, w.c0[:4 * C + 1], 4))
        assert k == 1 + KS, (N, "forced many", k)
        assert np.array_equal(many, want), N
