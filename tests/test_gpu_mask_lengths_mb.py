"""GPU: the multi-bit blind rotation (k_pbs_mb<10>, k_pbs_mb<11>, k_pbs_mb_wg and their rounded twins) at the edges of the TLWE dimension n:
the mask lengths of tests/mask_kit.py, where tests/test_gpu_pbs_mb.py holds the words at n <= 7 (npad = 64) and on one gate at n = 635.

n sizes both kernels' LDS carve by npad (n + 1 rounded up to 64): abar is the last region of every wave's slice, and behind the slice of wave 3
the wave kernel has its 32 KiB roots table at N = 1024 and the end of the allocation at N = 2048.  n is also the bit count the groups are cut
from.  The group tails these lengths give:

    n = 1, 2      a lone group (one bit; two bits: exact at g = 2, a two-bit tail at g = 3)
    n = 63        31 groups + a one-bit tail at g = 2, 21 exact at g = 3
    n = 64        32 exact at g = 2, 21 + a one-bit tail at g = 3
    n = 639, 703  319 / 351 + a one-bit tail at g = 2, 213 exact / 234 + a one-bit tail at g = 3
    n = 640, 704  320 / 352 exact at g = 2, 213 + a one-bit tail / 234 + a two-bit tail at g = 3
    n = 767       383 + a one-bit tail at g = 2, 255 + a two-bit tail at g = 3

63 / 639 / 703 / 767: n + 1 == npad, the body word abar[n] is the last word of the wave's slice; 64 / 640 / 704: one word into a new 64-block,
n + 1 odd; 767 the maximum, where the dynamic LDS is largest (147,328 B k_pbs_mb<10>, 146,304 B k_pbs_mb<11>, 120,704 B k_pbs_mb_wg of 163,840:
rtfhe_mbk_create's "no room in LDS" refusal cannot trigger for 1 <= n <= 767, so every mask length must be accepted at both rings -- there is no
try or skip around the key creation).

The wave shape runs count = 5: four live waves in workgroup 0 -- gate 3 is the wave whose slice borders the roots table or the end of the
allocation -- and a partly filled second workgroup.  Every comparison is np.array_equal on uint32 words against tests/mb_oracle.py (all gates
for n <= 64; gates 0, 3, 4 of the wave shape and 0, 2 of the workgroup shape for the long masks) or between two runs of the library: there is no
tolerance in this file."""
import numpy as np
import pytest

import gpu_kit as gk
import mb_oracle as mo
import round_oracle as ro
from kit import random_words
from mask_kit import ORDER

pytestmark = pytest.mark.gpu

MODES = (ro.REFERENCE, ro.ROUNDED)
KS_MASKS = {1024: (63, 64, 640, 767), 2048: (63, 64, 704, 767)}


class World:
    """one key set per (N, n): the oracle's keys, the multi-bit keys of both g with their oracle spectra, one engine with both uploaded"""

    def __init__(self, orc, N, n):
        import rustfhe_amd as R
        self.orc, self.R, self.N, self.n = orc, R, N, n
        self.P = orc.Params(n=n, N=N)
        self.p = R.Params(n=n, N=N)
        self.K = orc.Keys(self.P, 0x4D4C + N + n)
        self.tab = mo.Tables(R, N)
        self.e = gk.engine(R, self.p, self.K.bk_t, self.K.ksk)
        self.words = {g: R.mbk_keygen(self.p, self.K.key0, self.K.key1, g, seed=300 + g) for g in (2, 3)}
        self.key_f = {g: mo.key_spectra(self.P, orc.Plan(N), w) for g, w in self.words.items()}
        self.mbk = {g: self.e.multibit_key(w, g) for g, w in self.words.items()}      # no try / skip: every mask length is accepted
        self.cache = {}

    def want(self, g, tv, idx, ct, gates, mode):
        """the oracle's rows of `gates`, each computed once per world.  One after the other: the restatement is thousands of small numpy
        operations per gate, which the pool's threads only slow down (measured: three gates in 2.1 s on the pool against 0.75 s in turn)"""
        def one(k):
            return gk.memo(self.cache, (g, mode, tv[idx[k]], ct[k]),
                           lambda: mo.pbs_mb(self.P, gk.oracle_plan(self.orc, self.N), self.tab, self.key_f[g], self.K.ksk, tv[idx[k]], ct[k], g, mode))
        return np.stack([one(k) for k in gates])

    def inputs(self, g, count, seed):
        """count random ciphertexts; gate 0's first mask words mod-switch to 0, 1, N, 2N - 1, gate 1's first group to rotations summing to 0 mod
        2N; three random tables and an index per gate"""
        N, n = self.N, self.n
        rng = np.random.default_rng(seed)
        ct = random_words(rng, (count, n + 1))
        ct[0] = mo.plant(self.P, ct[0], [0, 1, N, 2 * N - 1][:n])
        ct[1] = mo.plant(self.P, ct[1], ([1, 2 * N - 1] if g == 2 else [1, N, N - 1])[:n])
        return ct, random_words(rng, (3, N)), rng.integers(0, 3, count).astype(np.int32)

    def set_mode(self, e, mode):
        e.set_decomposition(self.R._ffi.DECOMP_ROUNDED if mode == ro.ROUNDED else self.R._ffi.DECOMP_REFERENCE)

    def close(self):
        for k in self.mbk.values():
            k.close()
        self.e.close()


@pytest.fixture(scope="module", params=ORDER, ids=lambda m: "N%d-n%d" % m)
def world(request, orc):
    """built when the first test of its (N, n) runs and closed behind the last: one long-mask key set is alive at a time (at n = 767, N = 2048,
    g = 3 the words are 176 MB and the oracle's spectra 352 MB)"""
    w = World(orc, *request.param)
    yield w
    w.close()


def run_dev(e, mbk, lut, ct, idx):
    """the _dev form on the current stream into a guarded buffer: the rows, the guard words behind them checked"""
    import torch
    count, n1 = ct.shape
    out = gk.guarded_out(count * n1)
    st = torch.cuda.current_stream().cuda_stream
    e.pbs_mb_batch_dev(mbk, lut, gk.to_device(ct, np.uint32), out, count, gk.to_device(idx), st)
    e.sync(st)
    return gk.read_guarded(out, count * n1).reshape(count, n1)


def _seed(w, g):
    return 100000 * g + 10 * w.N + w.n


@pytest.mark.parametrize("mode", MODES, ids=["reference", "rounded"])
@pytest.mark.parametrize("g", [2, 3])
def test_wave_shape_five_gates_against_the_oracle(world, monkeypatch, g, mode):
    """RTFHE_MB_SHAPE=wave, count = 5, host and _dev form: gates 0, 3 and 4 (all five for n <= 64) equal the oracle word for word, and the two
    forms equal each other on the whole batch."""
    w = world
    ct, tv, idx = w.inputs(g, 5, _seed(w, g))
    gates = list(range(5)) if w.n <= 64 else [0, 3, 4]
    monkeypatch.setenv("RTFHE_MB_SHAPE", "wave")
    try:
        w.set_mode(w.e, mode)
        with w.e.lut(tv) as lut:
            host = w.e.pbs_mb_batch(w.mbk[g], lut, ct, idx)
            dev = run_dev(w.e, w.mbk[g], lut, ct, idx)
    finally:
        w.set_mode(w.e, ro.REFERENCE)
    want = w.want(g, tv, idx, ct, gates, mode)
    bad = [k for k, row in zip(gates, want) if not np.array_equal(host[k], row)]
    assert not bad, ("gates that differ from the oracle", bad)
    assert np.array_equal(dev, host), "_dev"


@pytest.mark.parametrize("mode", MODES, ids=["reference", "rounded"])
@pytest.mark.parametrize("g", [2, 3])
def test_workgroup_shape_three_gates_against_the_oracle_and_the_wave_shape(world, monkeypatch, g, mode):
    """N = 1024, RTFHE_MB_SHAPE=wg, count = 3 (the first three inputs of the wave test), host and _dev form: gates 0 and 2 (all three for
    n <= 64) equal the oracle, and the wave shape's rows for the same three inputs equal these word for word."""
    w = world
    if w.N != 1024:
        return
    ct, tv, idx = w.inputs(g, 5, _seed(w, g))
    ct, idx = ct[:3], idx[:3]
    gates = [0, 1, 2] if w.n <= 64 else [0, 2]
    got = {}
    try:
        w.set_mode(w.e, mode)
        with w.e.lut(tv) as lut:
            for shape in ("wg", "wave"):
                monkeypatch.setenv("RTFHE_MB_SHAPE", shape)
                got[shape] = w.e.pbs_mb_batch(w.mbk[g], lut, ct, idx)
                assert np.array_equal(run_dev(w.e, w.mbk[g], lut, ct, idx), got[shape]), (shape, "_dev")
    finally:
        w.set_mode(w.e, ro.REFERENCE)
    want = w.want(g, tv, idx, ct, gates, mode)
    bad = [k for k, row in zip(gates, want) if not np.array_equal(got["wg"][k], row)]
    assert not bad, ("gates that differ from the oracle", bad)
    assert np.array_equal(got["wave"], got["wg"]), "the wave shape's rows differ from the workgroup shape's"


def test_the_kernels_own_key_switch_gives_the_batch_key_switchs_words(world, monkeypatch):
    """key_switch_wave: a context made under RTFHE_KS_MM_MIN=0 (the kernel switches keys itself, its output row the only store) at n = 63, 64,
    767 and the first n past the change of the dispatch (640 / 704): both shapes, both g and both modes give the default engine's words on the
    whole batch of 5, and the guard words behind d_out keep their fill (run_dev checks them)."""
    w = world
    if w.n not in KS_MASKS[w.N]:
        return
    fused = gk.engine(w.R, w.p, w.K.bk_t, w.K.ksk, monkeypatch, {"RTFHE_KS_MM_MIN": "0"})
    try:
        for g in (2, 3):
            ct, tv, idx = w.inputs(g, 5, _seed(w, g) + 1)
            with fused.multibit_key(w.words[g], g) as key, fused.lut(tv) as flut, w.e.lut(tv) as lut:
                try:
                    for mode in MODES:
                        w.set_mode(w.e, mode)
                        w.set_mode(fused, mode)
                        want = w.e.pbs_mb_batch(w.mbk[g], lut, ct, idx)
                        for shape in ("wave", "wg")[:2 if w.N == 1024 else 1]:
                            monkeypatch.setenv("RTFHE_MB_SHAPE", shape)
                            assert np.array_equal(run_dev(fused, key, flut, ct, idx), want), (g, mode, shape)
                            monkeypatch.delenv("RTFHE_MB_SHAPE")
                finally:
                    w.set_mode(w.e, ro.REFERENCE)
    finally:
        fused.close()


def test_a_skipped_gate_among_odd_length_rows(world, monkeypatch):
    """n = 64 (rows of n + 1 = 65 words), _dev form, count = 6, table indices 3 and -1 on gates 0 and 4, both shapes: reported once by sync, the
    other four rows are the clean run's, the two skipped rows (parked in their sample slots across the batch key switch and put back by
    k_rows_restore) and the words behind the output keep their fill."""
    import torch
    w = world
    if w.n != 64:
        return
    R, n1, count = w.R, w.n + 1, 6
    ct, tv, idx = w.inputs(2, count, _seed(w, 2) + 2)
    bad = idx.copy()
    bad[[0, 4]] = [3, -1]
    st = torch.cuda.current_stream().cuda_stream
    with w.e.lut(tv) as lut:
        for shape in ("wave", "wg")[:2 if w.N == 1024 else 1]:
            monkeypatch.setenv("RTFHE_MB_SHAPE", shape)
            clean = run_dev(w.e, w.mbk[2], lut, ct, idx)
            out = gk.guarded_out(count * n1)
            w.e.pbs_mb_batch_dev(w.mbk[2], lut, gk.to_device(ct, np.uint32), out, count, gk.to_device(bad), st)
            with pytest.raises(R.RtfheError) as ei:
                w.e.sync(st)
            assert ei.value.code == R._ffi.ERR_INVALID, shape
            w.e.sync(st)                                    # reported once
            got = gk.read_guarded(out, count * n1).reshape(count, n1)
            assert np.array_equal(got[[1, 2, 3, 5]], clean[[1, 2, 3, 5]]), shape
            assert (got[[0, 4]] == gk.FILL).all(), (shape, "a skipped gate's row keeps its words behind the batch key switch too")
    assert np.array_equal(clean[1], w.want(2, tv, idx, ct, [1], ro.REFERENCE)[0])


def test_64_random_bits_decode_with_the_long_masks_keys(world):
    """n >= 639: 64 fresh encryptions of random bits through the constant-1/8 table decode at g = 2 and g = 3 in both modes (the assertion of
    test_64_random_bits_decode_at_both_g_in_both_modes, on this world's keys; the default shape of the ring)."""
    w = world
    if w.n < 639:
        return
    R = w.R
    bits = np.random.default_rng(64 + w.n).integers(0, 2, 64).astype(np.uint8)
    ct = R.encrypt_bits(w.p, w.K.key0, bits, 0x4D43 + w.n)
    want = np.where(bits == 1, 0x20000000, 0xE0000000).astype(np.uint32)
    with w.e.lut(np.full((1, w.N), 0x20000000, np.uint32)) as lut:
        try:
            for mode in MODES:
                w.set_mode(w.e, mode)
                for g in (2, 3):
                    out = w.e.pbs_mb_batch(w.mbk[g], lut, ct)
                    d = (R.phases(w.p, w.K.key0, out) - want).astype(np.uint32).view(np.int32) / 2.0 ** 32
                    print("N %d n %d mode %d g %d: phase error rms %.5f max %.5f" % (w.N, w.n, mode, g, np.sqrt(np.mean(d ** 2)), np.abs(d).max()))
                    assert np.array_equal(R.decrypt_bits(w.p, w.K.key0, out), bits), (mode, g)
        finally:
            w.set_mode(w.e, ro.REFERENCE)
