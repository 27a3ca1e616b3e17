"""GPU: the multi-bit blind rotation (rtfhe_pbs_mb_batch[_dev]; k_pbs_mb and k_pbs_mb_wg).  Every output word equals tests/mb_oracle.py, key
switch included: the wave kernel at both N over ragged and exact group layouts with planted rotations, the workgroup kernel at N = 1024, one
full-size gate; at full size the two kernels agree word for word, 64 random bits decode at g = 2 and 3 in both decomposition modes; a capture
first thing on a fresh stream replays to the eager words; bad arguments fail before anything is launched."""
import numpy as np
import pytest

import gpu_kit as gk
import mb_oracle as mo
import round_oracle as ro
from kit import random_words

pytestmark = pytest.mark.gpu

MODES = (ro.REFERENCE, ro.ROUNDED)


class World:
    """keys at a small n, the multi-bit keys of both g with their oracle spectra, and one engine with the key-switching key"""

    def __init__(self, orc, N, n):
        import rustfhe_amd as R
        self.orc, self.R = orc, R
        self.P = orc.Params(n=n, N=N)
        self.p = R.Params(n=n, N=N)
        self.plan = orc.Plan(N)
        self.K = orc.Keys(self.P, 0x4D42 + N + n, plan=self.plan)
        self.tab = mo.Tables(R, N)
        self.e = gk.engine(R, self.p, self.K.bk_t, self.K.ksk)
        self.words = {g: R.mbk_keygen(self.p, self.K.key0, self.K.key1, g, seed=100 + g) for g in (2, 3)}
        self.key_f = {g: mo.key_spectra(self.P, self.plan, w) for g, w in self.words.items()}
        self.mbk = {g: self.e.multibit_key(w, g) for g, w in self.words.items()}

    def want(self, g, tv, t, mode):
        return mo.pbs_mb(self.P, self.plan, self.tab, self.key_f[g], self.K.ksk, tv, t, g, mode)

    def close(self):
        for k in self.mbk.values():
            k.close()
        self.e.close()


@pytest.fixture(scope="module")
def worlds(orc):
    w = gk.Worlds(lambda N, n: World(orc, N, n))
    yield w
    w.close()


def inputs(w, g, count, seed):
    """count random ciphertexts; gate 0's first mask words mod-switch to 0, 1, N, 2N - 1, gate 1's first group to rotations summing to 0 mod
    2N; three random tables and an index per gate"""
    N, n = w.P.N, w.P.n
    rng = np.random.default_rng(seed)
    ct = random_words(rng, (count, n + 1))
    ct[0] = mo.plant(w.P, ct[0], [0, 1, N, 2 * N - 1][:n])
    if count > 1:
        ct[1] = mo.plant(w.P, ct[1], ([1, 2 * N - 1] if g == 2 else [1, N, N - 1])[:n])
    return ct, random_words(rng, (3, N)), rng.integers(0, 3, count).astype(np.int32)


def run_dev(e, mbk, lut, ct, idx):
    """the _dev form on the current stream into a guarded buffer"""
    import torch
    count, n1 = ct.shape
    out = gk.guarded_out(count * n1)
    st = torch.cuda.current_stream().cuda_stream
    e.pbs_mb_batch_dev(mbk, lut, gk.to_device(ct, np.uint32), out, count, gk.to_device(idx), st)
    e.sync(st)
    return gk.read_guarded(out, count * n1).reshape(count, n1)


def check_words(w, g, count, shape, monkeypatch, seed):
    """host and _dev forms in both decomposition modes under RTFHE_MB_SHAPE=shape: every word of every gate against the oracle"""
    R = w.R
    ct, tv, idx = inputs(w, g, count, seed)
    monkeypatch.setenv("RTFHE_MB_SHAPE", shape)
    try:
        with w.e.lut(tv) as lut:
            for mode in MODES:
                w.e.set_decomposition(R._ffi.DECOMP_ROUNDED if mode == ro.ROUNDED else R._ffi.DECOMP_REFERENCE)
                want = np.stack([w.want(g, tv[idx[k]], ct[k], mode) for k in range(count)])
                got = w.e.pbs_mb_batch(w.mbk[g], lut, ct, idx)
                assert np.array_equal(got, want), (shape, g, mode, np.argwhere(got != want)[:4])
                assert np.array_equal(run_dev(w.e, w.mbk[g], lut, ct, idx), want), (shape, g, mode, "_dev")
    finally:
        w.e.set_decomposition(R._ffi.DECOMP_REFERENCE)


@pytest.mark.parametrize("g", [2, 3])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 7])
@pytest.mark.parametrize("N", [1024, 2048])
def test_wave_kernel_words_equal_the_oracle(worlds, monkeypatch, N, n, g):
    """count = 5: the second workgroup is partly filled.  n = 1 is a lone ragged group, n = 2 (g = 2) and 3 (g = 3) exact fits, 5 and 7 leave one-
    and two-bit tails."""
    check_words(worlds(N, n), g, 5, "wave", monkeypatch, 1000 * N + 10 * n + g)


@pytest.mark.parametrize("g", [2, 3])
@pytest.mark.parametrize("count", [1, 3])
@pytest.mark.parametrize("n", [5, 7])
def test_workgroup_kernel_words_equal_the_oracle(worlds, monkeypatch, n, count, g):
    check_words(worlds(1024, n), g, count, "wg", monkeypatch, 7000 + 100 * n + 10 * count + g)


def test_default_dispatch_gives_the_same_words_on_both_routes_to_the_key_switch(worlds, monkeypatch):
    """no RTFHE_MB_SHAPE: the workgroup shape at N = 1024 and the wave shape at N = 2048; a context made under RTFHE_KS_MM_MIN=0
    (the kernel switches keys itself) gives the words of the default one (the batch key switch)."""
    for N in (1024, 2048):
        w = worlds(N, 5)
        ct, tv, idx = inputs(w, 2, 3, 31 + N)
        want = np.stack([w.want(2, tv[idx[k]], ct[k], ro.REFERENCE) for k in range(3)])
        with w.e.lut(tv) as lut:
            assert np.array_equal(w.e.pbs_mb_batch(w.mbk[2], lut, ct, idx), want)
        fused = gk.engine(w.R, w.p, w.K.bk_t, w.K.ksk, monkeypatch, {"RTFHE_KS_MM_MIN": "0"})
        try:
            with fused.multibit_key(w.words[2], 2) as k, fused.lut(tv) as lut:
                assert np.array_equal(fused.pbs_mb_batch(k, lut, ct, idx), want)
                for shape in ("wave", "wg")[:2 if N == 1024 else 1]:
                    monkeypatch.setenv("RTFHE_MB_SHAPE", shape)
                    assert np.array_equal(run_dev(fused, k, lut, ct, idx), want), shape
                    monkeypatch.delenv("RTFHE_MB_SHAPE")
        finally:
            fused.close()


# ---- full size: the suite's real key set (n = 635, N = 1024) ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full(engine, keys):
    """the multi-bit keys of the golden key set at g = 2 and 3, uploaded to the session's engine"""
    import rustfhe_amd as R
    words = {g: R.mbk_keygen(engine.p, keys.key0, keys.key1, g, seed=200 + g) for g in (2, 3)}
    before = engine.memory_bytes()
    mbk = {g: engine.multibit_key(w, g) for g, w in words.items()}
    spectra = sum(w.size for w in words.values()) * 4      # 8 bytes per word pair
    assert engine.memory_bytes() - before >= spectra, "rtfhe_ctx_memory_bytes counts the keys"
    yield words, mbk
    for k in mbk.values():
        k.close()


def test_full_size_gate_against_the_oracle_and_workgroup_against_wave(orc, engine, keys, full, monkeypatch):
    """n = 635, g = 2: 318 groups.  One gate against the oracle; count = 3 word for word between the two kernels, at g = 2 and g = 3."""
    import rustfhe_amd as R
    words, mbk = full
    P = keys.p
    plan = orc.Plan(P.N)
    rng = np.random.default_rng(635)
    ct = random_words(rng, (3, P.n + 1))
    tv = random_words(rng, (1, P.N))
    with engine.lut(tv) as lut:
        got = {}
        for g in (2, 3):
            for shape in ("wave", "wg"):
                monkeypatch.setenv("RTFHE_MB_SHAPE", shape)
                got[g, shape] = engine.pbs_mb_batch(mbk[g], lut, ct)
            assert np.array_equal(got[g, "wave"], got[g, "wg"]), g
        monkeypatch.delenv("RTFHE_MB_SHAPE")
    assert not np.array_equal(got[2, "wave"], got[3, "wave"])
    want = mo.pbs_mb(P, plan, mo.Tables(R, P.N), mo.key_spectra(P, plan, words[2]), keys.ksk, tv[0], ct[0], 2)
    assert np.array_equal(got[2, "wave"][0], want)


def test_64_random_bits_decode_at_both_g_in_both_modes(engine, keys, full):
    """The constant-1/8 table on fresh encryptions of random bits, count = 64: every output decodes, for g = 2 and g = 3, reference and rounded;
    rtfhe_pbs_batch on the same inputs decodes all 64 too.  (Measured sigma 0.0034 at g = 2 and 0.0039 at g = 3 in reference mode against the
    margin 1/8; the figures are printed.)"""
    import rustfhe_amd as R
    _, mbk = full
    p = engine.p
    bits = np.random.default_rng(64).integers(0, 2, 64).astype(np.uint8)
    ct = R.encrypt_bits(p, keys.key0, bits, 0x4D43)
    want = np.where(bits == 1, 0x20000000, 0xE0000000).astype(np.uint32)
    with engine.lut(np.full((1, p.N), 0x20000000, np.uint32)) as lut:
        try:
            for mode in (R._ffi.DECOMP_REFERENCE, R._ffi.DECOMP_ROUNDED):
                engine.set_decomposition(mode)
                outs = {"single": engine.pbs_batch(lut, ct), 2: engine.pbs_mb_batch(mbk[2], lut, ct), 3: engine.pbs_mb_batch(mbk[3], lut, ct)}
                for name, out in outs.items():
                    d = (R.phases(p, keys.key0, out) - want).astype(np.uint32).view(np.int32) / 2.0 ** 32
                    print("mode %d %s: phase error rms %.5f max %.5f" % (mode, name, np.sqrt(np.mean(d ** 2)), np.abs(d).max()))
                    assert np.array_equal(R.decrypt_bits(p, keys.key0, out), bits), (mode, name)
        finally:
            engine.set_decomposition(R._ffi.DECOMP_REFERENCE)


def test_pbs_multibit_example(engine, keys, full):
    """examples/pbs_multibit.py: seeded nibbles through PRESENT's S-box at count = 1 and 64, both ways, every one right; the mode is restored."""
    import rustfhe_amd as R
    from kit import load_example
    _, mbk = full
    rows = load_example("pbs_multibit").run(engine, keys.key0, mbk[2], seed=0x5B0D)
    assert [r[0] for r in rows] == [1, 64]
    for count, x, single, t1, multi, t2, want in rows:
        assert np.array_equal(multi, want) and np.array_equal(single, want), count
    assert engine.decomposition() == R._ffi.DECOMP_REFERENCE


# ---- capture, skipped gates, bad arguments ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["wave", "wg"])
def test_capture_first_thing_on_a_fresh_stream_replays_the_eager_words(worlds, monkeypatch, shape):
    import torch
    w = worlds(1024, 7)
    count, n1 = 5, w.P.n + 1
    ct_h, tv, idx_h = inputs(w, 3, count, 77)
    monkeypatch.setenv("RTFHE_MB_SHAPE", shape)
    with w.e.lut(tv) as lut:
        eager = w.e.pbs_mb_batch(w.mbk[3], lut, ct_h, idx_h)
        assert np.array_equal(eager[0], w.want(3, tv[idx_h[0]], ct_h[0], ro.REFERENCE))
        ct, idx = gk.to_device(ct_h, np.uint32), gk.to_device(idx_h)
        out = torch.zeros((count, n1), dtype=torch.int32, device="cuda")
        s = torch.cuda.Stream()      # nothing has run on it
        torch.cuda.synchronize()
        before = w.e.memory_bytes()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(graph, stream=s):
                w.e.pbs_mb_batch_dev(w.mbk[3], lut, ct, out, count, idx, s.cuda_stream)
        assert w.e.memory_bytes() == before, "nothing was allocated inside the capture"
        for _ in range(2):
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert np.array_equal(gk.words_of(out), eager)
        w.e.sync(s.cuda_stream)


@pytest.mark.parametrize("shape", ["wave", "wg"])
def test_bad_table_indices_skip_their_gates_only(worlds, monkeypatch, shape):
    """_dev form: gates with a table index outside [0, 3) are skipped and reported once by sync; every other gate's row is the clean run's, and
    the words behind the output keep their bytes.  The host form refuses the same indices before anything runs."""
    import torch
    w = worlds(1024, 5)
    R = w.R
    count = 6
    ct, tv, idx = inputs(w, 2, count, 78)
    bad = idx.copy()
    bad[[0, 4]] = [3, -1]
    monkeypatch.setenv("RTFHE_MB_SHAPE", shape)
    with w.e.lut(tv) as lut:
        clean = run_dev(w.e, w.mbk[2], lut, ct, idx)
        st = torch.cuda.current_stream().cuda_stream
        out = gk.guarded_out(count * (w.P.n + 1))
        w.e.pbs_mb_batch_dev(w.mbk[2], lut, gk.to_device(ct, np.uint32), out, count, gk.to_device(bad), st)
        with pytest.raises(R.RtfheError) as ei:
            w.e.sync(st)
        assert ei.value.code == R._ffi.ERR_INVALID
        w.e.sync(st)                                    # reported once
        got = gk.read_guarded(out, count * (w.P.n + 1)).reshape(count, -1)
        assert np.array_equal(got[[1, 2, 3, 5]], clean[[1, 2, 3, 5]])
        with pytest.raises(R.RtfheError) as ei:
            w.e.pbs_mb_batch(w.mbk[2], lut, ct, bad)
        assert ei.value.code == R._ffi.ERR_INVALID and "lut_idx[0] = 3" in str(ei.value)


def test_bad_arguments_fail_before_any_launch(worlds):
    import torch
    w = worlds(1024, 5)
    R, e = w.R, w.e
    ct, tv, idx = inputs(w, 2, 3, 79)
    n1 = w.P.n + 1
    st = torch.cuda.current_stream().cuda_stream
    other = gk.engine(R, w.p, w.K.bk_t, w.K.ksk)
    try:
        for g in (1, 4, 0, -3):                                                     # g outside {2, 3}
            with pytest.raises(R.RtfheError) as ei:
                e.multibit_key(w.words[2], g)
            assert ei.value.code == R._ffi.ERR_INVALID and "g = %d" % g in str(ei.value)
        with e.lut(tv) as lut, e.lut_encrypted(random_words(np.random.default_rng(1), (1, 2, w.P.N))) as enc, other.lut(tv) as other_lut, \
                other.multibit_key(w.words[2], 2) as other_key:
            out = gk.guarded_out(3 * n1)
            d_ct = gk.to_device(ct, np.uint32)
            calls = {"an encrypted table": lambda: e.pbs_mb_batch_dev(w.mbk[2], enc, d_ct, out, 3, None, st),
                     "a key of another context": lambda: e.pbs_mb_batch_dev(other_key, lut, d_ct, out, 3, None, st),
                     "a table of another context": lambda: e.pbs_mb_batch_dev(w.mbk[2], other_lut, d_ct, out, 3, None, st)}
            for what, call in calls.items():
                with pytest.raises(R.RtfheError) as ei:
                    call()
                assert ei.value.code == R._ffi.ERR_INVALID, what
            with pytest.raises(R.RtfheError):
                e.pbs_mb_batch(other_key, lut, ct)
            e.sync(st)
            assert (gk.read_guarded(out, 3 * n1) == gk.FILL).all(), "nothing was launched"
            try:                                                                    # the exact backends: the PBS family's refusal
                for b in (R._ffi.BACKEND_NTT_EXACT, R._ffi.BACKEND_FFT_SPLIT_EXACT):
                    e.set_backend(b)
                    with pytest.raises(R.RtfheError) as ei:
                        e.pbs_mb_batch(w.mbk[2], lut, ct)
                    assert ei.value.code == R._ffi.ERR_INVALID and "mirror" in str(ei.value)
            finally:
                e.set_backend(R._ffi.BACKEND_FFT64_MIRROR)
            assert np.array_equal(e.pbs_mb_batch(w.mbk[2], lut, ct)[0], w.want(2, tv[0], ct[0], ro.REFERENCE))      # the context stays usable
        # a key whose context is gone: the call is refused, destroying the handle only frees it
        gone = gk.engine(R, w.p, w.K.bk_t, w.K.ksk)
        key, lut2 = gone.multibit_key(w.words[3], 3), gone.lut(tv)
        gone.close()
        with pytest.raises(R.RtfheError) as ei:
            e.pbs_mb_batch(key, lut2, ct)
        assert ei.value.code in (R._ffi.ERR_STATE, R._ffi.ERR_INVALID)
        key.close()
        lut2.close()
    finally:
        other.close()
