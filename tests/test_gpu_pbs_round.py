"""GPU: the rounded gadget decomposition of the PBS family (rtfhe_set_decomposition; the k_pbs_round_* kernels of every FP64-mirror kernel
family).  In rounded mode every PBS entry gives the words of tests/round_oracle.py in every batch shape the dispatch takes; switching back
gives the reference words again; gates, bootstrap_batch and blind_rotate_batch never change; a LUT circuit keeps the mode it was recorded in;
and with the suite's real key set (n = 635, N = 1024) 4-bit messages go through one PBS and 3-bit messages through two."""
import numpy as np
import pytest

import gpu_kit as gk
import round_oracle as ro
from kit import phase_err, random_words
from lut_circuit_kit import create, host_compose, replay

pytestmark = pytest.mark.gpu

# further counts per N = 1024 shape, the smallest existing tests use: the default dispatch takes k_*_pair4 at 600, k_*_pair at 1,024 and
# k_*_pair_rr at 1,280 (k_*_wg serves 1, 5 and 37); without pair4 / pair_rr those counts go to k_*_pair with 3 and 4 gates per workgroup
EXTRA_1024 = {"default": (600, 1024, 1280), "RTFHE_PAIR4=0": (600,), "RTFHE_PAIR_RR=0": (1280,)}
# N = 2048: k_*_eo4 serves up to two gates per CU (1 .. 300), k_*_eo three and four (600, 1,024)
EXTRA_2048 = {"default": (300, 600, 1024), "RTFHE_N2048_EO4=0": (300,)}


class World:
    """n = 24 keys, their spectra and a plan for one N: what round_oracle needs"""

    def __init__(self, orc, N):
        self.orc = orc
        self.P = orc.Params(n=24, N=N)
        self.plan = orc.Plan(N)
        self.K = orc.Keys(self.P, 0x524F + N, plan=self.plan)

    def engine(self, monkeypatch=None, env=None, **kw):
        import rustfhe_amd as R
        return gk.engine(R, R.Params(n=24, N=self.P.N), self.K.bk_t, self.K.ksk, monkeypatch, env, **kw)

    def want(self, row, t, n_out, mode=ro.ROUNDED):
        return ro.pbs_many(self.P, self.plan, self.K.bk_f, self.K.ksk, row, t, n_out, mode)


@pytest.fixture(scope="module")
def worlds(orc):
    return gk.Worlds(lambda N: World(orc, N))


@pytest.fixture(scope="module")
def small(worlds):
    """the n = 24, N = 1024 world with one engine in the default shape"""
    w = worlds(1024)
    e = w.engine()
    yield w, e
    e.close()


def _many_dev(e, lut, ct, n_out, idx, pbs=False):
    """the _dev form of pbs_many_batch (pbs: of pbs_batch) on the current stream"""
    import torch
    G, n1 = ct.shape
    out = torch.zeros((G, n_out, n1), dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    if pbs:
        e.pbs_batch_dev(lut, gk.to_device(ct, np.uint32), out, G, gk.to_device(idx), st)
    else:
        e.pbs_many_batch_dev(lut, gk.to_device(ct, np.uint32), out, G, n_out, gk.to_device(idx), st)
    e.sync(st)
    return out.cpu().numpy().view(np.uint32)


def _check_words(w, e, counts, seed):
    """Rounded mode: pbs_many_batch with every n_out and pbs_batch, plain and encrypted tables, host and _dev forms, against round_oracle on
    the first, the last and one more gate of every batch."""
    import rustfhe_amd as R
    N, n1 = w.P.N, w.P.n + 1
    rng = np.random.default_rng(seed)
    tv = random_words(rng, (3, N))
    trl = random_words(rng, (3, 2, N))      # any words: an encrypted table is data to the kernel
    e.set_decomposition(R._ffi.DECOMP_ROUNDED)
    assert e.decomposition() == R._ffi.DECOMP_ROUNDED
    with e.lut(tv) as plain, e.lut_encrypted(trl) as enc:
        for count in counts:
            ct = random_words(rng, (count, n1))
            idx = rng.integers(0, 3, count).astype(np.int32)
            pick = sorted({0, count - 1, int(rng.integers(0, count))})
            for lut, rows in ((plain, tv), (enc, trl)):
                for n_out in (1, 2, 4, 8):
                    label = (count, "encrypted" if lut is enc else "plain", n_out)
                    out = e.pbs_many_batch(lut, ct, n_out, idx)
                    assert out.shape == (count, n_out, n1)
                    for g in pick:
                        assert np.array_equal(out[g], w.want(rows[idx[g]], ct[g], n_out)), (label, g)
                    assert np.array_equal(_many_dev(e, lut, ct, n_out, idx), out), (label, "_dev")
                    if n_out == 1:
                        assert np.array_equal(e.pbs_batch(lut, ct, idx), out[:, 0]), (label, "pbs_batch")
                        assert np.array_equal(_many_dev(e, lut, ct, 1, idx, pbs=True), out), (label, "pbs_batch_dev")


@pytest.mark.parametrize("env", gk.CONFIGS_1024, ids=gk.env_id)
def test_rounded_words_every_shape_n1024(worlds, monkeypatch, env):
    w = worlds(1024)
    e = w.engine(monkeypatch, env)
    try:
        _check_words(w, e, (1, 5, 37) + EXTRA_1024.get(gk.env_id(env), ()), 1024 + len(gk.env_id(env)))
    finally:
        e.close()


@pytest.mark.parametrize("env", gk.CONFIGS_2048, ids=gk.env_id)
def test_rounded_words_every_shape_n2048(worlds, monkeypatch, env):
    w = worlds(2048)
    e = w.engine(monkeypatch, env)
    try:
        _check_words(w, e, (1, 5, 37) + EXTRA_2048.get(gk.env_id(env), ()), 2048 + len(gk.env_id(env)))
    finally:
        e.close()


def test_switching_back_gives_the_reference_words_again(small):
    import rustfhe_amd as R
    w, e = small
    rng = np.random.default_rng(31)
    count = 37
    tv, trl = random_words(rng, (2, w.P.N)), random_words(rng, (2, 2, w.P.N))
    ct = random_words(rng, (count, w.P.n + 1))
    idx = rng.integers(0, 2, count).astype(np.int32)

    def run(plain, enc):
        return [e.pbs_batch(plain, ct, idx), e.pbs_many_batch(plain, ct, 4, idx), e.pbs_batch(enc, ct, idx), e.pbs_many_batch(enc, ct, 2, idx)]
    with e.lut(tv) as plain, e.lut_encrypted(trl) as enc:
        e.set_decomposition(R._ffi.DECOMP_REFERENCE)
        before = run(plain, enc)
        assert np.array_equal(before[1][0], w.want(tv[idx[0]], ct[0], 4, ro.REFERENCE))
        try:
            e.set_decomposition(R._ffi.DECOMP_ROUNDED)
            rounded = run(plain, enc)
        finally:
            e.set_decomposition(R._ffi.DECOMP_REFERENCE)
        assert e.decomposition() == R._ffi.DECOMP_REFERENCE
        after = run(plain, enc)
    for a, b, r in zip(before, after, rounded):
        assert np.array_equal(a, b)
        assert not np.array_equal(a, r)


def test_gates_bootstrap_and_blind_rotation_ignore_the_mode(small):
    import rustfhe_amd as R
    w, e = small
    rng = np.random.default_rng(32)
    a, b, c = (random_words(rng, (37, w.P.n + 1)) for _ in range(3))

    def run():
        return [e.gate_batch(R.NAND, a, b), e.gate_batch(R.XOR, a, b), e.mux_batch(c, a, b), e.bootstrap_batch(a), e.blind_rotate_batch(a)]
    e.set_decomposition(R._ffi.DECOMP_REFERENCE)
    ref = run()
    assert np.array_equal(ref[0][0], w.orc.gate(w.P, w.plan, w.orc.NAND, w.K.bk_f, None, w.K.ksk, a[0], b[0]))
    try:
        e.set_decomposition(R._ffi.DECOMP_ROUNDED)
        rounded = run()
    finally:
        e.set_decomposition(R._ffi.DECOMP_REFERENCE)
    for x, y in zip(ref, rounded):
        assert np.array_equal(x, y)


def test_a_lut_circuit_keeps_the_mode_it_was_recorded_in(small):
    """One wave of 40 two-output nodes (each the sum of two wires), recorded once per mode; each circuit replays its own mode's words -- the host
    composition through pbs_many_batch in that mode -- whatever the context is set to at replay."""
    import torch
    import rustfhe_amd as R
    w, e = small
    rng = np.random.default_rng(33)
    nodes, n1 = 40, w.P.n + 1
    d = {"fan_in": 2, "in_idx": np.stack([np.arange(nodes), (np.arange(nodes) + 1) % nodes], axis=1).astype(np.int32),
         "weights": np.ones((nodes, 2), np.int32), "cst": random_words(rng, nodes), "lut_idx": rng.integers(0, 2, nodes).astype(np.int32),
         "wave_offsets": np.array([0, nodes], np.int32), "wave_n_out": np.array([2], np.int32),
         "out_idx": (nodes + np.arange(2 * nodes)).astype(np.int32), "num_wires": 3 * nodes}
    start = random_words(rng, (3 * nodes, n1))
    R_, F_ = R._ffi.DECOMP_ROUNDED, R._ffi.DECOMP_REFERENCE
    want, circ, wires = {}, {}, {}
    with e.lut(random_words(rng, (2, w.P.N))) as lut:
        try:
            for mode in (R_, F_):
                e.set_decomposition(mode)
                want[mode] = host_compose(e, lut, d, start)
                wires[mode] = gk.to_device(start, np.uint32)
                circ[mode] = create(e, lut, d, wires[mode])
            assert not np.array_equal(want[R_], want[F_])
            for now in (F_, R_):          # replay both under each setting of the context
                e.set_decomposition(now)
                for mode in (R_, F_):
                    wires[mode].copy_(gk.to_device(start, np.uint32))
                    torch.cuda.synchronize()
                    assert np.array_equal(replay(e, circ[mode], wires[mode]), want[mode]), (now, mode)
        finally:
            e.set_decomposition(F_)
            for c in circ.values():
                e.circuit_destroy(c)
    # LutCircuitRunner(rounded=True) sets the mode around the recording and restores it
    net = R.lut_ripple_adder(2)
    msgs = np.array([[1, 0, 1, 1]])
    rp = R.Params(n=w.P.n, N=w.P.N)
    for rounded in (True, False):
        run = R.LutCircuitRunner(e, net, 1, rounded=rounded)
        run.set_inputs(R.encrypt_torus(rp, w.K.key0, R.encode_msgs(msgs.reshape(-1), 2), seed=5).reshape(1, 4, n1))
        run.run()
        assert e.decomposition() == F_
        assert list(R.decode_msgs(R.phases(rp, w.K.key0, run.outputs()[0]), 2)) == net.evaluate_plain(msgs[0])
        run.close()


# ---- meaning, with the suite's real key set (n = 635, N = 1024).  Every input below is seeded; the same seeds were run through round_oracle
# on the CPU before this file was committed: no wrong output in any of the three tests' rounded legs. -----------------------------------------
def inputs_4bit(R, p, key0):
    """1,024 fresh 4-bit ciphertexts, every message 64 times, and a random permutation of the 16 messages as the table"""
    perm = np.random.default_rng(0x4B17).permutation(16)
    msgs = np.arange(1024) % 16
    return msgs, perm, R.encrypt_torus(p, key0, R.encode_msgs(msgs, 4), seed=0x4B18)


def inputs_3bit(R, p, key0):
    perm = np.random.default_rng(0x3B17).permutation(8)
    msgs = np.arange(1024) % 8
    return msgs, perm, R.encrypt_torus(p, key0, R.encode_msgs(msgs, 3), seed=0x3B18)


def test_4bit_messages_through_one_pbs_and_the_noise_against_reference_mode(engine, keys):
    """Rounded: all 1,024 outputs decode to perm[m].  The same inputs in reference mode: an rms phase error of more than twice the rounded one
    (0.0111 against 0.0025 of the torus; half a 4-bit box is 1/64 = 0.0156)."""
    import rustfhe_amd as R
    p = engine.p
    msgs, perm, ct = inputs_4bit(R, p, keys.key0)
    with engine.lut(R.lut_polynomial(list(perm), p.N, 4)) as lut:
        try:
            engine.set_decomposition(R._ffi.DECOMP_ROUNDED)
            out = engine.pbs_batch(lut, ct)
        finally:
            engine.set_decomposition(R._ffi.DECOMP_REFERENCE)
        ref = engine.pbs_batch(lut, ct)
    er, ef = phase_err(R, p, keys.key0, out, perm[msgs], 4), phase_err(R, p, keys.key0, ref, perm[msgs], 4)
    rms_r, rms_f = float(np.sqrt(np.mean(er ** 2))), float(np.sqrt(np.mean(ef ** 2)))
    print("rounded: rms %.5f max %.5f; reference: rms %.5f max %.5f, %d wrong" %
          (rms_r, np.abs(er).max(), rms_f, np.abs(ef).max(), int(np.sum(R.decode_msgs(R.phases(p, keys.key0, ref), 4) != perm[msgs]))))
    assert np.array_equal(R.decode_msgs(R.phases(p, keys.key0, out), 4), perm[msgs])
    assert rms_f > 2 * rms_r, (rms_f, rms_r)


def test_3bit_messages_through_two_chained_pbs(engine, keys):
    """p = 3: the second PBS reads bootstrapped inputs, whose noise leaves about 9 sigma to half a box (1/32) in rounded mode: all 1,024 right
    after one and after two."""
    import rustfhe_amd as R
    p = engine.p
    msgs, perm, ct = inputs_3bit(R, p, keys.key0)
    with engine.lut(R.lut_polynomial(list(perm), p.N, 3)) as lut:
        try:
            engine.set_decomposition(R._ffi.DECOMP_ROUNDED)
            once = engine.pbs_batch(lut, ct)
            twice = engine.pbs_batch(lut, once)
        finally:
            engine.set_decomposition(R._ffi.DECOMP_REFERENCE)
    assert np.array_equal(R.decode_msgs(R.phases(p, keys.key0, once), 3), perm[msgs])
    assert np.array_equal(R.decode_msgs(R.phases(p, keys.key0, twice), 3), perm[perm[msgs]])


def test_pbs_4bit_example(engine, keys):
    """examples/pbs_4bit.py: 1,024 seeded nibbles through PRESENT's S-box, one PBS each, every one right in rounded mode; the engine's mode is
    restored."""
    import importlib.util
    import os
    import rustfhe_amd as R
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("pbs_4bit", os.path.join(root, "examples", "pbs_4bit.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    x, got, want = ex.run(engine, keys.key0, 1024, seed=0x5B0C)
    assert len(set(x.tolist())) == 16 and np.array_equal(got, want)
    assert engine.decomposition() == R._ffi.DECOMP_REFERENCE


# ---- capture, skipped gates, backends, bad modes ---------------------------------------------------------------------------------------------
def test_capture_and_replay_in_rounded_mode(small):
    """pbs_many_batch_dev in rounded mode inside a caller's capture: refused on a stream without a prior eager call (so is pbs_batch_dev with a
    plain table, which takes the many-LUT path in this mode), accepted after one; the replay gives the eager words, also after the context
    has been switched back (the kernels are baked in)."""
    import torch
    import rustfhe_amd as R
    w, e = small
    rng = np.random.default_rng(34)
    count, n1 = 300, w.P.n + 1
    tv = random_words(rng, (3, w.P.N))
    ct_h = random_words(rng, (count, n1))
    idx_h = rng.integers(0, 3, count).astype(np.int32)
    ct, idx = gk.to_device(ct_h, np.uint32), gk.to_device(idx_h)
    out = torch.zeros((count, 4, n1), dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    try:
        e.set_decomposition(R._ffi.DECOMP_ROUNDED)
        with e.lut(tv) as lut:
            refused = []
            with torch.cuda.stream(s):
                g0 = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g0, stream=s):
                    for call in (lambda: e.pbs_many_batch_dev(lut, ct, out, count, 4, idx, s.cuda_stream),
                                 lambda: e.pbs_batch_dev(lut, ct, out, count, idx, s.cuda_stream)):
                        try:
                            call()
                        except R.RtfheError as err:
                            refused.append(err)
                    out.zero_()
            assert len(refused) == 2 and all(r.code == R._ffi.ERR_STATE and "capture" in str(r) for r in refused)
            e.sync(s.cuda_stream)
            with torch.cuda.stream(s):
                e.pbs_many_batch_dev(lut, ct, out, count, 4, idx, s.cuda_stream)
                e.sync(s.cuda_stream)
                eager = out.clone()
                for g in (0, count - 1):
                    assert np.array_equal(eager[g].cpu().numpy().view(np.uint32), w.want(tv[idx_h[g]], ct_h[g], 4))
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=s):
                    e.pbs_many_batch_dev(lut, ct, out, count, 4, idx, s.cuda_stream)
                for mode in (R._ffi.DECOMP_ROUNDED, R._ffi.DECOMP_REFERENCE):
                    e.set_decomposition(mode)
                    out.zero_()
                    graph.replay()
                    torch.cuda.synchronize()
                    assert torch.equal(out, eager), mode
            e.sync(s.cuda_stream)
    finally:
        e.set_decomposition(R._ffi.DECOMP_REFERENCE)


BAD_LUT_IDX = (-1, 3, 2 ** 31 - 1, -2 ** 31)


def test_bad_table_indices_skip_their_gates_only(small):
    """Rounded mode, _dev forms, plain and encrypted tables: gates with a table index outside [0, 3) are skipped and reported once by sync; every
    other gate's rows are those of the clean run, and the guard rows around the output keep their words."""
    import torch
    import rustfhe_amd as R
    w, e = small
    rng = np.random.default_rng(35)
    G, n1, guard = 300, w.P.n + 1, 8
    tv, trl = random_words(rng, (3, w.P.N)), random_words(rng, (3, 2, w.P.N))
    ct = random_words(rng, (G, n1))
    idx = rng.integers(0, 3, G).astype(np.int32)
    bad = np.array([0, 5, 63, 64, G - 1])
    bad_idx = idx.astype(np.int64)
    bad_idx[bad] = [BAD_LUT_IDX[k % 4] for k in range(bad.size)]
    bad_idx = bad_idx.astype(np.int32)
    valid = np.ones(G, bool)
    valid[bad] = False
    st = torch.cuda.current_stream().cuda_stream

    def run(lut, n_out, pbs, indices):
        fill = random_words(rng, (G * n_out + 2 * guard, n1))
        big = gk.to_device(fill, np.uint32)
        rows = big[guard:guard + G * n_out]
        if pbs:
            e.pbs_batch_dev(lut, gk.to_device(ct, np.uint32), rows, G, gk.to_device(indices), st)
        else:
            e.pbs_many_batch_dev(lut, gk.to_device(ct, np.uint32), rows, G, n_out, gk.to_device(indices), st)
        return big, fill
    try:
        e.set_decomposition(R._ffi.DECOMP_ROUNDED)
        with e.lut(tv) as plain, e.lut_encrypted(trl) as enc:
            for lut, n_out, pbs in ((plain, 1, True), (plain, 4, False), (enc, 1, True), (enc, 2, False)):
                big, fill = run(lut, n_out, pbs, idx)
                e.sync(st)
                clean = big.cpu().numpy().view(np.uint32)[guard:guard + G * n_out].reshape(G, n_out, n1).copy()
                assert np.array_equal(clean[1], w.want((trl if lut is enc else tv)[idx[1]], ct[1], n_out))
                big, fill = run(lut, n_out, pbs, bad_idx)
                with pytest.raises(R.RtfheError) as ei:
                    e.sync(st)
                assert ei.value.code == R._ffi.ERR_INVALID
                e.sync(st)                                    # reported once
                got = big.cpu().numpy().view(np.uint32)
                assert np.array_equal(got[guard:guard + G * n_out].reshape(G, n_out, n1)[valid], clean[valid])
                assert np.array_equal(got[:guard], fill[:guard]) and np.array_equal(got[guard + G * n_out:], fill[guard + G * n_out:])
    finally:
        e.set_decomposition(R._ffi.DECOMP_REFERENCE)


def test_exact_backends_still_refuse_pbs_and_accept_the_setter(small):
    import rustfhe_amd as R
    w, e = small
    rng = np.random.default_rng(36)
    ct = random_words(rng, (5, w.P.n + 1))
    tv = random_words(rng, (1, w.P.N))
    with e.lut(tv) as lut:
        try:
            for b in (R._ffi.BACKEND_NTT_EXACT, R._ffi.BACKEND_FFT_SPLIT_EXACT):
                e.set_backend(b)
                for mode in (R._ffi.DECOMP_ROUNDED, R._ffi.DECOMP_REFERENCE, R._ffi.DECOMP_ROUNDED):
                    e.set_decomposition(mode)
                    assert e.decomposition() == mode
                for call in (lambda: e.pbs_batch(lut, ct), lambda: e.pbs_many_batch(lut, ct, 2)):
                    with pytest.raises(R.RtfheError) as ei:
                        call()
                    assert ei.value.code == R._ffi.ERR_INVALID and "mirror" in str(ei.value)
        finally:
            e.set_backend(R._ffi.BACKEND_FFT64_MIRROR)
        try:      # the mode set on an exact backend is in force on the mirror
            assert e.decomposition() == R._ffi.DECOMP_ROUNDED
            assert np.array_equal(e.pbs_batch(lut, ct)[0], w.want(tv[0], ct[0], 1)[0])
        finally:
            e.set_decomposition(R._ffi.DECOMP_REFERENCE)


def test_bad_modes_are_refused_and_leave_the_context_clean(small):
    import rustfhe_amd as R
    w, e = small
    for start in (R._ffi.DECOMP_ROUNDED, R._ffi.DECOMP_REFERENCE):
        e.set_decomposition(start)
        for bad in (2, -1, 255, 1 << 30):
            with pytest.raises(R.RtfheError) as ei:
                e.set_decomposition(bad)
            assert ei.value.code == R._ffi.ERR_INVALID and "decomposition" in str(ei.value)
            assert e.decomposition() == start
        e.sync()


def test_multi_entry_context_sets_every_entry(small):
    import rustfhe_amd as R
    w, e = small
    rng = np.random.default_rng(37)
    count = 301
    tv = random_words(rng, (2, w.P.N))
    ct = random_words(rng, (count, w.P.n + 1))
    idx = rng.integers(0, 2, count).astype(np.int32)
    multi = w.engine(devices=[0, 0])
    try:
        multi.set_decomposition(R._ffi.DECOMP_ROUNDED)
        e.set_decomposition(R._ffi.DECOMP_ROUNDED)
        with multi.lut(tv) as ml, e.lut(tv) as sl:
            ref = e.pbs_many_batch(sl, ct, 2, idx)
            assert np.array_equal(ref[count - 1], w.want(tv[idx[count - 1]], ct[count - 1], 2))
            assert np.array_equal(multi.pbs_many_batch(ml, ct, 2, idx), ref)
            assert np.array_equal(multi.pbs_batch(ml, ct, idx), e.pbs_batch(sl, ct, idx))
            assert np.array_equal(_many_dev(multi, ml, ct, 2, idx), ref)
    finally:
        e.set_decomposition(R._ffi.DECOMP_REFERENCE)
        multi.close()
