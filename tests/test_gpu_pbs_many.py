"""GPU: many-LUT programmable bootstrapping (rtfhe_pbs_many_batch[_dev], the k_pbs_many_* kernels of every FP64-mirror kernel family).
With one output it is rtfhe_pbs_batch word for word in every batch shape the dispatch takes; with 2, 4 or 8 outputs it is the oracle's many-LUT PBS
(tests/pbs_oracle.py: oracle_pbs_many) word for word, every shape gives the default shape's words, and encoded functions decrypt."""
import importlib.util
import os

import numpy as np
import pytest

import gpu_kit as gk
from kit import keys_2048, random_words
from pbs_oracle import oracle_pbs_many

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def keys2048(orc):
    return keys_2048(orc)


def _check_shape(e, ref_e, N, n1, counts, seed):
    """theta = 1 against pbs_batch on the same engine; theta = 4 against the reference (default-shape) engine."""
    rng = np.random.default_rng(seed)
    tv = random_words(rng, (3, N))
    with e.lut(tv) as lut, ref_e.lut(tv) as ref_lut:
        for count in counts:
            ct = random_words(rng, (count, n1))
            idx = rng.integers(0, 3, count).astype(np.int32)
            one = e.pbs_many_batch(lut, ct, 1, idx)
            assert one.shape == (count, 1, n1)
            assert np.array_equal(one[:, 0], e.pbs_batch(lut, ct, idx)), count
            if e is not ref_e:
                assert np.array_equal(e.pbs_many_batch(lut, ct, 4, idx), ref_e.pbs_many_batch(ref_lut, ct, 4, idx)), count


@pytest.mark.parametrize("env", gk.CONFIGS_1024, ids=gk.env_id)
def test_one_output_is_pbs_every_shape_n1024(params, keys, engine, monkeypatch, env):
    import rustfhe_amd as R
    p = R.Params(n=params.n, N=params.N)
    e = gk.engine(R, p, keys.bk_t, keys.ksk, monkeypatch, env) if env else engine
    try:
        _check_shape(e, engine, p.N, p.n + 1, (1, 37, 300, 600, 900, 1024, 1280, 2048), 4096)
    finally:
        if e is not engine:
            e.close()


@pytest.mark.parametrize("env", gk.CONFIGS_2048, ids=gk.env_id)
def test_one_output_is_pbs_every_shape_n2048(keys2048, monkeypatch, env):
    import rustfhe_amd as R
    P, K = keys2048
    ref = gk.engine(R, R.Params(N=2048), K.bk_t, K.ksk)
    e = gk.engine(R, R.Params(N=2048), K.bk_t, K.ksk, monkeypatch, env) if env else ref
    try:
        _check_shape(e, ref, P.N, P.n + 1, (1, 37, 300, 600, 1024, 1100), 8192)
    finally:
        if e is not ref:
            e.close()
        ref.close()


def _check_oracle(orc, P, plan, bk_f, ksk, e, count, n_out, seed):
    rng = np.random.default_rng(seed)
    tv = random_words(rng, (3, P.N))
    idx = rng.integers(0, 3, count).astype(np.int32)
    ct = random_words(rng, (count, P.n + 1))
    with e.lut(tv) as lut:
        out = e.pbs_many_batch(lut, ct, n_out, idx)
    assert out.shape == (count, n_out, P.n + 1)
    pick = sorted(set([0, count - 1]) | set(rng.choice(count, min(count, 14), replace=False).tolist()))
    for g in pick:
        assert np.array_equal(out[g], oracle_pbs_many(orc, P, plan, bk_f, ksk, tv[idx[g]], ct[g], n_out)), (g, n_out)


@pytest.mark.parametrize("n_out", [2, 4, 8])
def test_random_tables_against_the_oracle_n1024(orc, params, keys, engine, n_out):
    plan = orc.Plan(params.N)
    for count, seed in ((1, 31), (300, 32), (1024, 33), (1280, 34)):
        _check_oracle(orc, params, plan, keys.bk_f, keys.ksk, engine, count, n_out, seed + 10 * n_out)


@pytest.mark.parametrize("n_out", [2, 4, 8])
def test_random_tables_against_the_oracle_n2048(orc, keys2048, n_out):
    import rustfhe_amd as R
    P, K = keys2048
    e = gk.engine(R, R.Params(N=2048), K.bk_t, K.ksk)
    try:
        _check_oracle(orc, P, orc.Plan(P.N), K.bk_f, K.ksk, e, 1024, n_out, 77 + n_out)
    finally:
        e.close()


def _decode_all(R, p, key0, out, bits):
    return R.decode_msgs(R.phases(p, key0, out.reshape(-1, p.n + 1)), bits).reshape(out.shape[:-1])


@pytest.mark.parametrize("P,fs", [
    (2, [lambda m: m & 1, lambda m: m >> 1]),
    (2, [lambda m: m, lambda m: (m * m) % 4, lambda m: (m + 1) % 4, lambda m: 3 - m]),
    (1, [lambda m: m, lambda m: 1 - m] * 4),
], ids=["p2-two", "p2-four", "p1-eight"])
def test_encoded_functions_decrypt_and_chain(engine, keys, P, fs):
    """4,096 fresh ciphertexts (every message equally often): every output of one many-LUT PBS decodes to f_j(m), and every output of a second
    many-LUT PBS on ALL of those outputs decodes to f_k(f_j(m))."""
    import rustfhe_amd as R
    p = engine.p
    th = len(fs)
    msgs = np.arange(4096) % (1 << P)
    ct = R.encrypt_torus(p, keys.key0, R.encode_msgs(msgs, P), seed=0x4A00 + 16 * P + th)
    with engine.lut(R.many_lut_polynomial(fs, p.N, P)) as lut:
        once = engine.pbs_many_batch(lut, ct, th)
        twice = engine.pbs_many_batch(lut, once.reshape(-1, p.n + 1), th).reshape(len(msgs), th, th, p.n + 1)
    want1 = np.array([[f(m) for f in fs] for m in msgs])
    assert np.array_equal(_decode_all(R, p, keys.key0, once, P), want1)
    want2 = np.array([[[g(f(m)) for g in fs] for f in fs] for m in msgs])
    assert np.array_equal(_decode_all(R, p, keys.key0, twice, P), want2)


def test_eight_bit_adder_example(engine, keys):
    """examples/pbs_adder.py: 1,024 random pairs, 8 many-LUT PBS per addition, every 9-bit sum right."""
    import rustfhe_amd as R
    spec = importlib.util.spec_from_file_location("pbs_adder", os.path.join(ROOT, "examples", "pbs_adder.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    p = engine.p
    rng = np.random.default_rng(0xADD)
    a = rng.integers(0, 256, 1024)
    b = rng.integers(0, 256, 1024)
    ca = ex.encrypt_operands(p, keys.key0, a, seed=0xA1)
    cb = ex.encrypt_operands(p, keys.key0, b, seed=0xB1)
    with ex.adder_lut(engine) as lut:
        out = ex.add(engine, lut, ca, cb)
    assert out.shape == (1024, 9, p.n + 1)
    assert np.array_equal(ex.decode(p, keys.key0, out), a + b)
    assert R.decode_msgs(R.phases(p, keys.key0, out.reshape(-1, p.n + 1)), 2).max() <= 1


def test_bad_n_out_refused(engine):
    import rustfhe_amd as R
    p = engine.p
    ct = np.zeros((4, p.n + 1), np.uint32)
    with engine.lut(np.zeros(p.N, np.uint32)) as lut:
        engine.timer_begin()
        for n_out in (0, 3, 16, -1):
            with pytest.raises(R.RtfheError) as ei:
                engine.pbs_many_batch(lut, ct, n_out)
            assert ei.value.code == R._ffi.ERR_INVALID and "n_out" in str(ei.value)
        assert engine.timer_end()[1] == 0


def test_bad_indices_host_and_device(engine):
    import torch
    import rustfhe_amd as R
    p = engine.p
    rng = np.random.default_rng(18)
    count = 300
    tv = random_words(rng, (2, p.N))
    ct = random_words(rng, (count, p.n + 1))
    idx = rng.integers(0, 2, count).astype(np.int32)
    with engine.lut(tv) as lut:
        ref = engine.pbs_many_batch(lut, ct, 2, idx)
        bad = idx.copy()
        bad[5] = 2
        engine.timer_begin()
        with pytest.raises(R.RtfheError) as ei:
            engine.pbs_many_batch(lut, ct, 2, bad)
        assert ei.value.code == R._ffi.ERR_INVALID and "lut_idx[5]" in str(ei.value)
        assert engine.timer_end()[1] == 0, "the host entry checks before it launches anything"
        bad[7] = -1
        d_ct = torch.from_numpy(ct.view(np.int32)).cuda()
        d_out = torch.zeros((count, 2, p.n + 1), dtype=torch.int32, device="cuda")
        d_bad = torch.from_numpy(bad).cuda()
        st = torch.cuda.current_stream().cuda_stream
        engine.pbs_many_batch_dev(lut, d_ct, d_out, count, 2, d_bad, st)
        with pytest.raises(R.RtfheError) as ei:
            engine.sync(st)
        assert ei.value.code == R._ffi.ERR_INVALID
        out = d_out.cpu().numpy().view(np.uint32)
        keep = np.ones(count, bool)
        keep[[5, 7]] = False
        assert np.array_equal(out[keep], ref[keep])
        engine.sync(st)                                      # reported once
        d_idx = torch.from_numpy(idx).cuda()
        engine.pbs_many_batch_dev(lut, d_ct, d_out, count, 2, d_idx, st)
        engine.sync(st)
        assert np.array_equal(d_out.cpu().numpy().view(np.uint32), ref)


def test_multi_entry_context_matches_single(params, keys, engine):
    import torch
    import rustfhe_amd as R
    p = engine.p
    rng = np.random.default_rng(19)
    G = 4099
    tv = random_words(rng, (4, p.N))
    ct = random_words(rng, (G, p.n + 1))
    idx = rng.integers(0, 4, G).astype(np.int32)
    with engine.lut(tv) as lut:
        ref = engine.pbs_many_batch(lut, ct, 4, idx)
    multi = gk.engine(R, p, keys.bk_t, keys.ksk, devices=[0, 0])
    try:
        with multi.lut(tv) as lut:
            assert np.array_equal(multi.pbs_many_batch(lut, ct, 4, idx), ref)
            d_ct = torch.from_numpy(ct.view(np.int32)).cuda()
            d_out = torch.zeros((G, 4, p.n + 1), dtype=torch.int32, device="cuda")
            d_idx = torch.from_numpy(idx).cuda()
            st = torch.cuda.current_stream().cuda_stream
            multi.pbs_many_batch_dev(lut, d_ct, d_out, G, 4, d_idx, st)
            multi.sync(st)
            assert np.array_equal(d_out.cpu().numpy().view(np.uint32), ref)
    finally:
        multi.close()


def test_graph_capture_replays_eager_words(engine):
    import torch
    p = engine.p
    rng = np.random.default_rng(20)
    count = 600
    tv = random_words(rng, (3, p.N))
    ct = torch.from_numpy(random_words(rng, (count, p.n + 1)).view(np.int32)).cuda()
    idx = torch.from_numpy(rng.integers(0, 3, count).astype(np.int32)).cuda()
    s = torch.cuda.Stream()
    out = torch.zeros((count, 4, p.n + 1), dtype=torch.int32, device="cuda")
    with engine.lut(tv) as lut, torch.cuda.stream(s):
        engine.pbs_many_batch_dev(lut, ct, out, count, 4, idx, s.cuda_stream)
        engine.sync(s.cuda_stream)
        eager = out.clone()
        out.zero_()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            engine.pbs_many_batch_dev(lut, ct, out, count, 4, idx, s.cuda_stream)
        # a larger eager batch on the stream afterwards grows its sample buffer: the graph's one must stay alive
        big = torch.from_numpy(random_words(rng, (2 * count, p.n + 1)).view(np.int32)).cuda()
        big_out = torch.zeros((2 * count, 8, p.n + 1), dtype=torch.int32, device="cuda")
        engine.pbs_many_batch_dev(lut, big, big_out, 2 * count, 8, None, s.cuda_stream)
        engine.sync(s.cuda_stream)
        for _ in range(2):
            out.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, eager)
        engine.sync(s.cuda_stream)


def test_exact_backends_refuse_and_mirror_recovers(engine):
    import rustfhe_amd as R
    p = engine.p
    rng = np.random.default_rng(22)
    ct = random_words(rng, (37, p.n + 1))
    with engine.lut(random_words(rng, (1, p.N))) as lut:
        ref = engine.pbs_many_batch(lut, ct, 2)
        try:
            for b in (R._ffi.BACKEND_NTT_EXACT, R._ffi.BACKEND_FFT_SPLIT_EXACT):
                engine.set_backend(b)
                with pytest.raises(R.RtfheError) as ei:
                    engine.pbs_many_batch(lut, ct, 2)
                assert ei.value.code == R._ffi.ERR_INVALID and "mirror" in str(ei.value)
        finally:
            engine.set_backend(R._ffi.BACKEND_FFT64_MIRROR)
        assert np.array_equal(engine.pbs_many_batch(lut, ct, 2), ref)
        assert np.array_equal(engine.pbs_many_batch(lut, ct, 1)[:, 0], engine.pbs_batch(lut, ct))
