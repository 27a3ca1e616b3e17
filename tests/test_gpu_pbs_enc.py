"""GPU: programmable bootstrapping from encrypted tables (rtfhe_lut_create_encrypted; the k_pbs_enc_* kernels of every FP64-mirror kernel
family).  A trivial encryption (tv, 0) gives the plain table's words through every PBS entry in every batch shape; a real encryption gives the
oracle's words (tests/pbs_oracle.py: oracle_pbs_enc); encoded functions decrypt; index checks, sharding, graph capture, LUT circuits,
backend refusal and lifetimes follow the plain table's rules."""
import importlib.util
import os

import numpy as np
import pytest

import gpu_kit as gk
from kit import keys_2048, random_words
from lut_circuit_kit import adder_inputs, decode
from pbs_oracle import oracle_pbs_enc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = (1, 37, 1024, 1280)


@pytest.fixture(scope="module")
def keys2048(orc):
    return keys_2048(orc)


def _trivial(tv):
    """(tv, 0) rows: u32[n][2][N]"""
    tv = np.asarray(tv, np.uint32)
    return np.stack([tv, np.zeros_like(tv)], axis=1)


def _check_trivial(e, N, n1, counts, seed):
    """A trivially encrypted table against the plain one on the same engine: pbs_batch and pbs_many_batch with every n_out."""
    rng = np.random.default_rng(seed)
    tv = random_words(rng, (3, N))
    with e.lut(tv) as plain, e.lut_encrypted(_trivial(tv)) as enc:
        assert enc.encrypted and not plain.encrypted and enc.n_lut == 3
        for count in counts:
            ct = random_words(rng, (count, n1))
            idx = rng.integers(0, 3, count).astype(np.int32)
            assert np.array_equal(e.pbs_batch(enc, ct, idx), e.pbs_batch(plain, ct, idx)), count
            for n_out in (1, 2, 4, 8):
                assert np.array_equal(e.pbs_many_batch(enc, ct, n_out, idx), e.pbs_many_batch(plain, ct, n_out, idx)), (count, n_out)


@pytest.mark.parametrize("env", gk.CONFIGS_1024, ids=gk.env_id)
def test_trivial_encryption_is_the_plain_table_every_shape_n1024(params, keys, engine, monkeypatch, env):
    import rustfhe_amd as R
    p = R.Params(n=params.n, N=params.N)
    e = gk.engine(R, p, keys.bk_t, keys.ksk, monkeypatch, env) if env else engine
    try:
        _check_trivial(e, p.N, p.n + 1, COUNTS, 4097)
    finally:
        if e is not engine:
            e.close()


@pytest.mark.parametrize("env", gk.CONFIGS_2048, ids=gk.env_id)
def test_trivial_encryption_is_the_plain_table_every_shape_n2048(keys2048, monkeypatch, env):
    import rustfhe_amd as R
    P, K = keys2048
    e = gk.engine(R, R.Params(N=2048), K.bk_t, K.ksk, monkeypatch, env)
    try:
        _check_trivial(e, P.N, P.n + 1, COUNTS, 8193)
    finally:
        e.close()


def _check_oracle(orc, P, plan, bk_f, ksk, key1, e, count, seed):
    import rustfhe_amd as R
    rng = np.random.default_rng(seed)
    rp = R.Params(n=P.n, N=P.N)
    table = R.encrypt_lut(rp, key1, random_words(rng, (3, P.N)), seed=seed)
    idx = rng.integers(0, 3, count).astype(np.int32)
    ct = random_words(rng, (count, P.n + 1))
    with e.lut_encrypted(table) as lut:
        for n_out in (1, 2, 4, 8):
            out = e.pbs_many_batch(lut, ct, n_out, idx)
            if n_out == 1:
                assert np.array_equal(e.pbs_batch(lut, ct, idx), out[:, 0])
            for g in sorted({0, count - 1, int(rng.integers(0, count))}):
                assert np.array_equal(out[g], oracle_pbs_enc(orc, P, plan, bk_f, ksk, table[idx[g]], ct[g], n_out)), (g, n_out)


def test_real_encryption_against_the_oracle_n1024(orc, params, keys, engine):
    _check_oracle(orc, params, orc.Plan(params.N), keys.bk_f, keys.ksk, keys.key1, engine, 37, 51)


def test_real_encryption_against_the_oracle_n2048(orc, keys2048):
    import rustfhe_amd as R
    P, K = keys2048
    e = gk.engine(R, R.Params(N=2048), K.bk_t, K.ksk)
    try:
        _check_oracle(orc, P, orc.Plan(P.N), K.bk_f, K.ksk, K.key1, e, 37, 52)
    finally:
        e.close()


def _decode_all(R, p, key0, out, bits):
    return R.decode_msgs(R.phases(p, key0, out.reshape(-1, p.n + 1)), bits).reshape(out.shape[:-1])


@pytest.mark.parametrize("fs,chained_wrong", [
    ([lambda m: m & 1, lambda m: m >> 1], 0),
    ([lambda m: m, lambda m: (m * m) % 4, lambda m: (m + 1) % 4, lambda m: 3 - m], 16),
], ids=["two", "four"])
def test_encrypted_functions_decrypt_and_chain(engine, keys, fs, chained_wrong):
    """4,096 fresh 2-bit messages: every output of one PBS from an encrypted table decodes to f_j(m), and the outputs of a second one on ALL of
    those outputs decode to f_k(f_j(m)) -- every one at n_out = 2; at n_out = 4 at most `chained_wrong` of the 65,536, as with the plain table:
    its coarser mod switch leaves about 4 sigma for a bootstrapped input, and a second rotation that lands one box off spoils its 4 outputs
    (0-12 wrong for plain tables, 0-8 for their encryptions, same inputs)."""
    import rustfhe_amd as R
    p = engine.p
    th = len(fs)
    msgs = np.arange(4096) % 4
    ct = R.encrypt_torus(p, keys.key0, R.encode_msgs(msgs, 2), seed=0x5A00 + th)
    table = R.encrypt_lut(p, keys.key1, R.many_lut_polynomial(fs, p.N, 2), seed=0x5B00 + th)
    with engine.lut_encrypted(table) as lut:
        once = engine.pbs_many_batch(lut, ct, th)
        twice = engine.pbs_many_batch(lut, once.reshape(-1, p.n + 1), th).reshape(len(msgs), th, th, p.n + 1)
    assert np.array_equal(_decode_all(R, p, keys.key0, once, 2), np.array([[f(m) for f in fs] for m in msgs]))
    wrong = _decode_all(R, p, keys.key0, twice, 2) != np.array([[[g(f(m)) for g in fs] for f in fs] for m in msgs])
    assert int(wrong.sum()) <= chained_wrong, int(wrong.sum())


def test_bad_indices_host_and_device(engine, keys):
    import torch
    import rustfhe_amd as R
    p = engine.p
    rng = np.random.default_rng(18)
    count = 300
    ct = random_words(rng, (count, p.n + 1))
    idx = rng.integers(0, 2, count).astype(np.int32)
    with engine.lut_encrypted(R.encrypt_lut(p, keys.key1, random_words(rng, (2, p.N)), seed=18)) as lut:
        ref1 = engine.pbs_batch(lut, ct, idx)
        ref2 = engine.pbs_many_batch(lut, ct, 2, idx)
        bad = idx.copy()
        bad[5] = 2
        engine.timer_begin()
        for call in (lambda: engine.pbs_batch(lut, ct, bad), lambda: engine.pbs_many_batch(lut, ct, 2, bad)):
            with pytest.raises(R.RtfheError) as ei:
                call()
            assert ei.value.code == R._ffi.ERR_INVALID and "lut_idx[5]" in str(ei.value)
        assert engine.timer_end()[1] == 0, "the host entries check before they launch anything"
        bad[7] = -1
        d_ct = torch.from_numpy(ct.view(np.int32)).cuda()
        d_bad = torch.from_numpy(bad).cuda()
        keep = np.ones(count, bool)
        keep[[5, 7]] = False
        st = torch.cuda.current_stream().cuda_stream
        d_out = torch.zeros((count, p.n + 1), dtype=torch.int32, device="cuda")
        engine.pbs_batch_dev(lut, d_ct, d_out, count, d_bad, st)
        with pytest.raises(R.RtfheError) as ei:
            engine.sync(st)
        assert ei.value.code == R._ffi.ERR_INVALID
        assert np.array_equal(d_out.cpu().numpy().view(np.uint32)[keep], ref1[keep])
        d_out2 = torch.zeros((count, 2, p.n + 1), dtype=torch.int32, device="cuda")
        engine.pbs_many_batch_dev(lut, d_ct, d_out2, count, 2, d_bad, st)
        with pytest.raises(R.RtfheError) as ei:
            engine.sync(st)
        assert ei.value.code == R._ffi.ERR_INVALID
        assert np.array_equal(d_out2.cpu().numpy().view(np.uint32)[keep], ref2[keep])
        engine.sync(st)                                      # reported once
        engine.pbs_batch_dev(lut, d_ct, d_out, count, torch.from_numpy(idx).cuda(), st)
        engine.sync(st)
        assert np.array_equal(d_out.cpu().numpy().view(np.uint32), ref1)


def test_multi_entry_context_matches_single(params, keys, engine):
    import torch
    import rustfhe_amd as R
    p = engine.p
    rng = np.random.default_rng(19)
    G = 4099
    table = R.encrypt_lut(p, keys.key1, random_words(rng, (4, p.N)), seed=19)
    ct = random_words(rng, (G, p.n + 1))
    idx = rng.integers(0, 4, G).astype(np.int32)
    with engine.lut_encrypted(table) as lut:
        ref1 = engine.pbs_batch(lut, ct, idx)
        ref4 = engine.pbs_many_batch(lut, ct, 4, idx)
    multi = gk.engine(R, p, keys.bk_t, keys.ksk, devices=[0, 0])
    try:
        with multi.lut_encrypted(table) as lut:
            assert np.array_equal(multi.pbs_batch(lut, ct, idx), ref1)
            assert np.array_equal(multi.pbs_many_batch(lut, ct, 4, idx), ref4)
            d_ct = torch.from_numpy(ct.view(np.int32)).cuda()
            d_idx = torch.from_numpy(idx).cuda()
            st = torch.cuda.current_stream().cuda_stream
            d_out = torch.zeros((G, p.n + 1), dtype=torch.int32, device="cuda")
            multi.pbs_batch_dev(lut, d_ct, d_out, G, d_idx, st)
            d_out4 = torch.zeros((G, 4, p.n + 1), dtype=torch.int32, device="cuda")
            multi.pbs_many_batch_dev(lut, d_ct, d_out4, G, 4, d_idx, st)
            multi.sync(st)
            assert np.array_equal(d_out.cpu().numpy().view(np.uint32), ref1)
            assert np.array_equal(d_out4.cpu().numpy().view(np.uint32), ref4)
    finally:
        multi.close()


def test_graph_capture_replays_eager_words(engine, keys):
    import torch
    import rustfhe_amd as R
    p = engine.p
    rng = np.random.default_rng(20)
    count = 600
    table = R.encrypt_lut(p, keys.key1, random_words(rng, (3, p.N)), seed=20)
    ct = torch.from_numpy(random_words(rng, (count, p.n + 1)).view(np.int32)).cuda()
    idx = torch.from_numpy(rng.integers(0, 3, count).astype(np.int32)).cuda()
    s = torch.cuda.Stream()
    out = torch.zeros((count, 4, p.n + 1), dtype=torch.int32, device="cuda")
    out1 = torch.zeros((count, p.n + 1), dtype=torch.int32, device="cuda")
    with engine.lut_encrypted(table) as lut, torch.cuda.stream(s):
        engine.pbs_many_batch_dev(lut, ct, out, count, 4, idx, s.cuda_stream)      # the eager calls the capture rule asks for
        engine.pbs_batch_dev(lut, ct, out1, count, idx, s.cuda_stream)
        engine.sync(s.cuda_stream)
        eager, eager1 = out.clone(), out1.clone()
        out.zero_()
        out1.zero_()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            engine.pbs_many_batch_dev(lut, ct, out, count, 4, idx, s.cuda_stream)
            engine.pbs_batch_dev(lut, ct, out1, count, idx, s.cuda_stream)
        for _ in range(2):
            out.zero_()
            out1.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, eager) and torch.equal(out1, eager1)
        engine.sync(s.cuda_stream)


def test_lut_circuit_adder_with_encrypted_tables(engine, keys):
    """lut_ripple_adder at 1,024 replicas: with its tables encrypted every sum decrypts right; with them trivially encrypted the wire table
    equals the plain-table circuit's word for word."""
    import rustfhe_amd as R
    p = engine.p
    reps = 1024
    net = R.lut_ripple_adder(8)
    a, b, cts = adder_inputs(R, p, keys.key0, reps, 0xE1C)
    plain = R.LutCircuitRunner(engine, net, reps)
    enc = R.LutCircuitRunner(engine, net, reps, key1=keys.key1, seed=0xE1D)
    triv = R.LutCircuitRunner(engine, net, reps)
    try:
        for run in (plain, enc, triv):
            run.set_inputs(cts)
        d = triv.desc
        with engine.lut_encrypted(_trivial(net.polynomials(p.N))) as lut:
            triv._circuit = engine.lut_circuit_create(lut, d["fan_in"], d["in_idx"], d["weights"], d["cst"], d["lut_idx"], d["wave_offsets"],
                                                      d["wave_n_out"], d["out_idx"], triv.wires, d["num_wires"])
        for run in (plain, enc, triv):
            run.run()
        assert np.array_equal(decode(R, p, keys.key0, enc.outputs()), a + b)
        assert np.array_equal(triv.wires.cpu().numpy(), plain.wires.cpu().numpy())
        assert np.array_equal(decode(R, p, keys.key0, plain.outputs()), a + b)
    finally:
        for run in (plain, enc, triv):
            run.close()


def test_exact_backends_refuse_and_mirror_recovers(engine, keys):
    import rustfhe_amd as R
    p = engine.p
    rng = np.random.default_rng(22)
    ct = random_words(rng, (37, p.n + 1))
    with engine.lut_encrypted(R.encrypt_lut(p, keys.key1, random_words(rng, (1, p.N)), seed=22)) as lut:
        ref = engine.pbs_many_batch(lut, ct, 2)
        try:
            for b in (R._ffi.BACKEND_NTT_EXACT, R._ffi.BACKEND_FFT_SPLIT_EXACT):
                engine.set_backend(b)
                for call in (lambda: engine.pbs_many_batch(lut, ct, 2), lambda: engine.pbs_batch(lut, ct)):
                    with pytest.raises(R.RtfheError) as ei:
                        call()
                    assert ei.value.code == R._ffi.ERR_INVALID and "mirror" in str(ei.value)
        finally:
            engine.set_backend(R._ffi.BACKEND_FFT64_MIRROR)
        assert np.array_equal(engine.pbs_many_batch(lut, ct, 2), ref)
        assert np.array_equal(engine.pbs_many_batch(lut, ct, 1)[:, 0], engine.pbs_batch(lut, ct))


def test_lifetimes(params, keys):
    import rustfhe_amd as R
    p = R.Params(n=params.n, N=params.N)
    rng = np.random.default_rng(24)
    table = R.encrypt_lut(p, keys.key1, random_words(rng, (2, p.N)), seed=24)
    ct = random_words(rng, (37, p.n + 1))
    e = gk.engine(R, p, keys.bk_t, keys.ksk)
    other = gk.engine(R, p, keys.bk_t, keys.ksk)
    try:
        first = e.lut_encrypted(table)
        ref = e.pbs_many_batch(first, ct, 2)
        first.close()                                              # the table destroyed first: the context goes on
        with e.lut_encrypted(table) as again:
            assert np.array_equal(e.pbs_many_batch(again, ct, 2), ref)
            with pytest.raises(R.RtfheError) as ei:
                other.pbs_batch(again, ct)                         # a table of another context
            assert ei.value.code == R._ffi.ERR_INVALID and "another context" in str(ei.value)
        late = other.lut_encrypted(table)
    finally:
        e.close()
        other.close()
    with pytest.raises(R.RtfheError) as ei:
        other.pbs_many_batch(late, ct, 2)                          # the context destroyed first
    late.close()                                                   # only frees the handle


def test_private_lut_example(engine, keys):
    spec = importlib.util.spec_from_file_location("private_lut", os.path.join(ROOT, "examples", "private_lut.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    x, got, want = ex.run(engine, keys.key0, keys.key1, 1024, seed=0x9E)
    assert len(x) == 1024 and np.array_equal(got, want)
