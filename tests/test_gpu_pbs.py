"""GPU: programmable bootstrapping (rtfhe_lut_create / rtfhe_pbs_batch[_dev], the k_pbs_* twins of every FP64-mirror kernel family).
With the constant 1/8 table a PBS is the gate path's bootstrap, word for word, in every batch shape the dispatch takes; with random tables it is
the oracle's PBS (tests/pbs_oracle.py: oracle_pbs) word for word; with encoded functions it decrypts to them."""
import numpy as np
import pytest

import gpu_kit as gk
from kit import keys_2048, phase_err, random_words
from pbs_oracle import oracle_pbs

pytestmark = pytest.mark.gpu

EIGHTH = 0x20000000


@pytest.mark.parametrize("env", gk.CONFIGS_1024, ids=gk.env_id)
def test_constant_table_equals_bootstrap_every_shape_n1024(params, keys, monkeypatch, env):
    import rustfhe_amd as R
    p = R.Params(n=params.n, N=params.N)
    e = gk.engine(R, p, keys.bk_t, keys.ksk, monkeypatch, env)
    rng = np.random.default_rng(1024)
    try:
        with e.lut(np.full((2, p.N), EIGHTH, np.uint32)) as lut:       # two identical rows: random indices exercise the index path too
            for count in (1, 37, 300, 600, 900, 1024, 1280, 2048):
                ct = random_words(rng, (count, p.n + 1))
                ref = e.bootstrap_batch(ct)
                assert np.array_equal(e.pbs_batch(lut, ct), ref), count
                assert np.array_equal(e.pbs_batch(lut, ct, rng.integers(0, 2, count)), ref), count
    finally:
        e.close()


@pytest.fixture(scope="module")
def keys2048(orc):
    return keys_2048(orc)


@pytest.mark.parametrize("env", gk.CONFIGS_2048, ids=gk.env_id)
def test_constant_table_equals_bootstrap_every_shape_n2048(keys2048, monkeypatch, env):
    import rustfhe_amd as R
    P, K = keys2048
    e = gk.engine(R, R.Params(N=2048), K.bk_t, K.ksk, monkeypatch, env)
    rng = np.random.default_rng(2048)
    try:
        with e.lut(np.full(P.N, EIGHTH, np.uint32)) as lut:
            for count in (1, 37, 300, 600, 1024, 1100):
                ct = random_words(rng, (count, P.n + 1))
                assert np.array_equal(e.pbs_batch(lut, ct), e.bootstrap_batch(ct)), count
    finally:
        e.close()


def _check_random_tables(orc, P, plan, bk_f, ksk, e, count, seed):
    rng = np.random.default_rng(seed)
    tv = random_words(rng, (3, P.N))
    idx = rng.integers(0, 3, count).astype(np.int32)
    ct = random_words(rng, (count, P.n + 1))
    with e.lut(tv) as lut:
        out = e.pbs_batch(lut, ct, idx)
    pick = sorted(set([0, count - 1]) | set(rng.choice(count, min(count, 16), replace=False).tolist()))
    for g in pick:
        assert np.array_equal(out[g], oracle_pbs(orc, P, plan, bk_f, ksk, tv[idx[g]], ct[g])), g


def test_random_tables_against_the_oracle_n1024(orc, params, keys, engine):
    plan = orc.Plan(params.N)
    for count, seed in ((1280, 11), (37, 12)):
        _check_random_tables(orc, params, plan, keys.bk_f, keys.ksk, engine, count, seed)


def test_random_tables_against_the_oracle_n2048(orc, keys2048):
    import rustfhe_amd as R
    P, K = keys2048
    e = gk.engine(R, R.Params(N=2048), K.bk_t, K.ksk)
    try:
        _check_random_tables(orc, P, orc.Plan(P.N), K.bk_f, K.ksk, e, 600, 13)
    finally:
        e.close()


@pytest.mark.parametrize("fname", ["identity", "square", "succ", "msb"])
def test_encoded_functions_decrypt_through_two_pbs_2bit(engine, keys, fname):
    """p = 2: 1,024 fresh ciphertexts (every message 256 times), one PBS, then a second PBS on its outputs: every word decrypts to f, then f(f)."""
    import rustfhe_amd as R
    from pbs_oracle import FUNCS
    P = 2
    f = lambda m: FUNCS[fname](m, P)  # noqa: E731
    p = engine.p
    msgs = np.arange(1024) % (1 << P)
    ct = R.encrypt_torus(p, keys.key0, R.encode_msgs(msgs, P), seed=0x3B17 + len(fname))
    with engine.lut(R.lut_polynomial(f, p.N, P)) as lut:
        once = engine.pbs_batch(lut, ct)
        twice = engine.pbs_batch(lut, once)
    fm = np.array([f(m) for m in msgs])
    assert np.array_equal(R.decode_msgs(R.phases(p, keys.key0, once), P), fm)
    assert np.array_equal(R.decode_msgs(R.phases(p, keys.key0, twice), P), [f(m) for m in fm])


@pytest.mark.parametrize("fname", ["identity", "square", "succ", "msb"])
def test_encoded_functions_3bit(engine, keys, fname):
    """p = 3 at n = 635, N = 1024: the INPUT side has room (a mod-switch error of a few units against a half box of 64 units of 1/2N), every
    table lookup is right -- but a bootstrapped ciphertext carries the key switch's and the key's noise, which at these parameters is a
    sizeable fraction of a 3-bit box's half width (1/32 of the torus).  Checked: the error of every output is what that noise
    gives (never a wrong box by more than one, the typical error far inside the box), a 1-bit output of a 3-bit input (m >= 4) decrypts
    always, and the outputs of a first PBS chained into a second land in the right box in the large majority."""
    import rustfhe_amd as R
    from pbs_oracle import FUNCS
    P = 3
    f = lambda m: FUNCS[fname](m, P)  # noqa: E731
    p = engine.p
    msgs = np.arange(1024) % (1 << P)
    ct = R.encrypt_torus(p, keys.key0, R.encode_msgs(msgs, P), seed=0x3B30 + len(fname))
    fm = np.array([f(m) for m in msgs])
    with engine.lut(R.lut_polynomial(f, p.N, P)) as lut:
        once = engine.pbs_batch(lut, ct)
        twice = engine.pbs_batch(lut, once)
    e1 = phase_err(R, p, keys.key0, once, fm, P)
    assert np.abs(e1).max() < 1.5 / 16 and np.median(np.abs(e1)) < 1.0 / 64, (np.abs(e1).max(), np.median(np.abs(e1)))
    assert np.mean(R.decode_msgs(R.phases(p, keys.key0, once), P) == fm) >= 0.9
    assert np.mean(R.decode_msgs(R.phases(p, keys.key0, twice), P) == [f(m) for m in fm]) >= 0.85
    with engine.lut(R.lut_polynomial(lambda m: int(m >= 4), p.N, P, out_bits=1)) as lut:
        top = engine.pbs_batch(lut, ct)
    assert np.array_equal(R.decode_msgs(R.phases(p, keys.key0, top), 1), (msgs >= 4).astype(int))


def test_bad_indices_host_and_device(engine, keys):
    import torch
    import rustfhe_amd as R
    p = engine.p
    rng = np.random.default_rng(8)
    count = 300
    tv = random_words(rng, (2, p.N))
    ct = random_words(rng, (count, p.n + 1))
    idx = rng.integers(0, 2, count).astype(np.int32)
    with engine.lut(tv) as lut:
        ref = engine.pbs_batch(lut, ct, idx)
        bad = idx.copy()
        bad[5] = 2
        engine.timer_begin()
        with pytest.raises(R.RtfheError) as ei:
            engine.pbs_batch(lut, ct, bad)
        assert ei.value.code == R._ffi.ERR_INVALID and "lut_idx[5]" in str(ei.value)
        assert engine.timer_end()[1] == 0, "the host entry checks before it launches anything"
        bad[7] = -1
        d_ct = torch.from_numpy(ct.view(np.int32)).cuda()
        d_out = torch.zeros_like(d_ct)
        d_bad = torch.from_numpy(bad).cuda()
        st = torch.cuda.current_stream().cuda_stream
        engine.pbs_batch_dev(lut, d_ct, d_out, count, d_bad, st)
        with pytest.raises(R.RtfheError) as ei:
            engine.sync(st)
        assert ei.value.code == R._ffi.ERR_INVALID
        out = d_out.cpu().numpy().view(np.uint32)
        keep = np.ones(count, bool)
        keep[[5, 7]] = False
        assert np.array_equal(out[keep], ref[keep])
        engine.sync(st)                                      # reported once
        d_idx = torch.from_numpy(idx).cuda()
        engine.pbs_batch_dev(lut, d_ct, d_out, count, d_idx, st)
        engine.sync(st)
        assert np.array_equal(d_out.cpu().numpy().view(np.uint32), ref)


def test_multi_entry_context_matches_single(params, keys, engine):
    import torch
    import rustfhe_amd as R
    p = engine.p
    rng = np.random.default_rng(9)
    G = 8192
    tv = random_words(rng, (4, p.N))
    ct = random_words(rng, (G, p.n + 1))
    idx = rng.integers(0, 4, G).astype(np.int32)
    with engine.lut(tv) as lut:
        ref = engine.pbs_batch(lut, ct, idx)
    multi = gk.engine(R, p, keys.bk_t, keys.ksk, devices=[0, 0])
    try:
        with multi.lut(tv) as lut:
            assert np.array_equal(multi.pbs_batch(lut, ct, idx), ref)
            d_ct = torch.from_numpy(ct.view(np.int32)).cuda()
            d_out = torch.zeros_like(d_ct)
            d_idx = torch.from_numpy(idx).cuda()
            st = torch.cuda.current_stream().cuda_stream
            multi.pbs_batch_dev(lut, d_ct, d_out, G, d_idx, st)
            multi.sync(st)
            assert np.array_equal(d_out.cpu().numpy().view(np.uint32), ref)
    finally:
        multi.close()


def test_graph_capture_replays_eager_words(engine):
    import torch
    p = engine.p
    rng = np.random.default_rng(10)
    count = 600
    tv = random_words(rng, (3, p.N))
    ct = torch.from_numpy(random_words(rng, (count, p.n + 1)).view(np.int32)).cuda()
    idx = torch.from_numpy(rng.integers(0, 3, count).astype(np.int32)).cuda()
    s = torch.cuda.Stream()
    out = torch.zeros_like(ct)
    with engine.lut(tv) as lut, torch.cuda.stream(s):
        engine.pbs_batch_dev(lut, ct, out, count, idx, s.cuda_stream)
        engine.sync(s.cuda_stream)
        eager = out.clone()
        out.zero_()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            engine.pbs_batch_dev(lut, ct, out, count, idx, s.cuda_stream)
        for _ in range(2):
            out.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, eager)
        engine.sync(s.cuda_stream)


def test_exact_backends_refuse_and_mirror_recovers(engine):
    import rustfhe_amd as R
    p = engine.p
    rng = np.random.default_rng(12)
    ct = random_words(rng, (37, p.n + 1))
    with engine.lut(np.full(p.N, EIGHTH, np.uint32)) as lut:
        ref = engine.pbs_batch(lut, ct)
        try:
            for b in (R._ffi.BACKEND_NTT_EXACT, R._ffi.BACKEND_FFT_SPLIT_EXACT):
                engine.set_backend(b)
                with pytest.raises(R.RtfheError) as ei:
                    engine.pbs_batch(lut, ct)
                assert ei.value.code == R._ffi.ERR_INVALID and "mirror" in str(ei.value)
        finally:
            engine.set_backend(R._ffi.BACKEND_FFT64_MIRROR)
        assert np.array_equal(engine.pbs_batch(lut, ct), ref)
        assert np.array_equal(ref, engine.bootstrap_batch(ct))


def test_lut_outliving_its_context(params, keys):
    import rustfhe_amd as R
    e = gk.engine(R, R.Params(), keys.bk_t, keys.ksk)
    lut = e.lut(np.full(e.p.N, EIGHTH, np.uint32))
    e.close()
    lut.close()                                               # only frees the handle
