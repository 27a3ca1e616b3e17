"""GPU: TRLWE sample extraction (rtfhe_trlwe_extract_batch[_dev], rtfhe_trlwe_extract_lvl1_batch[_dev]; k_trlwe_extract).  Every word of both
forms against the oracle (orc.sample_extract, orc.key_switch) on TRLWEs of random words with planted edge words -- the arithmetic does not care
what a row encrypts --, cross-checks against the entry points that already extract (key_switch_batch, bootstrap_batch, cmux_tree_extract_batch),
both key-switch routes and every backend, meaning with real keys, capture and replay, refusals, bounds and launch counts.
Small TLWE dimensions as the tree's tests use: n = 40 at N = 1024, n = 24 at N = 2048."""
import types

import numpy as np
import pytest

import extract_helpers as X
import gpu_kit as gk
from gpu_kit import FILL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def worlds(orc):
    """per N, built on first use: keys from the product's keygen on an engine, the oracle's parameters, a memo of oracle words"""
    import rustfhe_amd as R

    def build(N):
        rp = R.Params(n=X.SMALL_N[N], N=N)
        key0, key1, bk, ksk = R.keygen(rp, 0xE7 + N)
        w = types.SimpleNamespace(R=R, N=N, rp=rp, key0=key0, key1=key1, bk=bk, ksk=ksk, P=orc.Params(n=rp.n, N=N), memo={})
        w.eng = gk.engine(R, rp, bk, ksk)
        return w
    made = gk.Worlds(build, close=lambda w: w.eng.close())
    yield made
    made.close()


def _case(orc, w, count, P, coef, stride=1, seed=0):
    """(x u32[count][2][N], the coefficients, the oracle's lvl1 and lvl0 words) of a shape: computed once per world, shared, read-only"""
    def compute():
        coefs = X.coefficients(w.N, P, coef, stride)
        x = X.trlwe_inputs(1000 * count + 10 * P + seed, w.N, count, coefs)
        return (x, coefs) + X.oracle_words(orc, w.P, w.ksk, x, coefs)
    return gk.memo(w.memo, (count, P, coef, stride, seed), compute)


def _dev(eng, x, P, coef, stride, lvl1, stream=None):
    """the _dev form into a 0x5A-filled buffer with CANARY words behind it, which are checked here; u32[count][P][words]"""
    import torch
    count, N = x.shape[0], x.shape[2]
    words = (N if lvl1 else eng.p.n) + 1
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream
    d_out = gk.guarded_out(count * P * words)
    (eng.trlwe_extract_lvl1_batch_dev if lvl1 else eng.trlwe_extract_batch_dev)(gk.to_device(x, np.uint32), P, d_out, count, coef, stride, st)
    eng.sync(st)
    return gk.read_guarded(d_out, count * P * words).reshape(count, P, words)


def _shapes():
    out = []
    for N in (1024, 2048):
        out += [(N, 1, 1, [0], 1), (N, 1, 1, [N - 1], 1), (N, 3, 5, [0, 1, N // 2, N - 2, N - 1], 1), (N, 2, 2, [5, 5], 1),
                (N, 1, 16, None, N // 16),         # exactly one tile
                (N, 1, 17, None, 1),               # one sample into a second tile
                (N, 37, 3, [1, N // 2, N - 1], 1),  # 111 samples: g changes inside tiles, the last tile is ragged
                (N, 2, 513, None, 1)]              # the 512-coefficient argument chunk; 1,026 samples pass the buffer's 1,024-sample minimum
    return out + [(1024, 1, 1024, None, 1)]        # a whole row


def _id(v):
    return "coef" if isinstance(v, list) else ("NULL" if v is None else str(v))


@pytest.mark.parametrize("N,count,P,coef,stride", _shapes(), ids=_id)
def test_every_word_equals_the_oracle(orc, worlds, N, count, P, coef, stride):
    """host and _dev forms, lvl1 and lvl0"""
    w = worlds(N)
    x, _, lvl1, lvl0 = _case(orc, w, count, P, coef, stride)
    got1 = w.eng.trlwe_extract_lvl1_batch(x, P, coef, stride)
    assert got1.shape == (count, P, N + 1) and got1.dtype == np.uint32
    bad = np.argwhere(got1 != lvl1)
    assert bad.size == 0, (len(bad), bad[:5])
    got0 = w.eng.trlwe_extract_batch(x, P, coef, stride)
    assert got0.shape == (count, P, w.rp.n + 1)
    bad = np.argwhere(got0 != lvl0)
    assert bad.size == 0, (len(bad), bad[:5])
    assert np.array_equal(_dev(w.eng, x, P, coef, stride, True), lvl1)
    assert np.array_equal(_dev(w.eng, x, P, coef, stride, False), lvl0)


@pytest.mark.parametrize("N", [1024, 2048])
def test_key_switch_of_the_lvl1_form_is_the_lvl0_form(orc, worlds, N):
    w = worlds(N)
    x, _, _, _ = _case(orc, w, 3, 5, [0, 1, N // 2, N - 2, N - 1])
    lvl1 = w.eng.trlwe_extract_lvl1_batch(x, 5, [0, 1, N // 2, N - 2, N - 1])
    assert np.array_equal(w.eng.key_switch_batch(lvl1).reshape(3, 5, -1), w.eng.trlwe_extract_batch(x, 5, [0, 1, N // 2, N - 2, N - 1]))


@pytest.mark.parametrize("N", [1024, 2048])
def test_blind_rotation_then_extraction_is_the_bootstrap(worlds, N):
    """no oracle: bootstrap_batch = key switch of sample extract 0 of the blind rotation"""
    w = worlds(N)
    tlwe = w.R.encrypt_bits(w.rp, w.key0, [0, 1, 1, 0, 1], 0xB007)
    acc = w.eng.blind_rotate_batch(tlwe)
    assert np.array_equal(w.eng.trlwe_extract_batch(acc, 1, [0])[:, 0], w.eng.bootstrap_batch(tlwe))


@pytest.mark.parametrize("N", [1024, 2048])
def test_tree_rows_then_extraction_is_the_tree_extract_form(worlds, N):
    """no oracle: cmux_tree_extract_batch(.., coef) = extraction at coef[g] of cmux_tree_batch's rows, one P-list with the diagonal picked"""
    w, R = worlds(N), worlds(N).R
    rng = np.random.default_rng(N + 41)
    depth, count = 2, 5
    bits = rng.integers(0, 2, 6).astype(np.uint8)
    table = R.encrypt_lut(w.rp, w.key1, rng.integers(0, 1 << 32, (6, N), dtype=np.uint64).astype(np.uint32), seed=0x7AB + N)
    sel_idx = rng.integers(0, 6, (count, depth)).astype(np.int32)
    row0 = rng.integers(0, 3, count).astype(np.int32)
    coef = np.array([0, 1, N // 2, N - 1, 1], np.int32)
    with w.eng.selectors(R.encrypt_selectors(w.rp, w.key1, bits, seed=0x5E1 + N)) as sel, w.eng.lut_encrypted(table) as lut:
        rows = w.eng.cmux_tree_batch(sel, lut, depth, count, sel_idx, row0)
        want = w.eng.cmux_tree_extract_batch(sel, lut, depth, count, sel_idx, row0, coef)
    got = w.eng.trlwe_extract_batch(rows, count, coef)
    assert np.array_equal(got[np.arange(count), np.arange(count)], want)


@pytest.mark.parametrize("N", [1024, 2048])
def test_other_key_switch_route_and_other_backends_give_the_same_words(orc, worlds, monkeypatch, N):
    w, R = worlds(N), worlds(N).R
    x, _, lvl1, lvl0 = _case(orc, w, 3, 5, [0, 1, N // 2, N - 2, N - 1])
    coef = [0, 1, N // 2, N - 2, N - 1]
    e = gk.engine(R, w.rp, w.bk, w.ksk, monkeypatch, {"RTFHE_KS_MM_MIN": "0"})      # no matrix key: k_key_switch_ext
    try:
        assert np.array_equal(e.trlwe_extract_batch(x, 5, coef), lvl0)
        assert np.array_equal(_dev(e, x, 5, coef, 1, False), lvl0)
        assert np.array_equal(e.trlwe_extract_lvl1_batch(x, 5, coef), lvl1)
    finally:
        e.close()
    for backend in (R._ffi.BACKEND_NTT_EXACT, R._ffi.BACKEND_FFT_SPLIT_EXACT):
        e = gk.engine(R, w.rp, w.bk, w.ksk)
        try:
            e.set_backend(backend)
            assert np.array_equal(e.trlwe_extract_batch(x, 5, coef), lvl0)
            assert np.array_equal(_dev(e, x, 5, coef, 1, True), lvl1)
        finally:
            e.close()


@pytest.mark.parametrize("N", [1024, 2048])
def test_meaning_encrypted_polynomial(orc, N):
    """Case A: an encrypted polynomial of 3-bit messages, read at [0, 1, N/2, N-1]; the seeds are checked on the oracle by
    tests/test_trlwe_extract_host.py, and the GPU's words are the oracle's"""
    import rustfhe_amd as R
    rp, key0, key1, ksk = X.meaning_keys(R, N)
    msgs, row, coef = X.meaning_case_a(R, N, rp, key1)
    e = R.Engine(rp, 0)
    try:
        e.load_ksk(ksk)
        got = e.trlwe_extract_batch(row, len(coef), coef)
    finally:
        e.close()
    assert np.array_equal(got, X.oracle_words(orc, orc.Params(n=rp.n, N=N), ksk, row, coef)[1])
    assert np.array_equal(R.decode_msgs(R.phases(rp, key0, got[0]), X.MEANING_BITS), msgs[coef])


def test_meaning_pack_then_extract(orc):
    """Case B: pack_batch(P = 8, rep = 1, pos = NULL), then extract(P = 8, NULL, 1), decodes to the packed messages -- every one"""
    import pack_oracle as O
    import rustfhe_amd as R
    N = 1024
    rp, key0, key1, ksk = X.meaning_keys(R, N)
    msgs, ct, pk = X.meaning_case_b(R, N, rp, key0, key1)
    e = R.Engine(rp, 0)
    try:
        e.load_ksk(ksk)
        with e.packing_key(pk) as key:
            packed = e.pack_batch(key, ct, X.MEANING_PACK_P, 1, None)
        got = e.trlwe_extract_batch(packed, X.MEANING_PACK_P, None, 1)
    finally:
        e.close()
    assert np.array_equal(packed, O.pack(rp, pk, ct, X.MEANING_PACK_P, None, 1))
    assert np.array_equal(got, X.oracle_words(orc, orc.Params(n=rp.n, N=N), ksk, packed, np.arange(X.MEANING_PACK_P))[1])
    assert np.array_equal(R.decode_msgs(R.phases(rp, key0, got[0]), X.MEANING_BITS), msgs)


def test_capture_and_replay(orc, worlds):
    import torch
    N = 1024
    w = worlds(N)
    R, e = w.R, w.eng
    count, P, coef = 3, 5, [0, 1, N // 2, N - 2, N - 1]
    a, _, a1, a0 = _case(orc, w, count, P, coef)
    b, _, b1, b0 = _case(orc, w, count, P, coef, seed=1)
    s = torch.cuda.Stream()
    d_in = gk.to_device(a, np.uint32)
    out0 = torch.zeros((count, P, w.rp.n + 1), dtype=torch.int32, device="cuda")
    out1 = torch.zeros((count, P, N + 1), dtype=torch.int32, device="cuda")
    host = lambda t: t.cpu().numpy().view(np.uint32)      # noqa: E731
    torch.cuda.synchronize()
    # a fresh stream, no eager call: the lvl0 form is refused (and the capture goes on), the lvl1 form allocates nothing and is captured
    refused = []
    with torch.cuda.stream(s):
        g1 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g1, stream=s):
            try:
                e.trlwe_extract_batch_dev(d_in, P, out0, count, coef, 1, s.cuda_stream)
            except R.RtfheError as err:
                refused.append(err)
            e.trlwe_extract_lvl1_batch_dev(d_in, P, out1, count, coef, 1, s.cuda_stream)
        assert len(refused) == 1 and refused[0].code == R._ffi.ERR_STATE and "capture" in str(refused[0]), refused
        for src, exp in ((a, a1), (b, b1)):
            d_in.copy_(gk.to_device(src, np.uint32))
            out1.zero_()
            g1.replay()
            torch.cuda.synchronize()
            assert np.array_equal(host(out1), exp)
        assert not host(out0).any()
        # an eager call on s, then the same call captured on s: replays on rewritten inputs give the oracle's words (coef is baked in)
        d_in.copy_(gk.to_device(a, np.uint32))
        e.trlwe_extract_batch_dev(d_in, P, out0, count, coef, 1, s.cuda_stream)
        e.sync(s.cuda_stream)
        assert np.array_equal(host(out0), a0)
        g0 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g0, stream=s):
            e.trlwe_extract_batch_dev(d_in, P, out0, count, coef, 1, s.cuda_stream)
        for src, exp in ((b, b0), (a, a0)):
            d_in.copy_(gk.to_device(src, np.uint32))
            out0.zero_()
            g0.replay()
            torch.cuda.synchronize()
            assert np.array_equal(host(out0), exp)
    e.sync(s.cuda_stream)


def test_refusals_leave_the_output_untouched(orc, worlds):
    import torch
    N = 1024
    w = worlds(N)
    R, e = w.R, w.eng
    x, _, lvl1, lvl0 = _case(orc, w, 3, 5, [0, 1, N // 2, N - 2, N - 1])
    d_in = gk.to_device(x, np.uint32)
    d_out = torch.full((3 * N * (N + 1) // 64,), FILL, dtype=torch.int32, device="cuda")      # room for every call below that could run
    d_both = torch.full((4, 2, N), FILL, dtype=torch.int32, device="cuda")                    # rows and output in one allocation
    i32 = lambda *v: np.array(v, np.int32)                                                    # noqa: E731
    e.timer_begin()
    for lvl1_form in (False, True):
        fn = e.L.rtfhe_trlwe_extract_lvl1_batch_dev if lvl1_form else e.L.rtfhe_trlwe_extract_batch_dev
        call = lambda P, coef, stride, count=3, src=d_in.data_ptr(), dst=d_out.data_ptr(): fn(      # noqa: E731
            e.h, src, P, None if coef is None else coef.ctypes.data, stride, dst, count, None)
        for args, word in (((0, None, 1), "P = 0"), ((N + 1, None, 1), "P = %d" % (N + 1)),
                           ((3, i32(0, -1, 5), 1), "sample 1: coef = -1"), ((3, i32(0, 1, N), 1), "sample 2: coef = %d" % N),
                           ((3, None, 0), "stride = 0"), ((3, None, -2), "stride = -2"),
                           ((3, None, N // 2), "sample 2: coef = %d" % N), ((N, None, 2), "sample %d: coef = %d" % (N // 2, N)),
                           ((1, i32(0), 1, 1 << 31), "count * P"), ((5, i32(0, 1, 2, 3, 4), 1, (1 << 31) // 5 + 1), "count * P"),
                           ((1, i32(0), 1, 3, 0), "null"), ((1, i32(0), 1, 3, d_in.data_ptr(), 0), "null"),
                           ((1, i32(0), 1, 2, d_both.data_ptr(), d_both[1].data_ptr()), "overlaps"),
                           ((1, i32(0), 1, 2, d_both[1].data_ptr(), d_both[1].data_ptr() - 64), "overlaps")):
            with pytest.raises(R.RtfheError) as ei:
                e._ck(call(*args))
            assert ei.value.code == R._ffi.ERR_INVALID and word in str(ei.value), (args[:3], str(ei.value))
        # host pointers where device pointers belong
        with pytest.raises(R.RtfheError) as ei:
            e._ck(call(1, i32(0), 1, 3, np.ascontiguousarray(x).ctypes.data))
        assert ei.value.code == R._ffi.ERR_INVALID and "device pointers" in str(ei.value)
        assert call(1, i32(0), 1, 0) == 0                           # count = 0
    assert e.timer_end()[1] == 0, "the checks come before any launch"
    e.sync()
    assert (d_out.cpu().numpy().view(np.uint32) == FILL).all() and (d_both.cpu().numpy().view(np.uint32) == FILL).all()
    assert w.eng.trlwe_extract_batch(x[:0], 5, [0, 1, 2, 3, 4]).shape == (0, 5, w.rp.n + 1)
    # d_out right behind the rows does not overlap them
    d_both[:2].copy_(gk.to_device(x[:2], np.uint32))
    e.trlwe_extract_lvl1_batch_dev(d_both[:2], 1, d_both[2], 2, [N - 1])
    e.sync()
    assert np.array_equal(d_both[2:].cpu().numpy().view(np.uint32).reshape(-1)[:2 * (N + 1)].reshape(2, 1, N + 1),
                          np.stack([X.extract_formula(x[g], N, N - 1) for g in range(2)])[:, None])
    # no key-switching key: the lvl0 form is a state error, the lvl1 form runs on a context with nothing loaded
    bare = R.Engine(w.rp, 0)
    try:
        with pytest.raises(R.RtfheError) as ei:
            bare.trlwe_extract_batch(x, 5, [0, 1, N // 2, N - 2, N - 1])
        assert ei.value.code == R._ffi.ERR_STATE and "key-switching key" in str(ei.value)
        d_keep = torch.full((3 * 5 * (w.rp.n + 1),), FILL, dtype=torch.int32, device="cuda")
        with pytest.raises(R.RtfheError) as ei:
            bare.trlwe_extract_batch_dev(d_in, 5, d_keep, 3, [0, 1, N // 2, N - 2, N - 1])
        assert ei.value.code == R._ffi.ERR_STATE
        bare.sync()
        assert (d_keep.cpu().numpy().view(np.uint32) == FILL).all()
        assert np.array_equal(bare.trlwe_extract_lvl1_batch(x, 5, [0, 1, N // 2, N - 2, N - 1]), lvl1)
        assert np.array_equal(_dev(bare, x, 5, [0, 1, N // 2, N - 2, N - 1], 1, True), lvl1)
    finally:
        bare.close()
    # a two-entry context: the call runs on the primary device and gives the same words
    multi = gk.engine(R, w.rp, w.bk, w.ksk, devices=[0, 0])
    try:
        assert multi.device_count() == 2
        assert np.array_equal(multi.trlwe_extract_batch(x, 5, [0, 1, N // 2, N - 2, N - 1]), lvl0)
        assert np.array_equal(_dev(multi, x, 5, [0, 1, N // 2, N - 2, N - 1], 1, False), lvl0)
        assert np.array_equal(_dev(multi, x, 5, [0, 1, N // 2, N - 2, N - 1], 1, True), lvl1)
    finally:
        multi.close()


@pytest.mark.parametrize("N", [1024, 2048])
def test_a_ragged_tile_writes_nothing_past_its_samples(orc, worlds, N):
    """111 samples = 6 tiles and 15 slots: the natural rows end exactly at sample 110 (canary words behind them keep their bytes), and a smaller
    call into the same buffer leaves the rows of the larger one beyond its own samples as they were"""
    import torch
    w = worlds(N)
    coef = [1, N // 2, N - 1]
    x, _, lvl1, lvl0 = _case(orc, w, 37, 3, coef)
    assert np.array_equal(_dev(w.eng, x, 3, coef, 1, True), lvl1) and np.array_equal(_dev(w.eng, x, 3, coef, 1, False), lvl0)
    st = torch.cuda.current_stream().cuda_stream
    d_out = torch.full((111 * (N + 1),), FILL, dtype=torch.int32, device="cuda")
    w.eng.trlwe_extract_lvl1_batch_dev(gk.to_device(x, np.uint32), 3, d_out, 6, coef, 1, st)        # 18 samples: one whole tile and 2 slots of the next
    w.eng.sync(st)
    out = d_out.cpu().numpy().view(np.uint32)
    assert np.array_equal(out[:18 * (N + 1)].reshape(6, 3, N + 1), lvl1[:6]) and (out[18 * (N + 1):] == FILL).all()


@pytest.mark.parametrize("route", ["matrix", "wave_per_sample"])
def test_launch_counts(orc, worlds, monkeypatch, route):
    """ceil(P / 512) extract launches plus one key-switch kernel; the lvl1 form has no key switch"""
    import torch
    N = 1024
    w = worlds(N)
    e = w.eng if route == "matrix" else gk.engine(w.R, w.rp, w.bk, w.ksk, monkeypatch, {"RTFHE_KS_MM_MIN": "0"})
    try:
        st = torch.cuda.current_stream().cuda_stream
        for count, P, coef, stride in ((1, 1, [N - 1], 1), (2, 513, None, 1)):
            x, _, lvl1, lvl0 = _case(orc, w, count, P, coef, stride)
            d_in = gk.to_device(x, np.uint32)
            for lvl1_form, want in ((False, lvl0), (True, lvl1)):
                d_out = torch.zeros(want.shape, dtype=torch.int32, device="cuda")
                e.timer_begin(st)
                (e.trlwe_extract_lvl1_batch_dev if lvl1_form else e.trlwe_extract_batch_dev)(d_in, P, d_out, count, coef, stride, st)
                launches = e.timer_end(st)[1]
                assert launches == -(-P // 512) + (0 if lvl1_form else 1), (route, P, lvl1_form, launches)
                assert np.array_equal(d_out.cpu().numpy().view(np.uint32), want)
    finally:
        if e is not w.eng:
            e.close()


def test_histogram_threshold_example(engine, keys):
    """examples/histogram_threshold.py at its default parameters on the session's engine and key set (no key generation of its own, so it
    takes what the other example tests take): the decrypted flags are the clear ones"""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("histogram_threshold", os.path.join(root, "examples", "histogram_threshold.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    want, got, hist = ex.run(engine, keys.key0, keys.key1, seed=0x7E5)
    assert hist.sum() == 12 and hist.max() <= 7 and 0 < want.sum() < 16, hist
    assert np.array_equal(got, want), (hist, got, want)
