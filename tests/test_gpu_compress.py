"""GPU: compressed results (rtfhe_tlwe_compress_batch_dev, rtfhe_trlwe_compress_batch_dev; k_compress_rows).  Every output word of both forms
against the numpy restatement of the specification (tests/compress_oracle.py) AND against the CPU twin, on rows of random words with planted
edge words -- the arithmetic does not care what a row encrypts --, into 0x5A-filled outputs with canary words behind them; one end-to-end
case with real keys (PBS -> pack -> compress on one stream, host expand, decode; the same captured and replayed); the other backends, a
two-entry context, and the refusals."""
import types

import numpy as np
import pytest

import compress_oracle as O
import gpu_kit as gk
from gpu_kit import FILL
from kit import SMALL_N

pytestmark = pytest.mark.gpu

KS = [2, 5, 12, 16, 31, 32]


@pytest.fixture(scope="module")
def worlds():
    """one engine per (N, n) with NO key loaded -- the calls need none --, built on first use"""
    import rustfhe_amd as R

    def build(N, n):
        w = types.SimpleNamespace(R=R, N=N, rp=R.Params(n=n, N=N))
        w.eng = R.Engine(w.rp, 0)
        return w
    made = gk.Worlds(build, close=lambda w: w.eng.close())
    yield made
    made.close()


def _tlwe_dev(eng, x, k, stream=None):
    """the lvl0 _dev form into a guarded buffer; u32[count][W]"""
    import torch
    count, W = x.shape[0], O.words(x.shape[1], k)
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream
    d_out = gk.guarded_out(count * W)
    eng.tlwe_compress_dev(gk.to_device(x, np.uint32), k, d_out, count, st)
    eng.sync(st)
    return gk.read_guarded(d_out, count * W).reshape(count, W)


def _trlwe_dev(eng, x, k, P, coef, stride, stream=None):
    import torch
    count, W = x.shape[0], O.words(x.shape[2] + P, k)
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream
    d_out = gk.guarded_out(count * W)
    eng.trlwe_compress_dev(gk.to_device(x, np.uint32), k, P, d_out, count, coef, stride, st)
    eng.sync(st)
    return gk.read_guarded(d_out, count * W).reshape(count, W)


def _same(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, len(bad), bad[:5])


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n,count", [(1, 1), (1, 67), (635, 1), (635, 67), (767, 3)])
def test_tlwe_every_word(worlds, n, count, k):
    """(n + 1) k is no multiple of 32 in most shapes: the padding rule and the row boundaries; 67 rows of 2 values: rows smaller than a word"""
    w = worlds(1024, n)
    x = O.tlwe_inputs(100 * n + count + k, n, count, k)
    got = _tlwe_dev(w.eng, x, k)
    _same(got, O.tlwe_compress(x, k), "restatement")
    _same(got, w.R.tlwe_compress(n, k, x), "CPU twin")


def _coef_for(N, P):
    """(coef, stride) of a P: [N-1] alone, the issue's [N-1, 0, N/2], 33 entries with duplicates, NULL for the long lists (513: a second launch
    of one value; N: a whole row)"""
    if P == 1:
        return [N - 1], 1
    if P == 3:
        return [N - 1, 0, N // 2], 1
    if P == 33:
        c = np.random.default_rng(N).integers(0, N, 33)
        c[5] = c[4] = c[30] = c[0]                                                   # duplicates, neighbours and far apart
        return [int(v) for v in c], 1
    return None, 1


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("P", [1, 3, 33, 513, "N", "stride"])
@pytest.mark.parametrize("count", [1, 3, 37])
@pytest.mark.parametrize("N", [1024, 2048])
def test_trlwe_every_word(worlds, N, count, P, k):
    w = worlds(N, 635)
    if P == "stride":
        P, coef, stride = 16, None, N // 16
    else:
        P = N if P == "N" else P
        coef, stride = _coef_for(N, P)
    x = O.trlwe_inputs(N + 1000 * count + 10 * P + k, N, count, k, O.coefficients(P, coef, stride))
    got = _trlwe_dev(w.eng, x, k, P, coef, stride)
    _same(got, O.trlwe_compress(x, k, P, coef, stride), "restatement")
    _same(got, w.R.trlwe_compress(N, k, x, P, coef, stride), "CPU twin")


def test_a_smaller_call_leaves_the_rows_behind_it_alone(worlds):
    """3 of 5 rows into a buffer of 5: rows 3 and 4 keep their bytes (a launch writes count * W words and nothing else)"""
    import torch
    w = worlds(1024, 635)
    k, W = 10, O.words(636, 10)
    x = O.tlwe_inputs(77, 635, 5, k)
    d_out = torch.full((5 * W,), FILL, dtype=torch.int32, device="cuda")
    w.eng.tlwe_compress_dev(gk.to_device(x, np.uint32), k, d_out, 3)
    w.eng.sync()
    out = gk.words_of(d_out)
    assert np.array_equal(out[:3 * W].reshape(3, W), O.tlwe_compress(x[:3], k)) and (out[3 * W:] == FILL).all()


def test_launch_counts(worlds):
    """one launch, one more per further 512 kept coefficients"""
    import torch
    N = 1024
    w = worlds(N, 635)
    e = w.eng
    st = torch.cuda.current_stream().cuda_stream
    x = O.trlwe_inputs(5, N, 2, 12, np.arange(N))
    d_in, d_out = gk.to_device(x, np.uint32), torch.zeros(2 * O.words(2 * N, 12), dtype=torch.int32, device="cuda")
    for P, want in ((1, 1), (512, 1), (513, 2), (N, 2)):
        e.timer_begin(st)
        e.trlwe_compress_dev(d_in, 12, P, d_out, 2, None, 1, st)
        assert e.timer_end(st)[1] == want, P
    t = gk.to_device(O.tlwe_inputs(6, 635, 4, 10), np.uint32)
    e.timer_begin(st)
    e.tlwe_compress_dev(t, 10, d_out, 4, st)
    assert e.timer_end(st)[1] == 1


@pytest.fixture(scope="module")
def real():
    """real keys at the small TLWE dimension the extract tests use (n = 40 at N = 1024), a packing key, and 32 encrypted 2-bit messages"""
    import rustfhe_amd as R
    N = 1024
    rp = R.Params(n=SMALL_N[N], N=N)
    key0, key1, bk, ksk = R.keygen(rp, 0xC0A1)
    w = types.SimpleNamespace(R=R, N=N, rp=rp, key0=key0, key1=key1, bk=bk, ksk=ksk)
    w.eng = gk.engine(R, rp, bk, ksk)
    w.pk = R.packing_keygen(rp, key0, key1, 0xBACC)
    w.key = w.eng.packing_key(w.pk)
    w.msgs = np.random.default_rng(12).integers(0, 4, 32)
    w.ct = R.encrypt_torus(rp, key0, R.encode_msgs(w.msgs, 2), 0x5EED)
    w.f = lambda m: (3 * m + 1) % 4                                                  # noqa: E731
    yield w
    w.key.close()
    w.eng.close()


def test_pbs_pack_compress_end_to_end_and_captured(real):
    """32 PBS results packed 16 to a TRLWE and compressed at k = 12 on one stream; the key holder expands and every message decodes.  Then the
    compression alone captured FIRST THING on a fresh stream (it allocates nothing), and the whole chain captured on a stream that has run it
    eagerly once (the packing key switch's own capture rule asks for that), each replayed twice: the eager words."""
    import torch
    w, R, e = real, real.R, real.eng
    N, n1, G, P, k = w.N, w.rp.n + 1, 2, 16, 12
    W = O.words(N + P, k)
    want = w.f(w.msgs).reshape(G, P)
    with e.lut(R.lut_polynomial(w.f, N, 2)) as lut:
        d_ct = gk.to_device(w.ct, np.uint32)
        d_res = torch.zeros((G * P, n1), dtype=torch.int32, device="cuda")
        d_rows = torch.zeros((G, 2, N), dtype=torch.int32, device="cuda")
        d_out = gk.guarded_out(G * W)
        torch.cuda.synchronize()

        def chain(stream):
            e.pbs_batch_dev(lut, d_ct, d_res, G * P, None, stream)
            e.pack_batch_dev(w.key, d_res, P, d_rows, G, 1, None, stream)
            e.trlwe_compress_dev(d_rows, k, P, d_out, G, None, 1, stream)

        s = torch.cuda.Stream()
        chain(s.cuda_stream)
        e.sync(s.cuda_stream)
        eager = gk.read_guarded(d_out, G * W).reshape(G, W).copy()
        rows = gk.words_of(d_rows).reshape(G, 2, N).copy()
        assert np.array_equal(eager, O.trlwe_compress(rows, k, P)) and np.array_equal(eager, R.trlwe_compress(N, k, rows, P))
        back = R.trlwe_expand(N, k, eager, P)
        assert np.array_equal(R.decode_msgs(R.trlwe_phase(w.rp, w.key1, back)[:, :P].reshape(-1), 2).reshape(G, P), want)
        err = ((R.trlwe_phase(w.rp, w.key1, back)[:, :P].astype(np.int64) - R.trlwe_phase(w.rp, w.key1, rows)[:, :P].astype(np.int64) + 2 ** 31) % 2 ** 32
               - 2 ** 31) / 2.0 ** 32
        assert np.abs(err).max() <= (int(w.key1.sum()) + 1) * 2.0 ** -(k + 1)
        # the compression alone, first thing on a fresh stream
        fresh = torch.cuda.Stream()
        d_out2 = gk.guarded_out(G * W)
        with torch.cuda.stream(fresh):
            g1 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g1, stream=fresh):
                e.trlwe_compress_dev(d_rows, k, P, d_out2, G, None, 1, fresh.cuda_stream)
            for _ in range(2):
                d_out2.copy_(gk.to_device(gk.guarded(G * W), np.uint32))
                g1.replay()
                torch.cuda.synchronize()
                assert np.array_equal(gk.read_guarded(d_out2, G * W).reshape(G, W), eager)
        # the whole chain in one graph
        with torch.cuda.stream(s):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                chain(s.cuda_stream)
            for _ in range(2):
                d_rows.zero_()
                d_out.copy_(gk.to_device(gk.guarded(G * W), np.uint32))
                g.replay()
                torch.cuda.synchronize()
                assert np.array_equal(gk.read_guarded(d_out, G * W).reshape(G, W), eager)
        e.sync(s.cuda_stream)


def test_other_backends_and_a_two_entry_context_give_the_same_words(real):
    w, R = real, real.R
    N, n = w.N, w.rp.n
    t = O.tlwe_inputs(31, n, 5, 10)
    x = O.trlwe_inputs(32, N, 3, 12, np.array([N - 1, 0, N // 2]))
    want_t, want_x = O.tlwe_compress(t, 10), O.trlwe_compress(x, 12, 3, [N - 1, 0, N // 2])
    for backend in (R._ffi.BACKEND_NTT_EXACT, R._ffi.BACKEND_FFT_SPLIT_EXACT, "multi"):
        e = gk.engine(R, w.rp, w.bk, w.ksk, devices=[0, 0]) if backend == "multi" else gk.engine(R, w.rp, w.bk, w.ksk)
        try:
            if backend != "multi":
                e.set_backend(backend)
            assert np.array_equal(_tlwe_dev(e, t, 10), want_t), backend
            assert np.array_equal(_trlwe_dev(e, x, 12, 3, [N - 1, 0, N // 2], 1), want_x), backend
        finally:
            e.close()


def test_compressed_results_example(engine, keys):
    """examples/compressed_results.py at its default parameters on the session's engine and key set: every message decodes on all three routes,
    the routes are as small as the header says, and what the compression adds to the phase stays within its bound"""
    import importlib.util
    import os
    import rustfhe_amd as R
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("compressed_results", os.path.join(root, "examples", "compressed_results.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    res = ex.run(engine, keys.key0, keys.key1, R.packing_keygen(engine.p, keys.key0, keys.key1, 0xBACC), seed=0xC0FE)
    print({k: {a: (round(b, 5) if isinstance(b, float) else b) for a, b in v.items()} for k, v in res.items()})
    assert [r["bytes_per_result"] for r in res.values()] == [2544.0, 796.0, 3.0]
    for name, r in res.items():
        assert r["decoded"] == ex.RESULTS, (name, r)
        assert r["bound"] is None or r["added_max"] <= r["bound"], (name, r)


def test_refusals_launch_nothing(worlds):
    import torch
    N = 1024
    w = worlds(N, 635)
    R, e = w.R, w.eng
    n1 = w.rp.n + 1
    x = O.trlwe_inputs(9, N, 3, 12, np.arange(5))
    d_in = gk.to_device(x, np.uint32)
    d_out = torch.full((4 * 2 * N,), FILL, dtype=torch.int32, device="cuda")
    d_both = torch.full((4, 2, N), FILL, dtype=torch.int32, device="cuda")
    i32 = lambda *v: np.array(v, np.int32)                                          # noqa: E731
    INV = R._ffi.ERR_INVALID
    e.timer_begin()
    tl = lambda k, count=3, src=d_in.data_ptr(), dst=d_out.data_ptr(), ctx=e.h: e.L.rtfhe_tlwe_compress_batch_dev(ctx, k, src, dst, count, None)      # noqa: E731
    for args, word in (((1,), "k = 1"), ((33,), "k = 33"), ((0,), "k = 0"), ((-4,), "k = -4"), ((10, (1 << 31) // n1 + 1), "count * L"),
                       ((10, 3, 0), "null"), ((10, 3, d_in.data_ptr(), 0), "null"),
                       ((10, 2, d_both.data_ptr(), d_both.data_ptr()), "overlaps"), ((10, 2, d_both.data_ptr(), d_both.data_ptr() + 2 * n1 * 4 - 4), "overlaps")):
        with pytest.raises(R.RtfheError) as ei:
            e._ck(tl(*args))
        assert ei.value.code == INV and word in str(ei.value), (args, str(ei.value))
    assert tl(10, 3, d_in.data_ptr(), d_out.data_ptr(), None) == INV                # null context
    assert tl(10, 0) == 0                                                           # count = 0
    tr = lambda k, P, coef, stride, count=3, src=d_in.data_ptr(), dst=d_out.data_ptr(): e.L.rtfhe_trlwe_compress_batch_dev(      # noqa: E731
        e.h, k, src, P, None if coef is None else coef.ctypes.data, stride, dst, count, None)
    for args, word in (((1, 1, None, 1), "k = 1"), ((33, 1, None, 1), "k = 33"), ((12, 0, None, 1), "P = 0"), ((12, N + 1, None, 1), "P = %d" % (N + 1)),
                       ((12, 3, i32(0, -1, 5), 1), "sample 1: coef = -1"), ((12, 3, i32(0, 1, N), 1), "sample 2: coef = %d" % N),
                       ((12, 3, None, 0), "stride = 0"), ((12, 3, None, -2), "stride = -2"), ((12, 3, None, N // 2), "sample 2: coef = %d" % N),
                       ((12, N, None, 2), "sample %d: coef = %d" % (N // 2, N)), ((12, 1, None, 1, (1 << 31) // (N + 1) + 1), "count * L"),
                       ((12, 1, None, 1, 3, 0), "null"), ((12, 1, None, 1, 3, d_in.data_ptr(), 0), "null"),
                       ((12, 1, None, 1, 2, d_both.data_ptr(), d_both[1].data_ptr()), "overlaps"),
                       ((12, 1, None, 1, 2, d_both[1].data_ptr(), d_both[1].data_ptr() - 64), "overlaps")):
        with pytest.raises(R.RtfheError) as ei:
            e._ck(tr(*args))
        assert ei.value.code == INV and word in str(ei.value), (args[:4], str(ei.value))
    assert tr(12, 1, None, 1, 0) == 0
    # host pointers where device pointers belong
    for call in (lambda: tl(10, 3, np.ascontiguousarray(x).ctypes.data), lambda: tr(12, 1, None, 1, 3, np.ascontiguousarray(x).ctypes.data)):
        with pytest.raises(R.RtfheError) as ei:
            e._ck(call())
        assert ei.value.code == INV and "device pointers" in str(ei.value)
    assert e.timer_end()[1] == 0, "the checks come before any launch"
    e.sync()
    assert (gk.words_of(d_out) == FILL).all() and (gk.words_of(d_both) == FILL).all()
    # the output right behind the rows does not overlap them
    d_both[:2].copy_(gk.to_device(x[:2], np.uint32))
    e.trlwe_compress_dev(d_both[:2], 12, 5, d_both[2], 2, None, 1)
    e.sync()
    W = O.words(N + 5, 12)
    assert np.array_equal(gk.words_of(d_both[2:]).reshape(-1)[:2 * W].reshape(2, W), O.trlwe_compress(x[:2], 12, 5))
