"""GPU: device-side expansion of compressed rows (rtfhe_tlwe_expand_batch_dev, rtfhe_trlwe_expand_batch_dev; k_expand_rows).  Every output
word of both forms against the numpy restatement of the specification (tests/compress_oracle.py) AND against the CPU twin, on packed rows made
by the restatement from random rows with planted edge words, into 0x5A-filled outputs with canary words behind them -- a word the kernel does
not write shows as 0x5A5A5A5A, so "b is zero where nothing was kept" is checked on every word; the same with random bits in the padding of
every row's last word; the round trips with the compress calls on the device; the launch counts; the consumers of expanded rows; one
end-to-end chain with real keys through both forms, with the expansion captured first thing on a fresh stream; the other backends, a two-entry
context, the refusals, and the example."""
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


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _tlwe_dev(eng, words, n, k, stream=None):
    """the lvl0 _dev form into a guarded buffer; u32[count][n+1]"""
    count = words.shape[0]
    st = _stream() if stream is None else stream
    d_out = gk.guarded_out(count * (n + 1))
    eng.tlwe_expand_dev(gk.to_device(words, np.uint32), k, d_out, count, st)
    eng.sync(st)
    return gk.read_guarded(d_out, count * (n + 1)).reshape(count, n + 1)


def _trlwe_dev(eng, words, N, k, P, coef, stride, stream=None):
    count = words.shape[0]
    st = _stream() if stream is None else stream
    d_out = gk.guarded_out(count * 2 * N)
    eng.trlwe_expand_dev(gk.to_device(words, np.uint32), k, P, d_out, count, coef, stride, st)
    eng.sync(st)
    return gk.read_guarded(d_out, count * 2 * N).reshape(count, 2, N)


def _same(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, len(bad), bad[:5])


def _with_padding_bits(words, L, k, seed):
    """a copy with random bits planted in the bits of every row's last word past L k (none where L k is a multiple of 32)"""
    pad = words.shape[1] * 32 - L * k
    out = words.copy()
    if pad:
        junk = np.random.default_rng(seed).integers(1, 1 << pad, words.shape[0], dtype=np.uint64)
        junk |= np.uint64(1) << np.uint64(pad - 1)                                     # the top bit always: no row is left clean
        out[:, -1] |= (junk << np.uint64(32 - pad)).astype(np.uint32)
    return out


@pytest.mark.parametrize("padding", ["zero", "random"])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n,count", [(1, 1), (1, 67), (635, 1), (635, 67), (767, 3)])
def test_tlwe_every_word(worlds, n, count, k, padding):
    """rows smaller than a word (n = 1), values that straddle words, (n + 1) k no multiple of 32; padding bits reach no result"""
    w = worlds(1024, n)
    packed = O.tlwe_compress(O.tlwe_inputs(100 * n + count + k, n, count, k), k)
    want = O.tlwe_expand(packed, n, k)
    if padding == "random":
        packed = _with_padding_bits(packed, n + 1, k, n + count + k)
    got = _tlwe_dev(w.eng, packed, n, k)
    _same(got, want, "restatement")
    _same(got, w.R.tlwe_expand(n, k, packed), "CPU twin")


def test_tlwe_rows_of_a_larger_table_at_4_byte_alignment(worlds):
    """n = 634: rows of 635 words, so odd rows start 4 bytes off an 8-byte boundary, and W = 199 is odd too.  The output is rows 1 .. count of
    a larger table, the packed rows start one word into their buffer: both sides 4-byte aligned only; the rows around the range keep their bytes"""
    import torch
    n, k, count = 634, 10, 5
    w = worlds(1024, n)
    W = O.words(n + 1, k)
    assert (n + 1) % 2 == 1 and W % 2 == 1
    packed = O.tlwe_compress(O.tlwe_inputs(4321, n, count, k), k)
    d_table = torch.full((count + 2, n + 1), int(np.uint32(FILL).view(np.int32)), dtype=torch.int32, device="cuda")
    d_words = torch.zeros(count * W + 1, dtype=torch.int32, device="cuda")
    d_words[1:].copy_(gk.to_device(packed.reshape(-1), np.uint32))
    assert d_table[1].data_ptr() % 8 == 4 and d_words[1:].data_ptr() % 8 == 4
    w.eng.tlwe_expand_dev(d_words[1:], k, d_table[1], count)
    w.eng.sync()
    out = gk.words_of(d_table)
    _same(out[1:count + 1], O.tlwe_expand(packed, n, k), "restatement")
    assert (out[0] == FILL).all() and (out[count + 1] == FILL).all()


def _coef_for(N, P):
    """(coef, stride) of a P: [N-1] alone, the issue's [N-1, 0, N/2], 33 entries with duplicates (neighbours and far apart), NULL for the
    long lists"""
    if P == 1:
        return [N - 1], 1
    if P == 3:
        return [N - 1, 0, N // 2], 1
    if P == 33:
        c = np.random.default_rng(N).integers(0, N, 33)
        c[5] = c[4] = c[30] = c[0]
        return [int(v) for v in c], 1
    return None, 1


def _distinct_values(packed, N, P, k):
    """the packed rows with the P kept values replaced by values that differ from entry to entry where k allows, so that WHICH duplicate wins shows"""
    vals = O.unpack_rows(packed, N + P, k)
    vals[:, N:] = (vals[:, N:] + np.arange(P)) % (1 << k)
    return O.pack_rows(vals, k)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("P", [1, 3, 33, 513, "N", "stride"])
@pytest.mark.parametrize("count", [1, 3, 37])
@pytest.mark.parametrize("N", [1024, 2048])
def test_trlwe_every_word(worlds, N, count, P, k):
    """a at every word, b at every kept coefficient, the later entry of a duplicate, and ZERO at every other coefficient: the buffer is
    0x5A-filled, so a word that was skipped, or scattered over a memset, would show"""
    w = worlds(N, 635)
    if P == "stride":
        P, coef, stride = 16, None, N // 16
    else:
        P = N if P == "N" else P
        coef, stride = _coef_for(N, P)
    coefs = O.coefficients(P, coef, stride)
    packed = _distinct_values(O.trlwe_compress(O.trlwe_inputs(N + 1000 * count + 10 * P + k, N, count, k, coefs), k, P, coef, stride), N, P, k)
    packed = _with_padding_bits(packed, N + P, k, N + count + P + k)
    got = _trlwe_dev(w.eng, packed, N, k, P, coef, stride)
    want = O.trlwe_expand(packed, N, k, P, coef, stride)
    _same(got, want, "restatement")
    _same(got, w.R.trlwe_expand(N, k, packed, P, coef, stride), "CPU twin")
    others = np.setdiff1d(np.arange(N), coefs)
    assert not got[:, 0][:, others].any()


@pytest.mark.parametrize("k", KS)
def test_round_trips_on_the_device(worlds, k):
    """expand_dev(compress_dev(x)) is within 2^(31-k) of x on every word (b: on the kept words; zero elsewhere), and
    compress_dev(expand_dev(w)) is w again, for both forms"""
    N, n, count, P = 1024, 635, 5, 33
    w = worlds(N, n)
    e = w.eng
    lim = 0 if k == 32 else 2 ** (31 - k)
    centered = lambda d: ((d.astype(np.int64) + 2 ** 31) % 2 ** 32) - 2 ** 31      # noqa: E731
    # lvl0
    x = O.tlwe_inputs(50 + k, n, count, k)
    W = O.words(n + 1, k)
    d_x, d_w = gk.to_device(x, np.uint32), gk.guarded_out(count * W)
    d_y, d_w2 = gk.guarded_out(count * (n + 1)), gk.guarded_out(count * W)
    e.tlwe_compress_dev(d_x, k, d_w, count)
    e.tlwe_expand_dev(d_w, k, d_y, count)
    e.tlwe_compress_dev(d_y, k, d_w2, count)
    e.sync()
    y = gk.read_guarded(d_y, count * (n + 1)).reshape(count, n + 1)
    assert np.abs(centered(y.astype(np.int64) - x.astype(np.int64))).max() <= lim
    assert np.array_equal(gk.read_guarded(d_w2, count * W), gk.read_guarded(d_w, count * W))
    # TRLWE, a list with duplicates
    coef, _ = _coef_for(N, P)
    kept = np.unique(coef)
    x = O.trlwe_inputs(60 + k, N, count, k, np.asarray(coef))
    W = O.words(N + P, k)
    d_x, d_w = gk.to_device(x, np.uint32), gk.guarded_out(count * W)
    d_y, d_w2 = gk.guarded_out(count * 2 * N), gk.guarded_out(count * W)
    e.trlwe_compress_dev(d_x, k, P, d_w, count, coef)
    e.trlwe_expand_dev(d_w, k, P, d_y, count, coef)
    e.trlwe_compress_dev(d_y[:count * 2 * N], k, P, d_w2, count, coef)
    e.sync()
    y = gk.read_guarded(d_y, count * 2 * N).reshape(count, 2, N)
    assert np.abs(centered(y[:, 1].astype(np.int64) - x[:, 1].astype(np.int64))).max() <= lim
    assert np.abs(centered(y[:, 0][:, kept].astype(np.int64) - x[:, 0][:, kept].astype(np.int64))).max() <= lim
    assert not y[:, 0][:, np.setdiff1d(np.arange(N), kept)].any()
    assert np.array_equal(gk.read_guarded(d_w2, count * W), gk.read_guarded(d_w, count * W))


def test_launch_counts(worlds):
    """lvl0: one launch.  TRLWE with a NULL list: one, at both N.  With a list the inverse map travels 1,024 entries a launch: ceil(N / 1024)
    launches -- one at N = 1024, two at N = 2048 -- whatever P is"""
    import torch
    st = _stream()
    for N, with_list in ((1024, 1), (2048, 2)):
        e = worlds(N, 635).eng
        for P in (1, 33, N):
            W = O.words(N + P, 12)
            d_w = torch.zeros(2 * W, dtype=torch.int32, device="cuda")
            d_out = torch.zeros(2 * 2 * N, dtype=torch.int32, device="cuda")
            e.timer_begin(st)
            e.trlwe_expand_dev(d_w, 12, P, d_out, 2, None, 1, st)
            assert e.timer_end(st)[1] == 1, (N, P)
            e.timer_begin(st)
            e.trlwe_expand_dev(d_w, 12, P, d_out, 2, list(range(P - 1, -1, -1)), 1, st)
            assert e.timer_end(st)[1] == with_list, (N, P)
    e = worlds(1024, 635).eng
    d_w = torch.zeros(4 * O.words(636, 10), dtype=torch.int32, device="cuda")
    d_out = torch.zeros(4 * 636, dtype=torch.int32, device="cuda")
    e.timer_begin(st)
    e.tlwe_expand_dev(d_w, 10, d_out, 4, st)
    assert e.timer_end(st)[1] == 1


def test_a_smaller_call_leaves_the_rows_behind_it_alone(worlds):
    """3 of 5 rows: rows 3 and 4 of the output keep their bytes, in both forms (at N = 2048 with a list: both launches)"""
    import torch
    fill = int(np.uint32(FILL).view(np.int32))
    w = worlds(1024, 635)
    packed = O.tlwe_compress(O.tlwe_inputs(77, 635, 5, 10), 10)
    d_out = torch.full((5, 636), fill, dtype=torch.int32, device="cuda")
    w.eng.tlwe_expand_dev(gk.to_device(packed, np.uint32), 10, d_out, 3)
    w.eng.sync()
    out = gk.words_of(d_out)
    assert np.array_equal(out[:3], O.tlwe_expand(packed[:3], 635, 10)) and (out[3:] == FILL).all()
    N, P, coef = 2048, 3, [2047, 0, 1024]
    w = worlds(N, 635)
    packed = O.trlwe_compress(O.trlwe_inputs(78, N, 5, 12, np.asarray(coef)), 12, P, coef)
    d_out = torch.full((5, 2, N), fill, dtype=torch.int32, device="cuda")
    w.eng.trlwe_expand_dev(gk.to_device(packed, np.uint32), 12, P, d_out, 3, coef)
    w.eng.sync()
    out = gk.words_of(d_out)
    assert np.array_equal(out[:3], O.trlwe_expand(packed[:3], N, 12, P, coef)) and (out[3:] == FILL).all()


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


def test_extract_reads_device_expanded_rows_as_it_reads_cpu_expanded_ones(real):
    import torch
    w, R, e = real, real.R, real.eng
    N, n1, count, P, k = w.N, w.rp.n + 1, 3, 5, 12
    coef = [N - 1, 7, 7, 0, N // 2]
    packed = O.trlwe_compress(O.trlwe_inputs(91, N, count, k, np.asarray(coef)), k, P, coef)
    d_dev = e.upload_trlwe_compressed(packed, k, P, coef)
    d_cpu = gk.to_device(R.trlwe_expand(N, k, packed, P, coef), np.uint32)
    outs = []
    for d_rows in (d_dev, d_cpu):
        d_out = torch.zeros((count, P, n1), dtype=torch.int32, device="cuda")
        e.trlwe_extract_batch_dev(d_rows, P, d_out, count, coef, 1, _stream())
        e.sync(_stream())
        outs.append(gk.words_of(d_out))
    assert np.array_equal(gk.words_of(d_dev), gk.words_of(d_cpu)) and np.array_equal(outs[0], outs[1])


def test_an_encrypted_table_takes_expanded_rows(real):
    """Lut.update_dev from device-expanded rows, then Lut.read_dev: those rows"""
    import torch
    w, R, e = real, real.R, real.eng
    N, count, k = w.N, 3, 12
    packed = O.trlwe_compress(O.trlwe_inputs(92, N, count, k, np.arange(N)), k, N)
    d_rows = e.upload_trlwe_compressed(packed, k, N)
    with e.lut_encrypted(np.zeros((count + 1, 2, N), np.uint32)) as lut:
        d_back = torch.zeros((count, 2, N), dtype=torch.int32, device="cuda")
        lut.update_dev(d_rows, 1, count, _stream())
        lut.read_dev(d_back, 1, count, _stream())
        e.sync(_stream())
    assert np.array_equal(gk.words_of(d_back), O.trlwe_expand(packed, N, k, N))
    assert np.array_equal(gk.words_of(d_back), R.trlwe_expand(N, k, packed, N))


def test_both_forms_end_to_end_and_captured(real):
    """PBS -> compress k = 10 -> host -> upload_tlwe_compressed -> PBS -> decode, and the packed form at k = 12 through pack, compress,
    upload_trlwe_compressed, extract and PBS: f(f(m)) for all 32 messages both ways.  Then each expansion captured FIRST THING on a fresh stream
    (it allocates nothing; the list is baked in when the call is captured) and replayed twice: the eager words."""
    import torch
    w, R, e = real, real.R, real.eng
    N, n, n1, G, P = w.N, w.rp.n, w.rp.n + 1, 2, 16
    k0, k1 = 10, 12
    W0, W1 = O.words(n1, k0), O.words(N + P, k1)
    want = w.f(w.f(w.msgs))
    st = _stream()
    with e.lut(R.lut_polynomial(w.f, N, 2)) as lut:
        d_ct = gk.to_device(w.ct, np.uint32)
        d_res = torch.zeros((G * P, n1), dtype=torch.int32, device="cuda")
        d_rows = torch.zeros((G, 2, N), dtype=torch.int32, device="cuda")
        d_w0, d_w1 = gk.guarded_out(G * P * W0), gk.guarded_out(G * W1)
        e.pbs_batch_dev(lut, d_ct, d_res, G * P, None, st)
        e.tlwe_compress_dev(d_res, k0, d_w0, G * P, st)
        e.pack_batch_dev(w.key, d_res, P, d_rows, G, 1, None, st)
        e.trlwe_compress_dev(d_rows, k1, P, d_w1, G, None, 1, st)
        e.sync(st)
        lvl0 = gk.read_guarded(d_w0, G * P * W0).reshape(G * P, W0).copy()           # what a server keeps at rest
        packed = gk.read_guarded(d_w1, G * W1).reshape(G, W1).copy()
        # lvl0 form
        d_in = e.upload_tlwe_compressed(lvl0, k0)
        assert np.array_equal(gk.words_of(d_in), R.tlwe_expand(n, k0, lvl0))
        d_out = torch.zeros((G * P, n1), dtype=torch.int32, device="cuda")
        e.pbs_batch_dev(lut, d_in, d_out, G * P, None, st)
        e.sync(st)
        assert np.array_equal(R.decode_msgs(R.phases(w.rp, w.key0, gk.words_of(d_out)), 2), want)
        # packed form
        d_full = e.upload_trlwe_compressed(packed, k1, P)
        assert np.array_equal(gk.words_of(d_full), R.trlwe_expand(N, k1, packed, P))
        d_ext = torch.zeros((G, P, n1), dtype=torch.int32, device="cuda")
        e.trlwe_extract_batch_dev(d_full, P, d_ext, G, None, 1, st)
        e.pbs_batch_dev(lut, d_ext, d_out, G * P, None, st)
        e.sync(st)
        assert np.array_equal(R.decode_msgs(R.phases(w.rp, w.key0, gk.words_of(d_out)), 2), want)
    # captured first thing on a fresh stream
    d_l, d_p = gk.to_device(lvl0, np.uint32), gk.to_device(packed, np.uint32)
    coef = np.arange(P, dtype=np.int32)
    for run, words, eager in ((lambda d, s: e.tlwe_expand_dev(d_l, k0, d, G * P, s), G * P * n1, gk.words_of(d_in).reshape(-1)),
                              (lambda d, s: e.trlwe_expand_dev(d_p, k1, P, d, G, coef, 1, s), G * 2 * N, gk.words_of(d_full).reshape(-1))):
        fresh = torch.cuda.Stream()
        d_cap = gk.guarded_out(words)
        with torch.cuda.stream(fresh):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=fresh):
                run(d_cap, fresh.cuda_stream)
            coef[:] = 0                                                              # the capture holds its own copy of the list
            for _ in range(2):
                d_cap.copy_(gk.to_device(gk.guarded(words), np.uint32))
                g.replay()
                torch.cuda.synchronize()
                assert np.array_equal(gk.read_guarded(d_cap, words), eager)
        coef[:] = np.arange(P)


def test_other_backends_and_a_two_entry_context_give_the_same_words(real):
    w, R = real, real.R
    N, n = w.N, w.rp.n
    coef = [N - 1, 0, N // 2]
    t = O.tlwe_compress(O.tlwe_inputs(31, n, 5, 10), 10)
    x = O.trlwe_compress(O.trlwe_inputs(32, N, 3, 12, np.array(coef)), 12, 3, coef)
    want_t, want_x = O.tlwe_expand(t, n, 10), O.trlwe_expand(x, N, 12, 3, coef)
    for backend in (R._ffi.BACKEND_NTT_EXACT, R._ffi.BACKEND_FFT_SPLIT_EXACT, "multi"):
        e = gk.engine(R, w.rp, w.bk, w.ksk, devices=[0, 0]) if backend == "multi" else gk.engine(R, w.rp, w.bk, w.ksk)
        try:
            if backend != "multi":
                e.set_backend(backend)
            assert np.array_equal(_tlwe_dev(e, t, n, 10), want_t), backend
            assert np.array_equal(_trlwe_dev(e, x, N, 12, 3, coef, 1), want_x), backend
        finally:
            e.close()


def test_compressed_store_example(engine, keys):
    """examples/compressed_store.py at its default parameters, the computing side on the session's engine and the reading side on a fresh one
    with the same evaluation keys: all 1,024 results decode after the second PBS on both forms and on the uncompressed chain"""
    import importlib.util
    import os
    import rustfhe_amd as R
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("compressed_store", os.path.join(root, "examples", "compressed_store.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    reader = gk.engine(R, engine.p, keys.bk_t, keys.ksk)
    try:
        res = ex.run(engine, reader, keys.key0, keys.key1, R.packing_keygen(engine.p, keys.key0, keys.key1, 0xBACC), seed=0xC0FE)
    finally:
        reader.close()
    print({k: {a: (round(b, 5) if isinstance(b, float) else b) for a, b in v.items()} for k, v in res.items()})
    assert len(res) == 3
    for name, r in res.items():
        assert r["decoded"] == ex.RESULTS == 1024, (name, r)


def test_refusals_launch_nothing(worlds):
    import torch
    N = 1024
    w = worlds(N, 635)
    R, e = w.R, w.eng
    n1 = w.rp.n + 1
    W0, W1 = O.words(n1, 10), O.words(N + 1, 12)
    d_in = torch.full((4 * 2 * N,), FILL, dtype=torch.int32, device="cuda")
    d_out = torch.full((4 * 2 * N,), FILL, dtype=torch.int32, device="cuda")
    d_both = torch.full((4, 2, N), FILL, dtype=torch.int32, device="cuda")
    host = np.zeros(4 * 2 * N, np.uint32)
    i32 = lambda *v: np.array(v, np.int32)                                          # noqa: E731
    INV = R._ffi.ERR_INVALID
    e.timer_begin()
    tl = lambda k, count=3, src=d_in.data_ptr(), dst=d_out.data_ptr(), ctx=e.h: e.L.rtfhe_tlwe_expand_batch_dev(ctx, k, src, dst, count, None)      # noqa: E731
    for args, word in (((1,), "k = 1"), ((33,), "k = 33"), ((0,), "k = 0"), ((-4,), "k = -4"), ((10, (1 << 31) // n1 + 1), "count * L"),
                       ((10, 3, 0), "null"), ((10, 3, d_in.data_ptr(), 0), "null"),
                       ((10, 2, d_both.data_ptr(), d_both.data_ptr()), "overlaps"), ((10, 2, d_both.data_ptr(), d_both.data_ptr() + 2 * W0 * 4 - 4), "overlaps"),
                       ((10, 2, d_both.data_ptr() + 2 * n1 * 4 - 4, d_both.data_ptr()), "overlaps")):
        with pytest.raises(R.RtfheError) as ei:
            e._ck(tl(*args))
        assert ei.value.code == INV and word in str(ei.value) and "rtfhe_tlwe_expand_batch_dev" in str(ei.value), (args, str(ei.value))
    assert tl(10, 3, d_in.data_ptr(), d_out.data_ptr(), None) == INV                # null context
    assert tl(10, 0) == 0                                                           # count = 0
    tr = lambda k, P, coef, stride, count=3, src=d_in.data_ptr(), dst=d_out.data_ptr(): e.L.rtfhe_trlwe_expand_batch_dev(      # noqa: E731
        e.h, k, src, P, None if coef is None else coef.ctypes.data, stride, dst, count, None)
    for args, word in (((1, 1, None, 1), "k = 1"), ((33, 1, None, 1), "k = 33"), ((12, 0, None, 1), "P = 0"), ((12, N + 1, None, 1), "P = %d" % (N + 1)),
                       ((12, 3, i32(0, -1, 5), 1), "sample 1: coef = -1"), ((12, 3, i32(0, 1, N), 1), "sample 2: coef = %d" % N),
                       ((12, 3, None, 0), "stride = 0"), ((12, 3, None, -2), "stride = -2"), ((12, 3, None, N // 2), "sample 2: coef = %d" % N),
                       ((12, N, None, 2), "sample %d: coef = %d" % (N // 2, N)), ((12, 1, None, 1, (1 << 31) // (N + 1) + 1), "count * L"),
                       ((12, 1, None, 1, 3, 0), "null"), ((12, 1, None, 1, 3, d_in.data_ptr(), 0), "null"),
                       ((12, 1, None, 1, 2, d_both.data_ptr(), d_both.data_ptr() + 2 * W1 * 4 - 4), "overlaps"),
                       ((12, 1, None, 1, 2, d_both[1].data_ptr(), d_both[1].data_ptr() - 64), "overlaps")):
        with pytest.raises(R.RtfheError) as ei:
            e._ck(tr(*args))
        assert ei.value.code == INV and word in str(ei.value) and "rtfhe_trlwe_expand_batch_dev" in str(ei.value), (args[:4], str(ei.value))
    assert tr(12, 1, None, 1, 0) == 0
    # host pointers where device pointers belong
    for call in (lambda: tl(10, 3, host.ctypes.data), lambda: tr(12, 1, None, 1, 3, host.ctypes.data),
                 lambda: tl(10, 3, d_in.data_ptr(), host.ctypes.data), lambda: tr(12, 1, None, 1, 3, d_in.data_ptr(), host.ctypes.data)):
        with pytest.raises(R.RtfheError) as ei:
            e._ck(call())
        assert ei.value.code == INV and "device pointers" in str(ei.value)
    # the upload helpers refuse on the host
    for bad in (lambda: e.upload_tlwe_compressed(np.zeros((2, W0 + 1), np.uint32), 10), lambda: e.upload_tlwe_compressed(np.zeros((2, W0), np.uint32), 1),
                lambda: e.upload_trlwe_compressed(np.zeros((2, W1), np.uint32), 12, 0), lambda: e.upload_trlwe_compressed(np.zeros(W1 + 1, np.uint32), 12, 1)):
        with pytest.raises(R.RtfheError) as ei:
            bad()
        assert ei.value.code == INV
    assert e.timer_end()[1] == 0, "the checks come before any launch"
    e.sync()
    assert (gk.words_of(d_out) == FILL).all() and (gk.words_of(d_both) == FILL).all() and not host.any()
    # the full rows right behind the packed rows do not overlap them
    packed = O.trlwe_compress(O.trlwe_inputs(9, N, 2, 12, np.arange(5)), 12, 5)
    W5 = packed.shape[1]
    flat = d_both.reshape(-1)
    flat[:2 * W5].copy_(gk.to_device(packed.reshape(-1), np.uint32))
    e.trlwe_expand_dev(flat, 12, 5, flat[2 * W5:], 2, None, 1)
    e.sync()
    assert np.array_equal(gk.words_of(flat[2 * W5:2 * W5 + 2 * 2 * N]).reshape(2, 2, N), O.trlwe_expand(packed, N, 12, 5))
