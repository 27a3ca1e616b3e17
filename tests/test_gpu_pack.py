"""GPU: the packing key switch (rtfhe_packing_key_create, rtfhe_pack_batch[_dev], rtfhe_lut_update_dev; k_pkmat_build, k_pack_ks_mm,
k_pack_combine).  Every word against the numpy oracle (tests/pack_oracle.py) on keys of random words with planted edge words -- the arithmetic
does not care what the key encrypts --, the table convention against lut_polynomial, meaning and noise with real keys, a tree PBS composed
from the existing entry points, capture and replay, the exact backends, refusals and lifetimes."""
import types

import numpy as np
import pytest

import gpu_kit as gk
import pack_helpers as H
import pack_oracle as O

pytestmark = pytest.mark.gpu

EDGE_KEY = np.array([0, 0x7F, 0x80, 0xFF, 0x7FFFFFFF, 0x80000000, 0x80808080, 0x7F7F7F7F, 0xFFFFFFFF], np.uint32)
EDGE_A = np.array([0x00007FFF, 0x00008000, 0xFFFF7FFF, 0xFFFF8000, 0xFFFFFFFF, 0], np.uint32)


def _inputs(rng, rp, M):
    """M lvl0 rows of random words with the edge values of the rounding among the a_i of every row"""
    t = rng.integers(0, 1 << 32, (M, rp.n + 1), dtype=np.uint64).astype(np.uint32)
    for m in range(M):
        for k in range(min(rp.n, 2 * len(EDGE_A))):
            t[m, (5 * m + 3 * k) % rp.n if rp.n > 12 else k % rp.n] = EDGE_A[(m + k) % len(EDGE_A)]
    return t


def _plant(rp, pk, tlwe):
    """edge words into the key rows that the digits of the first rows of tlwe select"""
    rows = pk.reshape(-1, 2 * rp.N)
    d = O.digits(tlwe[:4, :rp.n])
    r = 0
    for m in range(d.shape[0]):
        for i, j in zip(*np.nonzero(d[m])):
            row = (i * rp.ks_t + j) * 3 + d[m, i, j] - 1
            for e, w in enumerate(EDGE_KEY):
                rows[row, (11 * r + 5 * e) % (2 * rp.N)] = w
            r += 1
            if r % 200 == 0:
                break


@pytest.fixture(scope="module")
def worlds():
    """one engine (no bootstrapping key, no key-switching key), one key of random words and its handle per (N, n); built on first use"""
    import rustfhe_amd as R

    def build(N, n):
        rng = np.random.default_rng(N + n)
        w = types.SimpleNamespace(R=R, rp=R.Params(n=n, N=N), N=N)
        w.pk = rng.integers(0, 1 << 32, (n, 8, 3, 2, N), dtype=np.uint64).astype(np.uint32)
        w.probe = _inputs(np.random.default_rng(1), w.rp, 4)      # rows 0 .. 3 of every shape's batch (see _shape_inputs)
        _plant(w.rp, w.pk, w.probe)
        w.eng = R.Engine(w.rp, 0)
        w.key = w.eng.packing_key(w.pk)
        return w
    made = gk.Worlds(build, close=lambda w: (w.key.close(), w.eng.close()))
    yield made
    made.close()


def _shape_inputs(w, count, P, seed):
    t = _inputs(np.random.default_rng(seed), w.rp, count * P)
    k = min(4, count * P)
    t[:k] = w.probe[:k]                                             # the rows whose digits select the planted key words
    return t.reshape(count, P, w.rp.n + 1)


def _pack_dev(w, tlwe, P, pos, rep, eng=None, key=None, stream=None):
    import torch
    e, key = eng or w.eng, key or w.key
    count = tlwe.shape[0]
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream
    d_in = gk.to_device(tlwe, np.uint32)
    d_out = torch.full((count, 2, w.N), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    e.pack_batch_dev(key, d_in, P, d_out, count, rep, pos, st)
    e.sync(st)
    return d_out.cpu().numpy().view(np.uint32)


N1 = 1024
SHAPES = [
    # N, n, count, P, rep, pos
    (N1, 635, 1, 1, 1, [0]),
    (N1, 635, 3, 5, 1, None),
    (N1, 635, 2, 5, 1, [0, 1, N1 - 1, N1, 2 * N1 - 1]),
    (N1, 635, 3, 4, 256, "table2"),
    (N1, 635, 5, 16, 3, [0, 1, 2, 2, 700, 1022, 1023, 1024, 1025, 2046, 2047, 5, 6, 300, 1500, 1501]),      # overlapping runs; M = 80
    (N1, 33, 37, 16, 1, None),                                                                             # M = 592: a second workgroup
    (N1, 1, 2, 3, 1, None),
    (N1, 636, 2, 3, 1, None),
    (N1, 767, 2, 3, 1, None),
    (2048, 635, 2, 3, 1, None),
    (2048, 635, 2, 3, 512, None),
]


@pytest.mark.parametrize("N,n,count,P,rep,pos", SHAPES, ids=lambda v: "table" if isinstance(v, str) else ("pos" if isinstance(v, list) else str(v)))
def test_every_word_equals_the_oracle(worlds, N, n, count, P, rep, pos):
    w = worlds(N, n)
    if pos == "table2":
        pos, r2 = w.R.lut_pack_layout(N, 2)
        assert r2 == rep
    tlwe = _shape_inputs(w, count, P, 1000 * count + 10 * P + rep)
    want = O.pack(w.rp, w.pk, tlwe, P, pos, rep)
    got = w.eng.pack_batch(w.key, tlwe, P, rep, pos)
    assert got.shape == (count, 2, N) and got.dtype == np.uint32
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), bad[:5])
    assert np.array_equal(_pack_dev(w, tlwe, P, pos, rep), want)


def test_more_positions_than_one_launch_carries(worlds):
    """P = 600 > 512: the combine step runs as two launches, the second adding to the first's words; rep = 1 and rep = 2 (overlapping runs)"""
    w = worlds(N1, 33)
    P = 600
    tlwe = _shape_inputs(w, 2, P, 77)
    pos = np.random.default_rng(5).integers(0, 2 * N1, P).astype(np.int32)
    for rep in (1, 2):
        want = O.pack(w.rp, w.pk, tlwe, P, pos, rep)
        assert np.array_equal(w.eng.pack_batch(w.key, tlwe, P, rep, pos), want)
        assert np.array_equal(_pack_dev(w, tlwe, P, pos, rep), want)


@pytest.mark.parametrize("N,p", [(1024, 1), (1024, 2), (1024, 3), (2048, 2)])
def test_table_layout_on_the_device(N, p):
    """zero key, trivial samples: lut_polynomial's words, as in the host test"""
    import rustfhe_amd as R
    rp = R.Params(n=12, N=N)
    f = np.random.default_rng(100 * p + N).integers(0, 1 << p, 1 << p)
    tlwe = np.zeros((1, 1 << p, rp.n + 1), np.uint32)
    tlwe[0, :, rp.n] = R.encode_msgs(f, p)
    pos, rep = R.lut_pack_layout(N, p)
    e = R.Engine(rp, 0)
    try:
        with e.packing_key(np.zeros((rp.n, 8, 3, 2, N), np.uint32)) as key:
            out = e.pack_batch(key, tlwe, 1 << p, rep, pos)
        assert np.array_equal(out[0, 0], R.lut_polynomial(list(f), N, p)) and not out[0, 1].any()
    finally:
        e.close()


@pytest.fixture(scope="module")
def real_dev(params, keys, engine):
    """the suite's key set (n = 635, N = 1024) with a packing key on the session's engine, 1,024 fresh encryptions of +-1/8 and their
    key-switched rows from the oracle (shared, read-only)"""
    import rustfhe_amd as R
    w = types.SimpleNamespace(R=R, rp=engine.p, N=params.N, eng=engine, key0=keys.key0, key1=keys.key1)
    w.pk = R.packing_keygen(w.rp, w.key0, w.key1, 0xBACC)
    w.key = engine.packing_key(w.pk)
    w.mu = np.where(np.random.default_rng(3).integers(0, 2, 1024) == 1, 0x20000000, 0xE0000000).astype(np.uint32)
    w.ct = R.encrypt_torus(w.rp, w.key0, w.mu, 5)
    w.S = O.key_switch(w.rp, w.pk, w.ct)
    yield w
    w.key.close()


@pytest.mark.parametrize("case", ["P1024_rep1", "table_P4_rep256"])
def test_meaning_with_real_keys(real_dev, case):
    w = real_dev
    if case == "P1024_rep1":
        P, pos, rep = 1024, None, 1
    else:
        pos, rep = w.R.lut_pack_layout(w.N, 2)
        P = 4
    tlwe = w.ct.reshape(-1, P, w.rp.n + 1)
    got = w.eng.pack_batch(w.key, tlwe, P, rep, pos)
    inside, outside = H.pack_noise(w.R, w.rp, w.key0, w.key1, w.ct, got, P, pos, rep)
    bound = H.noise_bound(w.rp, w.key0, P, rep)
    print("%s: h = %d, max distance on runs %.3e, outside runs %.3e, bound %.3e" % (case, int(w.key0.sum()), inside, outside, bound))
    assert inside <= bound and outside <= bound
    assert np.array_equal(got, O.combine(w.S, P, pos, rep))
    assert np.array_equal(_pack_dev(w, tlwe, P, pos, rep), got)


def _tree_inputs(w, seed):
    """a random 4-bit -> 2-bit function f[hi][lo] and 8 replicas of each of the 16 (hi, lo) pairs, encrypted at 2 bits"""
    R = w.R
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 4, (4, 4))
    hi, lo = np.repeat(np.arange(16) >> 2, 8), np.repeat(np.arange(16) & 3, 8)
    c_hi = R.encrypt_torus(w.rp, w.key0, R.encode_msgs(hi, 2), seed + 1)
    c_lo = R.encrypt_torus(w.rp, w.key0, R.encode_msgs(lo, 2), seed + 2)
    tabs = np.stack([R.lut_polynomial(list(f[h]), w.N, 2) for h in range(4)])
    return f, hi, lo, c_hi, c_lo, tabs


def test_tree_pbs_on_the_device(real_dev):
    """f(hi, lo) in 5 bootstraps: four PBS of lo with the sub-tables f(h, .), their outputs packed into an encrypted table row per input,
    one PBS of hi with that row.  Nothing leaves the device between the stages."""
    import torch
    w, R, e = real_dev, real_dev.R, real_dev.eng
    f, hi, lo, c_hi, c_lo, tabs = _tree_inputs(w, 41)
    G, n1 = 128, w.rp.n + 1
    st = torch.cuda.current_stream().cuda_stream
    pos, rep = R.lut_pack_layout(w.N, 2)
    with e.lut(tabs) as sub, e.lut_encrypted(np.zeros((G, 2, w.N), np.uint32)) as row:
        d_lo4 = gk.to_device(np.repeat(c_lo, 4, axis=0), np.uint32)                 # input g four times: with sub-table 0 .. 3
        d_idx4 = gk.to_device(np.tile(np.arange(4, dtype=np.int32), G))
        d_sub = torch.zeros((G * 4, n1), dtype=torch.int32, device="cuda")
        d_rows = torch.zeros((G, 2, w.N), dtype=torch.int32, device="cuda")
        d_hi, d_g = gk.to_device(c_hi, np.uint32), gk.to_device(np.arange(G, dtype=np.int32))
        d_out = torch.zeros((G, n1), dtype=torch.int32, device="cuda")
        e.pbs_batch_dev(sub, d_lo4, d_sub, G * 4, d_idx4, st)
        e.pack_batch_dev(w.key, d_sub, 4, d_rows, G, rep, pos, st)
        row.update_dev(d_rows, 0, G, st)
        e.pbs_batch_dev(row, d_hi, d_out, G, d_g, st)
        e.sync(st)
        got = R.decode_msgs(R.phases(w.rp, w.key0, d_out.cpu().numpy().view(np.uint32)), 2)
        assert np.array_equal(got, f[hi, lo]), np.flatnonzero(got != f[hi, lo])
        # the packed rows are tables of h -> f(h, lo_g): every box centre within 1/16 of its entry
        ph = R.trlwe_phase(w.rp, w.key1, d_rows.cpu().numpy().view(np.uint32))
        for h in range(1, 4):
            assert np.array_equal(R.decode_msgs(ph[:, h * rep], 2), f[h, lo])


def test_tree_pbs_through_the_host_forms(real_dev):
    w, R, e = real_dev, real_dev.R, real_dev.eng
    f, hi, lo, c_hi, c_lo, tabs = _tree_inputs(w, 43)
    G = 128
    pos, rep = R.lut_pack_layout(w.N, 2)
    with e.lut(tabs) as sub:
        s1 = e.pbs_batch(sub, np.repeat(c_lo, 4, axis=0), np.tile(np.arange(4, dtype=np.int32), G))
    rows = e.pack_batch(w.key, s1.reshape(G, 4, -1), 4, rep, pos)
    with e.lut_encrypted(rows) as row:
        out = e.pbs_batch(row, c_hi, np.arange(G, dtype=np.int32))
    got = R.decode_msgs(R.phases(w.rp, w.key0, out), 2)
    assert np.array_equal(got, f[hi, lo]), np.flatnonzero(got != f[hi, lo])


def test_capture_replay_and_two_streams(worlds):
    import torch
    w = worlds(N1, 33)
    R, e = w.R, w.eng
    count, P, rep = 3, 4, 256
    pos, _ = R.lut_pack_layout(N1, 2)
    a, b = _shape_inputs(w, count, P, 501), _shape_inputs(w, count, P, 502)
    want_a, want_b = O.pack(w.rp, w.pk, a, P, pos, rep), O.pack(w.rp, w.pk, b, P, pos, rep)
    s, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    d_in, d_in2 = gk.to_device(a, np.uint32), gk.to_device(b, np.uint32)
    out = torch.zeros((count, 2, N1), dtype=torch.int32, device="cuda")
    out2 = torch.zeros((count, 2, N1), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    # a capture on a stream that never ran an eager pack is refused, and the capture goes on
    refused = []
    with torch.cuda.stream(s):
        g0 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g0, stream=s):
            try:
                e.pack_batch_dev(w.key, d_in, P, out, count, rep, pos, s.cuda_stream)
            except R.RtfheError as err:
                refused.append(err)
            out2.zero_()
    assert len(refused) == 1 and refused[0].code == R._ffi.ERR_STATE and "capture" in str(refused[0])
    e.sync(s.cuda_stream)
    # eager on s, then captured on s: the replay gives the eager words, also after the input is rewritten (pos is baked in)
    e.pack_batch_dev(w.key, d_in, P, out, count, rep, pos, s.cuda_stream)
    e.sync(s.cuda_stream)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want_a)
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            e.pack_batch_dev(w.key, d_in, P, out, count, rep, pos, s.cuda_stream)
        for src, exp in ((a, want_a), (b, want_b)):
            d_in.copy_(gk.to_device(src, np.uint32))
            out.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy().view(np.uint32), exp)
    # two streams side by side, each with its own buffer of key-switched samples
    d_in.copy_(gk.to_device(a, np.uint32))
    torch.cuda.synchronize()
    for _ in range(3):
        e.pack_batch_dev(w.key, d_in, P, out, count, rep, pos, s.cuda_stream)
        e.pack_batch_dev(w.key, d_in2, P, out2, count, rep, pos, s2.cuda_stream)
    e.sync(s.cuda_stream)
    e.sync(s2.cuda_stream)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want_a) and np.array_equal(out2.cpu().numpy().view(np.uint32), want_b)


def test_larger_eager_pack_retires_the_buffer_a_graph_holds(worlds):
    """A fresh stream: an eager pack of 3 x 4 samples, the same call captured, then an eager pack of 9 x 4 samples on that stream, which replaces
    the stream's buffer of key-switched samples.  The graph holds the old buffer's address: it is kept, not freed, so the replays still give
    the small call's words, and the large call gives the oracle's."""
    import torch
    w = worlds(N1, 33)
    R, e = w.R, w.eng
    P, rep = 4, 256
    pos, _ = R.lut_pack_layout(N1, 2)
    a, b = _shape_inputs(w, 3, P, 501), _shape_inputs(w, 9, P, 503)
    want_a, want_b = O.pack(w.rp, w.pk, a, P, pos, rep), O.pack(w.rp, w.pk, b, P, pos, rep)
    s = torch.cuda.Stream()
    d_a, d_b = gk.to_device(a, np.uint32), gk.to_device(b, np.uint32)
    out = torch.zeros((3, 2, N1), dtype=torch.int32, device="cuda")
    big = torch.zeros((9, 2, N1), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        e.pack_batch_dev(w.key, d_a, P, out, 3, rep, pos, s.cuda_stream)
        e.sync(s.cuda_stream)
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want_a)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            e.pack_batch_dev(w.key, d_a, P, out, 3, rep, pos, s.cuda_stream)
        e.pack_batch_dev(w.key, d_b, P, big, 9, rep, pos, s.cuda_stream)
        e.sync(s.cuda_stream)
        assert np.array_equal(big.cpu().numpy().view(np.uint32), want_b)
        for _ in range(2):
            out.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy().view(np.uint32), want_a)
    e.sync(s.cuda_stream)


def test_exact_backends_give_the_same_words(worlds):
    w = worlds(N1, 33)
    R, e = w.R, w.eng
    tlwe = _shape_inputs(w, 2, 5, 601)
    want = e.pack_batch(w.key, tlwe, 5, 3, None)
    assert np.array_equal(want, O.pack(w.rp, w.pk, tlwe, 5, None, 3))
    try:
        for backend in (R._ffi.BACKEND_NTT_EXACT, R._ffi.BACKEND_FFT_SPLIT_EXACT):
            e.set_backend(backend)
            assert np.array_equal(e.pack_batch(w.key, tlwe, 5, 3, None), want)
    finally:
        e.set_backend(R._ffi.BACKEND_FFT64_MIRROR)


def test_refusals_and_lifetimes(worlds):
    import ctypes as C
    import torch
    w = worlds(N1, 33)
    R, e, N = w.R, w.eng, N1
    tlwe = _shape_inputs(w, 1, 3, 701)
    ref = e.pack_batch(w.key, tlwe, 3, 1, None)
    big = np.zeros((1, N + 1, w.rp.n + 1), np.uint32)

    def refused(fn, code=R._ffi.ERR_INVALID, word=None):
        with pytest.raises(R.RtfheError) as ei:
            fn()
        assert ei.value.code == code and (word is None or word in str(ei.value)), str(ei.value)
        e.sync()                                                    # nothing was launched, nothing is pending

    out = np.empty((1, 2, N), np.uint32)
    call = lambda t, P, pos, rep: e.L.rtfhe_pack_batch(e.h, w.key.h, t.ctypes.data, P, None if pos is None else pos.ctypes.data, rep, out.ctypes.data, 1)    # noqa: E731
    i32 = lambda *v: np.array(v, np.int32)                                                                                                             # noqa: E731
    for args, word in (((tlwe, 0, None, 1), "P = 0"), ((big, N + 1, None, 1), "P = %d" % (N + 1)), ((tlwe, 3, None, 0), "rep = 0"),
                       ((tlwe, 3, None, N + 1), "rep"), ((tlwe, 3, i32(0, 2 * N, 1), 1), "pos = %d" % (2 * N)), ((tlwe, 3, i32(0, 1, -1), 1), "pos = -1"),
                       ((tlwe, 3, None, N), "pos NULL")):
        refused(lambda: e._ck(call(*args)), word=word)
    d_in, d_out = gk.to_device(tlwe, np.uint32), torch.zeros((1, 2, N), dtype=torch.int32, device="cuda")
    refused(lambda: e.pack_batch_dev(w.key, d_in, 0, d_out, 1), word="P = 0")
    refused(lambda: e.pack_batch_dev(w.key, d_in, 3, d_out, 1, 1, [0, -1, 5]), word="pos = -1")
    refused(lambda: e._ck(e.L.rtfhe_pack_batch_dev(e.h, w.key.h, tlwe.ctypes.data, 3, None, 1, d_out.data_ptr(), 1, None)), word="device pointers")
    # ks parameters other than (8, 2): no such key (and no such context) can be made
    with pytest.raises(R.RtfheError) as ei:
        R.packing_keygen(R.Params(n=33, ks_t=4, ks_basebit=4), np.zeros(33, np.int32), np.zeros(N, np.int32), 1)
    assert ei.value.code == R._ffi.ERR_INVALID
    h = C.c_void_p()
    assert e.L.rtfhe_ctx_create(C.byref(R.Params(n=33, ks_t=4, ks_basebit=4)), 0, C.byref(h)) == R._ffi.ERR_INVALID and not h.value
    # rtfhe_lut_update_dev: plain tables and bad ranges
    d_row = torch.zeros((2, 2, N), dtype=torch.int32, device="cuda")
    with e.lut(np.zeros((2, N), np.uint32)) as plain, e.lut_encrypted(np.zeros((2, 2, N), np.uint32)) as enc:
        refused(lambda: plain.update_dev(d_row, 0, 1), word="plain")
        for first, n in ((-1, 1), (0, 3), (2, 1), (1, 2), (0, -1)):
            refused(lambda: enc.update_dev(d_row, first, n), word="outside")
        refused(lambda: e._ck(e.L.rtfhe_lut_update_dev(enc.h, np.zeros(4 * N, np.uint32).ctypes.data, 0, 1, None)), word="device pointer")
        enc.update_dev(d_row, 0, 2)
        enc.update_dev(d_row, 2, 0)
        e.sync()
    # a key of another context; a key and a table that outlive their context
    other = R.Engine(w.rp, 0)
    late = other.packing_key(w.pk)
    late_lut = other.lut_encrypted(np.zeros((1, 2, N), np.uint32))
    try:
        refused(lambda: e.pack_batch(late, tlwe, 3, 1, None), word="another context")
        assert np.array_equal(other.pack_batch(late, tlwe, 3, 1, None), ref)
    finally:
        other.close()
    refused(lambda: e.pack_batch(late, tlwe, 3, 1, None), code=R._ffi.ERR_STATE, word="destroyed")
    assert e.L.rtfhe_lut_update_dev(late_lut.h, d_row.data_ptr(), 0, 1, None) == R._ffi.ERR_STATE
    late.close()                                                    # only frees the handles
    late_lut.close()
    assert np.array_equal(e.pack_batch(w.key, tlwe, 3, 1, None), ref)
    # a key destroyed first: the context goes on
    with e.packing_key(w.pk) as again:
        assert np.array_equal(e.pack_batch(again, tlwe, 3, 1, None), ref)
    assert np.array_equal(e.pack_batch(w.key, tlwe, 3, 1, None), ref)


def test_tree_pbs_example(real_dev):
    """examples/tree_pbs.py on 48 random inputs of a random function"""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("tree_pbs", os.path.join(root, "examples", "tree_pbs.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    rng = np.random.default_rng(0x7EE)
    f = rng.integers(0, 4, (4, 4))
    hi, lo = rng.integers(0, 4, 48), rng.integers(0, 4, 48)
    got, per = ex.run(real_dev.eng, real_dev.key, real_dev.key0, f, hi, lo, seed=0x7EE)
    assert np.array_equal(got, f[hi, lo]) and per > 0
