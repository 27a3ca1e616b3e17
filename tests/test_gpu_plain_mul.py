"""GPU: the exact TRLWE x plain-polynomial product (rtfhe_plain_create, rtfhe_trlwe_mul_plain_batch[_dev]; k_plain_build, k_trlwe_mul_plain).
Every word against the numpy oracle (tests/plain_mul_oracle.py: np.convolve in int64, folded, masked) on rows of random words with the split's
edge words planted -- the arithmetic does not care what a row encrypts --, the largest sums the exactness domain admits, identities, every
backend setting and a two-entry context, meaning with real keys, capture and replay, launch counts and refusals.  Contexts hold no key unless
a test decrypts: n = 40 at N = 1024, n = 24 at N = 2048 as the extract tests use."""
import numpy as np
import pytest

import gpu_kit as gk
import plain_mul_oracle as O
from gpu_kit import CANARY, FILL
from kit import SMALL_N, i32

pytestmark = pytest.mark.gpu

LIMIT = O.L1_PER_N      # K * wmax <= 192 N


class World:
    """per N, built on first use: a context with nothing loaded, a weight set of 8 polynomials at l1 = 24 N each (K = 8 sits exactly on the
    limit), 12 rows with planted edge words, and a memo of oracle words -- computed once, shared, read-only"""

    def __init__(self, R, N):
        self.R, self.N = R, N
        self.rp = R.Params(n=SMALL_N[N], N=N)
        self.eng = R.Engine(self.rp, 0)
        self.w = O.weights(0xA11 + N, N, 8, LIMIT * N // 8)
        self.w.setflags(write=False)
        self.x = O.rows_with_edges(0xB22 + N, N, 12)
        self.x.setflags(write=False)
        self.pp = self.eng.plain_polys(self.w)
        self.memo = {}

    def oracle(self, K, w_idx, x_idx, acc, count):
        return gk.memo(self.memo, (K, w_idx, x_idx, acc, count), lambda: O.mul_plain(self.w, self.x, K, w_idx, x_idx, acc, count))

    def close(self):
        self.pp.close()
        self.eng.close()


@pytest.fixture(scope="module")
def worlds():
    import rustfhe_amd as R
    made = gk.Worlds(lambda N: World(R, N))
    yield made
    made.close()


def _dev(eng, pp, x, count, K=1, w_idx=None, x_idx=None, acc=None, stream=None):
    """the _dev form into a 0x5A-filled buffer (or a copy of acc) with CANARY words behind it, which are checked here; u32[count][2][N]"""
    import torch
    N = x.shape[2]
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream
    d_out = gk.guarded_out(count * 2 * N, init=acc)
    eng.trlwe_mul_plain_batch_dev(pp, gk.to_device(x, np.uint32), x.shape[0], d_out, count, K, gk.to_device(w_idx), gk.to_device(x_idx), acc is not None, st)
    eng.sync(st)
    return gk.read_guarded(d_out, count * 2 * N).reshape(count, 2, N)


# (count, K, w_idx, x_idx, accumulate): ragged workgroups (count 1, 2, 3, 5), K 1, 2, 3, 8, NULL and given indices with duplicates, one x row
# shared by all samples, accumulate off and into a 0x5A-filled / a random out
SHAPES = [
    (1, 1, None, None, None),
    (2, 2, [[0, 7], [7, 7]], [[3, 3], [0, 11]], "fill"),
    (3, 3, None, None, "random"),
    (5, 8, [[(g + k) % 8 for k in range(8)] for g in range(5)], [[(3 * g + 5 * k) % 12 for k in range(8)] for g in range(5)], None),
    (5, 1, [[4], [4], [0], [7], [1]], [[6]] * 5, "random"),
    (1, 8, None, None, "fill"),
    (3, 2, [[1, 2], [3, 4], [5, 6]], None, None),
    (2, 3, None, [[11, 0, 11], [5, 5, 5]], "fill"),
]


@pytest.mark.parametrize("N", [1024, 2048])
@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_every_word_equals_the_oracle(worlds, N, shape):
    """host and _dev forms"""
    w = worlds(N)
    count, K, w_idx, x_idx, kind = SHAPES[shape]
    w_idx, x_idx = (None if w_idx is None else i32(w_idx)), (None if x_idx is None else i32(x_idx))
    acc = gk.acc_rows(kind, count, N)
    want = w.oracle(K, w_idx, x_idx, acc, count)
    got = w.eng.trlwe_mul_plain_batch(w.pp, w.x, K, w_idx, x_idx, acc) if (w_idx is not None or x_idx is not None or acc is not None) else \
        w.eng.trlwe_mul_plain_batch(w.pp, w.x[:count * K], K)
    assert got.shape == (count, 2, N) and got.dtype == np.uint32
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), bad[:5])
    dev = _dev(w.eng, w.pp, w.x, count, K, w_idx, x_idx, acc)
    bad = np.argwhere(dev != want)
    assert bad.size == 0, (len(bad), bad[:5])


@pytest.mark.parametrize("N", [1024, 2048])
@pytest.mark.parametrize("K", [1, 8])
def test_the_largest_sums_of_the_domain(worlds, N, K):
    """weights at the limit K * wmax = 192 N in the four sign patterns against rows of 0x7FFF7FFF / 0x80008000 signed so that every term of
    output coefficients 0, N/2 and N-1 aligns: both halves' sums reach 192 N 2^15 (tests/test_plain_mul_host.py), the most the rounding sees"""
    w = worlds(N)
    ew = O.extreme_weights(N, LIMIT // K)
    rows = O.aligned_rows(ew, N)
    count = rows.shape[0]
    w_idx = np.repeat(np.arange(4, dtype=np.int32), 3)[:, None].repeat(K, axis=1)
    x_idx = np.arange(count, dtype=np.int32)[:, None].repeat(K, axis=1)
    want = O.mul_plain(ew, rows, K, w_idx, x_idx)
    with w.eng.plain_polys(ew) as pp:
        assert pp.wmax * K == LIMIT * N and pp.n == 4
        got = w.eng.trlwe_mul_plain_batch(pp, rows, K, w_idx, x_idx)
        dev = _dev(w.eng, pp, rows, count, K, w_idx, x_idx, gk.acc_rows("random", count, N))
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), bad[:5])
    assert np.array_equal(dev, want + gk.acc_rows("random", count, N))


@pytest.mark.parametrize("N", [1024, 2048])
def test_identities(worlds, N):
    w = worlds(N)
    e, x = w.eng, w.x
    one = np.zeros((5, N), np.int32)
    one[0, 0], one[1, 0], one[2, 1], one[3, N // 2], one[4, N - 1] = 1, -1, 1, 1, 1
    with e.plain_polys(one) as pp:
        rows = x[:5]
        got = e.trlwe_mul_plain_batch(pp, rows, 1, i32([[0], [1], [2], [3], [4]]), None)
    assert np.array_equal(got[0], rows[0]), "w = 1 gives x"
    assert np.array_equal(got[1], (0 - rows[1].astype(np.int64)).astype(np.uint32)), "w = -1 gives -x"
    for g, r in ((2, 1), (3, N // 2), (4, N - 1)):      # w = X^r: the negacyclic rotation
        rot = np.concatenate([(0 - rows[g][:, N - r:].astype(np.int64)).astype(np.uint32), rows[g][:, :N - r]], axis=1)
        assert np.array_equal(got[g], rot), r
    # mul(w1 + w2) = mul(w1) + mul(w2)
    both = np.stack([w.w[0], w.w[1], w.w[0] + w.w[1]])
    with e.plain_polys(both) as pp:
        got = e.trlwe_mul_plain_batch(pp, x[:1], 1, i32([[0], [1], [2]]), i32([[0], [0], [0]]))
    assert np.array_equal(got[2], got[0] + got[1])
    # K = 2 equals two K = 1 calls with accumulate
    first = e.trlwe_mul_plain_batch(w.pp, x, 1, i32([[3], [5]]), i32([[2], [9]]))
    second = e.trlwe_mul_plain_batch(w.pp, x, 1, i32([[4], [5]]), i32([[7], [9]]), acc=first)
    assert np.array_equal(second, e.trlwe_mul_plain_batch(w.pp, x, 2, i32([[3, 4], [5, 5]]), i32([[2, 7], [9, 9]])))


@pytest.mark.parametrize("N", [1024, 2048])
def test_every_backend_and_a_two_entry_context_give_the_same_words(worlds, N):
    w, R = worlds(N), worlds(N).R
    count, K, w_idx, x_idx, kind = SHAPES[3]
    w_idx, x_idx = i32(w_idx), i32(x_idx)
    want = w.oracle(K, w_idx, x_idx, None, count)
    for backend in (R._ffi.BACKEND_FFT64_MIRROR, R._ffi.BACKEND_NTT_EXACT, R._ffi.BACKEND_FFT_SPLIT_EXACT):
        e = R.Engine(w.rp, 0)            # nothing loaded
        try:
            e.set_backend(backend)
            with e.plain_polys(w.w) as pp:
                assert np.array_equal(e.trlwe_mul_plain_batch(pp, w.x, K, w_idx, x_idx), want)
                assert np.array_equal(_dev(e, pp, w.x, count, K, w_idx, x_idx), want)
        finally:
            e.close()
    multi = R.Engine(w.rp, devices=[0, 0])
    try:
        assert multi.device_count() == 2
        with multi.plain_polys(w.w) as pp:
            assert np.array_equal(multi.trlwe_mul_plain_batch(pp, w.x, K, w_idx, x_idx), want)
            assert np.array_equal(_dev(multi, pp, w.x, count, K, w_idx, x_idx), want)
    finally:
        multi.close()


@pytest.mark.parametrize("N", [1024, 2048])
def test_a_plain_set_shares_the_split_fft_backends_table(worlds, N):
    """a context WITH keys on the split-FFT exact backend: the plain set is created first, so the backend's first batch finds the twiddle table
    the set built and must compute with it; gates decrypt, and the product gives the oracle's words before and after"""
    w, R = worlds(N), worlds(N).R
    key0, _, bk, ksk = R.keygen(w.rp, 0x5F7 + N)
    e = gk.engine(R, w.rp, bk, ksk)
    try:
        e.set_backend(R._ffi.BACKEND_FFT_SPLIT_EXACT)
        with e.plain_polys(w.w) as pp:
            want = w.oracle(3, None, None, None, 3)
            assert np.array_equal(e.trlwe_mul_plain_batch(pp, w.x[:9], 3), want)
            a, b = np.array([0, 1, 0, 1], np.uint8), np.array([0, 0, 1, 1], np.uint8)
            out = e.gate_batch(R.NAND, R.encrypt_bits(w.rp, key0, a, 1), R.encrypt_bits(w.rp, key0, b, 2))
            assert np.array_equal(R.decrypt_bits(w.rp, key0, out), 1 - (a & b))
            assert np.array_equal(_dev(e, pp, w.x, 3, 3), want)
    finally:
        e.close()


@pytest.mark.parametrize("N", [1024, 2048])
def test_meaning_dense_layer_with_real_keys(N):
    """d small integers in a row times dense_layer_polys of a random W in [-8, 8], K = 2 (two input rows, two weight polynomials): every dot
    product within 6 sqrt(sum ||w||_2^2) 2^-25 + sum ||w||_1 2^-28 of its value -- the sampler's sigma and its documented +2^-28.7 mean
    (rtfhe_keygen.cpp), scaled by the weights; the product adds nothing"""
    import rustfhe_amd as R
    rp = R.Params(n=SMALL_N[N], N=N)
    _, key1, _, _ = R.keygen(rp, 0xD07 + N, want_bk=False, want_ksk=False)
    rng = np.random.default_rng(N + 7)
    d, unit = 8, 1 << 22
    m = N // d
    W = rng.integers(-8, 9, (2, m, d))
    xs = rng.integers(0, 4, (2, d))
    polys = np.concatenate([R.dense_layer_polys(W[k], d, N)[0] for k in range(2)])
    coef = R.dense_layer_polys(W[0], d, N)[1]
    rows = R.encrypt_lut(rp, key1, R.dense_layer_input(xs, d, N, unit), seed=0xC1 + N)
    e = R.Engine(rp, 0)
    try:
        with e.plain_polys(polys) as pp:
            out = e.trlwe_mul_plain_batch(pp, rows, 2)
    finally:
        e.close()
    assert np.array_equal(out, O.mul_plain(polys, rows, 2))
    phase = R.trlwe_phase(rp, key1, out)[0][coef].astype(np.int64)
    dots = (W[0] @ xs[0] + W[1] @ xs[1]) * unit
    err = ((phase - dots + 2 ** 31) % 2 ** 32 - 2 ** 31) / 2.0 ** 32
    l2, l1 = float(np.sqrt((polys.astype(np.int64) ** 2).sum())), float(np.abs(polys.astype(np.int64)).sum())
    bound = 6 * l2 * 2.0 ** -25 + l1 * 2.0 ** -28
    print("N = %d: largest |error| %.3e, bound %.3e" % (N, np.abs(err).max(), bound))
    assert np.abs(err).max() <= bound, (np.abs(err).max(), bound)


def test_encrypted_dense_layer_example(engine, keys):
    """examples/encrypted_dense_layer.py on the session's engine and key set at a small client count: product -> extraction -> PBS, the
    decrypted flags are the clear ones"""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("encrypted_dense_layer", os.path.join(root, "examples", "encrypted_dense_layer.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    want, got, sums = ex.run(engine, keys.key0, keys.key1, clients=3, threshold=4, seed=0xDE5)
    assert want.shape == (3, ex.M) and 0 < want.sum() < want.size and sums.min() >= 0 and sums.max() <= 7, sums
    assert np.array_equal(got, want), (sums, got, want)


def test_capture_first_thing_on_a_fresh_stream_and_replay(worlds):
    import torch
    N = 1024
    w = worlds(N)
    e = w.eng
    count, K, w_idx, x_idx, _ = SHAPES[3]
    w_idx, x_idx = i32(w_idx), i32(x_idx)
    acc = gk.acc_rows("random", count, N)
    want = w.oracle(K, w_idx, x_idx, acc, count)
    eager = _dev(e, w.pp, w.x, count, K, w_idx, x_idx, acc)
    assert np.array_equal(eager, want)
    s = torch.cuda.Stream()
    d_x, d_wi, d_xi = gk.to_device(w.x, np.uint32), gk.to_device(w_idx, np.int32), gk.to_device(x_idx, np.int32)
    d_out = gk.to_device(acc, np.uint32)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):      # nothing has run on s: the call allocates nothing
            e.trlwe_mul_plain_batch_dev(w.pp, d_x, w.x.shape[0], d_out, count, K, d_wi, d_xi, True, s.cuda_stream)
        for _ in range(2):
            d_out.copy_(gk.to_device(acc, np.uint32))
            g.replay()
            torch.cuda.synchronize()
            assert np.array_equal(d_out.cpu().numpy().view(np.uint32), eager)
    e.sync(s.cuda_stream)


@pytest.mark.parametrize("N", [1024, 2048])
def test_one_launch_per_call(worlds, N):
    import torch
    w = worlds(N)
    st = torch.cuda.current_stream().cuda_stream
    d_x = gk.to_device(w.x, np.uint32)
    for count, K in ((1, 1), (5, 2), (1, 8)):
        d_out = torch.zeros((count, 2, N), dtype=torch.int32, device="cuda")
        w.eng.timer_begin(st)
        w.eng.trlwe_mul_plain_batch_dev(w.pp, d_x, 12, d_out, count, K, None, None, False, st)
        assert w.eng.timer_end(st)[1] == 1
        assert np.array_equal(d_out.cpu().numpy().view(np.uint32), w.oracle(K, None, None, None, count))


def test_refusals_leave_the_output_untouched(worlds):
    import torch
    N = 1024
    w = worlds(N)
    R, e = w.R, w.eng
    d_x = gk.to_device(w.x, np.uint32)
    d_out = torch.full((5, 2, N), FILL, dtype=torch.int32, device="cuda")
    d_both = torch.full((6, 2, N), FILL, dtype=torch.int32, device="cuda")      # rows and output in one allocation
    at_limit = np.full((1, N), LIMIT, np.int32)          # K * wmax = 192 N exactly for K = 1
    over = at_limit.copy()
    over[0, 5] = -(LIMIT + 1)                            # one over
    pp_at, pp_over = e.plain_polys(at_limit), e.plain_polys(over)
    assert pp_at.wmax == LIMIT * N and pp_over.wmax == LIMIT * N + 1
    out_host = np.full((5, 2, N), FILL, np.uint32)
    d_zero2 = gk.to_device([[0, 0]], np.int32)
    e.timer_begin()

    def dev(pp=w.pp, wi=None, x=d_x.data_ptr(), n_x=12, xi=None, K=1, acc=0, out=d_out.data_ptr(), count=3, h=e.h):
        return e.L.rtfhe_trlwe_mul_plain_batch_dev(h, pp.h if pp is not None else None, wi, x, n_x, xi, K, acc, out, count, None)

    def host(pp=w.pp, wi=None, n_x=12, xi=None, K=1, count=3, x=w.x):
        return e.L.rtfhe_trlwe_mul_plain_batch(e.h, pp.h, None if wi is None else wi.ctypes.data, x.ctypes.data, n_x, None if xi is None else xi.ctypes.data, K, 0,
                                               out_host.ctypes.data, count)

    for call, word in ((lambda: dev(K=0), "K = 0"), (lambda: dev(K=9), "K = 9"), (lambda: host(K=0), "K = 0"), (lambda: host(K=9), "K = 9"),
                       (lambda: dev(pp=pp_over), "exactness domain"), (lambda: host(pp=pp_over), "exactness domain"),
                       (lambda: dev(pp=pp_at, K=2, count=1, wi=d_zero2.data_ptr()), "K * wmax = 2 * %d" % (LIMIT * N)),
                       (lambda: host(wi=i32([[0], [8], [1]])), "sample 1: w_idx[0] = 8"), (lambda: host(wi=i32([[0], [1], [-1]])), "sample 2: w_idx[0] = -1"),
                       (lambda: host(xi=i32([[0, 1], [2, 12]]), K=2, count=2), "sample 1: x_idx[1] = 12"),
                       (lambda: host(K=3, count=5), "x_idx NULL: sample 4"), (lambda: dev(K=3, count=5), "x_idx NULL: sample 4"),
                       (lambda: dev(n_x=0), "n_x = 0"), (lambda: dev(count=1 << 31), "count * K"), (lambda: dev(K=8, count=(1 << 31) // 8), "count * K"),
                       (lambda: dev(x=0), "null"), (lambda: dev(out=0), "null"), (lambda: dev(pp=None), "null plain set"),
                       (lambda: dev(x=d_both.data_ptr(), n_x=3, out=d_both[2].data_ptr()), "overlaps"),
                       (lambda: dev(x=d_both[2].data_ptr(), n_x=3, out=d_both.data_ptr()), "overlaps"),
                       (lambda: dev(x=d_both[3].data_ptr(), n_x=3, out=d_both[3].data_ptr() - 4), "overlaps"),
                       (lambda: dev(x=w.x.ctypes.data), "device pointers")):
        with pytest.raises(R.RtfheError) as ei:
            e._ck(call())
        assert ei.value.code == R._ffi.ERR_INVALID and word in str(ei.value), (word, str(ei.value))
    # w_idx NULL needs n_w >= K: a one-polynomial set at K = 2
    with e.plain_polys(w.w[:1]) as pp1:
        for call in (lambda: dev(pp=pp1, K=2, count=1), lambda: host(pp=pp1, K=2, count=1)):
            with pytest.raises(R.RtfheError) as ei:
                e._ck(call())
            assert ei.value.code == R._ffi.ERR_INVALID and "w_idx NULL" in str(ei.value)
    assert e.L.rtfhe_trlwe_mul_plain_batch_dev(None, w.pp.h, None, d_x.data_ptr(), 12, None, 1, 0, d_out.data_ptr(), 3, None) == R._ffi.ERR_INVALID      # null context
    assert dev(count=0) == 0 and host(count=0) == 0
    assert e.timer_end()[1] == 0, "the checks come before any launch"
    e.sync()
    assert (d_out.cpu().numpy().view(np.uint32) == FILL).all() and (d_both.cpu().numpy().view(np.uint32) == FILL).all() and (out_host == FILL).all()
    # accepted exactly at the limit; d_out right behind the rows does not overlap them
    want = O.mul_plain(at_limit, w.x[:3], 1, i32([[0]] * 3))
    assert np.array_equal(e.trlwe_mul_plain_batch(pp_at, w.x[:3], 1, i32([[0]] * 3), None), want)
    d_both[:3].copy_(gk.to_device(w.x[:3], np.uint32))
    e.trlwe_mul_plain_batch_dev(pp_at, d_both[:3], 3, d_both[3:], 3, 1, gk.to_device([[0]] * 3, np.int32))
    e.sync()
    assert np.array_equal(d_both[3:].cpu().numpy().view(np.uint32), want)
    pp_at.close()
    pp_over.close()
    # a set of another context, and a set whose context is gone
    other = R.Engine(w.rp, 0)
    pp_other = other.plain_polys(w.w[:1])
    with pytest.raises(R.RtfheError) as ei:
        e._ck(dev(pp=pp_other))
    assert ei.value.code == R._ffi.ERR_INVALID and "another context" in str(ei.value)
    other.close()
    rc = e.L.rtfhe_trlwe_mul_plain_batch_dev(e.h, pp_other.h, None, d_x.data_ptr(), 12, None, 1, 0, d_out.data_ptr(), 3, None)
    assert rc == R._ffi.ERR_STATE and b"destroyed" in e.L.rtfhe_last_error(e.h)
    pp_other.close()            # only frees the handle
    e.sync()
    assert (d_out.cpu().numpy().view(np.uint32) == FILL).all()
    import ctypes as C
    h = C.c_void_p()
    assert e.L.rtfhe_plain_create(e.h, w.w.ctypes.data, 0, C.byref(h)) == R._ffi.ERR_INVALID and not h.value and b"n_w = 0" in e.L.rtfhe_last_error(e.h)
    assert e.L.rtfhe_plain_create(e.h, None, 1, C.byref(h)) == R._ffi.ERR_INVALID and not h.value


@pytest.mark.parametrize("N", [1024, 2048])
def test_a_bad_device_index_skips_its_sample_and_sync_reports_once(worlds, N):
    w, R = worlds(N), worlds(N).R
    count, K = 5, 2
    w_idx = i32([[0, 1], [2, 8], [3, 4], [5, 6], [7, 0]])            # sample 1: a weight index out of range
    x_idx = i32([[0, 1], [2, 3], [4, 5], [6, 12], [8, 9]])           # sample 3: a row index out of range
    ok_w, ok_x = w_idx.copy(), x_idx.copy()
    ok_w[1, 1], ok_x[3, 1] = 0, 0
    want = w.oracle(K, ok_w, ok_x, None, count)
    import torch
    st = torch.cuda.current_stream().cuda_stream
    d_out = torch.full((count * 2 * N + CANARY,), FILL, dtype=torch.int32, device="cuda")
    w.eng.trlwe_mul_plain_batch_dev(w.pp, gk.to_device(w.x, np.uint32), 12, d_out, count, K, gk.to_device(w_idx, np.int32), gk.to_device(x_idx, np.int32), False, st)
    with pytest.raises(R.RtfheError) as ei:
        w.eng.sync(st)
    assert ei.value.code == R._ffi.ERR_INVALID
    w.eng.sync(st)              # reported once
    out = d_out.cpu().numpy().view(np.uint32)
    assert (out[count * 2 * N:] == FILL).all()
    out = out[:count * 2 * N].reshape(count, 2, N)
    assert (out[[1, 3]] == FILL).all(), "a skipped sample's row was written"
    assert np.array_equal(out[[0, 2, 4]], want[[0, 2, 4]])
