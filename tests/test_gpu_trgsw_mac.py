"""GPU: the TRLWE x TRGSW multiply-accumulate (rtfhe_trlwe_mul_trgsw_batch[_dev]; k_trlwe_mul_trgsw).  Every word against the restatement
(tests/trgsw_mac_oracle.py: the oracle's own blocks with the running sums carried over the K terms) in both leveled decomposition modes, on
real TRGSW encryptions of ternary polynomials and rows of random words with the decomposition's edge words planted; anchors (the stage-level
external product, a zero selector, the trivial TRGSW of 1); the largest sums K = 8 admits, which the narrow conversion gets wrong; meaning with
real keys and the example; capture and replay, launch counts, refusals, skipped samples, the exact backends, a two-entry context, a destroyed
context.  Contexts hold no key unless a test needs one: n = 40 (n = 24 at N = 2048, as the extract tests use)."""
import importlib.util
import os

import numpy as np
import pytest

import gpu_kit as gk
import round_oracle as ro
import trgsw_mac_oracle as O
from gpu_kit import CANARY, FILL
from kit import SMALL_N, i32

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_SEL, N_X = 16, 12


class World:
    """per N, built on first use: a context with nothing loaded, 16 TRGSW encryptions of ternary polynomials as its selector set (the last one
    replaced by the zero TRGSW), 12 rows with planted edge words, the oracle's plan and spectra, and a memo of oracle words -- computed once,
    shared, read-only"""

    def __init__(self, R, orc, N):
        self.R, self.orc, self.N = R, orc, N
        self.rp = R.Params(n=SMALL_N[N], N=N)
        self.p = orc.Params(n=SMALL_N[N], N=N)
        self.plan = orc.Plan(N)
        _, self.key1, _, _ = R.keygen(self.rp, 0x7AC + N, want_bk=False, want_ksk=False)
        rng = np.random.default_rng(0x7AD + N)
        self.mu = rng.integers(-1, 2, (N_SEL, N)).astype(np.int32)
        self.mu[N_SEL - 1] = 0
        self.sel_t = R.encrypt_trgsw_polys(self.rp, self.key1, self.mu, seed=0x7AE + N)
        self.sel_t[N_SEL - 1] = 0                                     # the zero TRGSW: all words 0
        self.sel_t.setflags(write=False)
        self.sel_f = O.spectra(self.p, self.plan, self.sel_t)
        self.x = O.rows_with_edges(0xB23 + N, N, N_X)
        self.x.setflags(write=False)
        self.eng = R.Engine(self.rp, 0)
        self.sel = self.eng.selectors(self.sel_t)
        self.memo = {}

    def oracle(self, mode, K, s_idx, x_idx, acc, count):
        nat = np.arange(count * K).reshape(count, K)
        return gk.memo(self.memo, (mode, K, s_idx, x_idx, acc, count),
                       lambda: O.mac(self.p, self.plan, self.sel_f, nat if s_idx is None else s_idx, self.x, nat if x_idx is None else x_idx, acc, mode))

    def mode(self, mode):
        self.eng.set_leveled_decomposition(self.R._ffi.DECOMP_ROUNDED if mode == O.ROUNDED else self.R._ffi.DECOMP_REFERENCE)

    def close(self):
        self.sel.close()
        self.eng.close()


@pytest.fixture(scope="module")
def worlds(orc):
    import rustfhe_amd as R
    made = gk.Worlds(lambda N: World(R, orc, N))

    def get(N):
        w = made(N)
        w.mode(O.REFERENCE)
        return w
    yield get
    made.close()


def _dev(eng, sel, x, count, K=1, s_idx=None, x_idx=None, acc=None, stream=None):
    """the _dev form into a 0x5A-filled buffer (or a copy of acc) with CANARY words behind it, which are checked here; u32[count][2][N]"""
    import torch
    N = x.shape[2]
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream
    d_out = gk.guarded_out(count * 2 * N, init=acc)
    eng.trlwe_mul_trgsw_batch_dev(sel, gk.to_device(x, np.uint32), x.shape[0], d_out, count, K, gk.to_device(s_idx), gk.to_device(x_idx), acc is not None, st)
    eng.sync(st)
    return gk.read_guarded(d_out, count * 2 * N).reshape(count, 2, N)


# (count, K, s_idx, x_idx, accumulate): ragged four-wave workgroups (count 1, 2, 3, 5), K 1, 2, 3, 8, NULL and given indices with duplicates,
# one selector shared by all samples, one row shared by all samples, accumulate off and into a 0x5A-filled / a random out
SHAPES = [
    (1, 1, None, None, None),
    (2, 2, [[0, 14], [14, 14]], [[3, 3], [0, 11]], "fill"),
    (3, 3, None, None, "random"),
    (5, 8, [[(g + 3 * k) % N_SEL for k in range(8)] for g in range(5)], [[(3 * g + 5 * k) % N_X for k in range(8)] for g in range(5)], None),
    (5, 1, [[4]] * 5, [[6]] * 5, "random"),
    (1, 8, None, None, "fill"),
    (3, 2, [[1, 2], [3, 4], [5, 6]], None, None),
    (2, 3, None, [[11, 0, 11], [5, 5, 5]], "fill"),
]


@pytest.mark.parametrize("N", [1024, 2048])
@pytest.mark.parametrize("mode", [O.REFERENCE, O.ROUNDED])
@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_every_word_equals_the_restatement(worlds, N, mode, shape):
    """host and _dev forms"""
    w = worlds(N)
    w.mode(mode)
    count, K, s_idx, x_idx, kind = SHAPES[shape]
    s_idx, x_idx = (None if s_idx is None else i32(s_idx)), (None if x_idx is None else i32(x_idx))
    acc = gk.acc_rows(kind, count, N)
    want = w.oracle(mode, K, s_idx, x_idx, acc, count)
    got = w.eng.trlwe_mul_trgsw_batch(w.sel, w.x, K, s_idx, x_idx, acc) if (s_idx is not None or x_idx is not None or acc is not None) else \
        w.eng.trlwe_mul_trgsw_batch(w.sel, w.x[:count * K], K)
    assert got.shape == (count, 2, N) and got.dtype == np.uint32
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), bad[:5])
    dev = _dev(w.eng, w.sel, w.x, count, K, s_idx, x_idx, acc)
    bad = np.argwhere(dev != want)
    assert bad.size == 0, (len(bad), bad[:5])


@pytest.mark.parametrize("N", [1024, 2048])
def test_anchors(worlds, N):
    """K = 1 is rtfhe_external_product_batch on the same TRGSW and row, word for word, in both modes (the selector words loaded as a
    bootstrapping key); K = 2 with a zero second selector is K = 1; the trivial TRGSW of the constant 1 -- the gadget rows only -- returns each
    row within the decomposition's recomposition error e = sum_j digit_j 2^(32 - 6 (j+1)) - x: rounded mode rounds to nearest at 2^14,
    e in [1 - 2^13, 2^13]; the reference mask adds a whole unit 2^14 and its xor flips the last field's unit bit, e in [1 - 2^14, 2^15]; one
    more unit of 2^-32 either way for the truncation toward zero of a sum that is an integer up to the transforms' rounding."""
    w, R = worlds(N), worlds(N).R
    bk = np.zeros((w.rp.n, 2, 2 * w.rp.l, N), np.uint32)
    bk[:N_SEL] = w.sel_t
    keyed = R.Engine(w.rp, 0)
    one = np.zeros((1, 2, 2 * w.rp.l, N), np.uint32)
    for j in range(w.rp.l):
        one[0, 0, j, 0] = one[0, 1, w.rp.l + j, 0] = 1 << (32 - (j + 1) * w.rp.bgbit)
    try:
        keyed.load_bk_torus(bk)
        idx = i32([3, 0, 15, 7, 7])
        rows = w.x[[2, 5, 5, 0, 11]]
        with w.eng.selectors(one) as sel_one:
            for mode, lo, hi in ((O.REFERENCE, 1 - 2 ** 14, 2 ** 15), (O.ROUNDED, 1 - 2 ** 13, 2 ** 13)):
                w.mode(mode)
                keyed.set_leveled_decomposition(R._ffi.DECOMP_ROUNDED if mode == O.ROUNDED else R._ffi.DECOMP_REFERENCE)
                stage = keyed.external_product_batch(idx, rows)
                got = w.eng.trlwe_mul_trgsw_batch(w.sel, rows, 1, idx[:, None], None)
                assert np.array_equal(got, stage), mode
                assert np.array_equal(_dev(w.eng, w.sel, rows, 5, 1, idx[:, None], None), stage), mode
                with_zero = w.eng.trlwe_mul_trgsw_batch(w.sel, rows, 2, np.stack([idx, np.full(5, N_SEL - 1, np.int32)], axis=1), i32([[g, (g + 1) % 5] for g in range(5)]))
                assert np.array_equal(with_zero, got), mode
                back = w.eng.trlwe_mul_trgsw_batch(sel_one, w.x[:5], 1, i32([[0]] * 5), None)
                e = (back - w.x[:5]).view(np.int32).astype(np.int64)
                assert lo - 1 <= e.min() and e.max() <= hi + 1, (mode, e.min(), e.max())
                assert e.min() < 0 < e.max()
    finally:
        keyed.close()


@pytest.mark.parametrize("N", [1024, 2048])
@pytest.mark.parametrize("mode", [O.REFERENCE, O.ROUNDED])
def test_the_largest_sums_need_the_wide_conversion(worlds, N, mode):
    """every selector word 0x80000000, every digit of every row -Bg/2 (round_oracle.digits), K = 8: the aligned coefficients reach
    K * 2l * N * (Bg/2) * 2^31 = 2^51.6 (N = 1024) / 2^52.6 (N = 2048), where trunc_to_torus's magic-add form is no longer exact
    (tests/test_trgsw_mac_host.py shows it gives other words on these inputs); every word equals the restatement"""
    w = worlds(N)
    w.mode(mode)
    ma, mx = ro.constants(w.rp.l, w.rp.bgbit, mode)
    rows = O.extreme_rows(N, 2, mode)
    assert (ro.digits(rows[0, 0], w.rp.l, w.rp.bgbit, ma, mx) == -32).all()
    sel_t = np.full((2, 2, 2 * w.rp.l, N), 0x80000000, np.uint32)
    s_idx, x_idx = i32([[0, 1] * 4, [1] * 8, [0] * 8]), i32([[0] * 8, [0, 1] * 4, [1] * 8])
    want = O.mac(w.p, w.plan, O.spectra(w.p, w.plan, sel_t), s_idx, rows, x_idx, None, mode)
    with w.eng.selectors(sel_t) as sel:
        got = w.eng.trlwe_mul_trgsw_batch(sel, rows, 8, s_idx, x_idx)
        dev = _dev(w.eng, sel, rows, 3, 8, s_idx, x_idx, gk.acc_rows("random", 3, N))
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), bad[:5])
    assert np.array_equal(dev, want + gk.acc_rows("random", 3, N))


def test_meaning_with_real_keys(worlds, orc):
    """trgsw_mac_oracle.meaning_world on the device, rounded mode: K = 4 encrypted ternary polynomials times four fresh rows per sample; the
    device's words are the restatement's, so every coefficient of the phase is sum_k mu_k * m_k within the bound that
    tests/test_trgsw_mac_host.py holds the restatement to"""
    w, R = worlds(1024), worlds(1024).R
    m = O.meaning_world(R)
    assert (m.rp.n, m.rp.N) == (w.rp.n, w.rp.N)
    w.mode(O.ROUNDED)
    with w.eng.selectors(m.sel_t) as sel:
        got = w.eng.trlwe_mul_trgsw_batch(sel, m.rows, m.K)
    ph = R.trlwe_phase(m.rp, m.key1, got)
    for g in range(m.COUNT):
        err = float(np.abs(O.torus_err(ph[g], m.want[g])).max())
        print("sample %d: largest |error| %.3e, bound %.3e" % (g, err, m.bound[g]))
        assert err <= m.bound[g], (g, err, m.bound[g])


def test_private_dense_layer_example(engine, keys):
    """examples/private_dense_layer.py on the session's engine and key set at three clients: product (TRGSW-encrypted weights, the bias
    through accumulate) -> extraction -> PBS, the decrypted flags are the clear ones"""
    spec = importlib.util.spec_from_file_location("private_dense_layer", os.path.join(ROOT, "examples", "private_dense_layer.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    before = (engine.decomposition(), engine.leveled_decomposition())
    want, got, sums = ex.run(engine, keys.key0, keys.key1, clients=3, threshold=4, seed=0xDE6)
    assert (engine.decomposition(), engine.leveled_decomposition()) == before
    assert want.shape == (3, ex.M) and 0 < want.sum() < want.size and sums.min() >= 0 and sums.max() <= 7, sums
    assert np.array_equal(got, want), (sums, got, want)


def test_capture_first_thing_on_a_fresh_stream_and_replay():
    """a fresh context whose first product call sits in a capture, on a stream nothing has run on"""
    import torch
    import rustfhe_amd as R
    import orc as orc_mod
    N = 1024
    rp = R.Params(n=SMALL_N[N], N=N)
    p, plan = orc_mod.Params(n=SMALL_N[N], N=N), orc_mod.Plan(N)
    _, key1, _, _ = R.keygen(rp, 0x7C1, want_bk=False, want_ksk=False)
    sel_t = R.encrypt_trgsw_polys(rp, key1, np.random.default_rng(3).integers(-1, 2, (4, N)).astype(np.int32), seed=0x7C2)
    x = O.rows_with_edges(0x7C3, N, 6)
    count, K = 5, 2
    s_idx, x_idx = i32([[0, 1], [2, 3], [3, 3], [1, 0], [2, 2]]), i32([[0, 1], [2, 3], [4, 5], [5, 5], [0, 3]])
    acc = gk.acc_rows("random", count, N)
    want = O.mac(p, plan, O.spectra(p, plan, sel_t), s_idx, x, x_idx, acc, O.REFERENCE)
    e = R.Engine(rp, 0)
    try:
        with e.selectors(sel_t) as sel:
            s = torch.cuda.Stream()
            d_x, d_si, d_xi = gk.to_device(x, np.uint32), gk.to_device(s_idx, np.int32), gk.to_device(x_idx, np.int32)
            d_out = gk.to_device(acc, np.uint32)
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=s):      # nothing has run on s, and no product on this context: the call allocates nothing
                    e.trlwe_mul_trgsw_batch_dev(sel, d_x, x.shape[0], d_out, count, K, d_si, d_xi, True, s.cuda_stream)
                for _ in range(2):
                    d_out.copy_(gk.to_device(acc, np.uint32))
                    g.replay()
                    torch.cuda.synchronize()
                    assert np.array_equal(d_out.cpu().numpy().view(np.uint32), want)
            e.sync(s.cuda_stream)
            del g
    finally:
        e.close()


@pytest.mark.parametrize("N", [1024, 2048])
def test_one_launch_per_call(worlds, N):
    import torch
    w = worlds(N)
    st = torch.cuda.current_stream().cuda_stream
    d_x = gk.to_device(w.x, np.uint32)
    for count, K in ((1, 1), (5, 2), (1, 8)):
        d_out = torch.zeros((count, 2, N), dtype=torch.int32, device="cuda")
        w.eng.timer_begin(st)
        w.eng.trlwe_mul_trgsw_batch_dev(w.sel, d_x, N_X, d_out, count, K, None, None, False, st)
        assert w.eng.timer_end(st)[1] == 1
        assert np.array_equal(d_out.cpu().numpy().view(np.uint32), w.oracle(O.REFERENCE, K, None, None, None, count))


def test_refusals_leave_the_output_untouched(worlds):
    import torch
    N = 1024
    w = worlds(N)
    R, e = w.R, w.eng
    d_x = gk.to_device(w.x, np.uint32)
    d_out = torch.full((5, 2, N), FILL, dtype=torch.int32, device="cuda")
    d_both = torch.full((6, 2, N), FILL, dtype=torch.int32, device="cuda")      # rows and output in one allocation
    out_host = np.full((5, 2, N), FILL, np.uint32)
    e.timer_begin()

    def dev(sel=w.sel, si=None, x=d_x.data_ptr(), n_x=N_X, xi=None, K=1, acc=0, out=d_out.data_ptr(), count=3, h=e.h):
        return e.L.rtfhe_trlwe_mul_trgsw_batch_dev(h, sel.h if sel is not None else None, si, x, n_x, xi, K, acc, out, count, None)

    def host(sel=w.sel, si=None, n_x=N_X, xi=None, K=1, count=3, x=w.x):
        return e.L.rtfhe_trlwe_mul_trgsw_batch(e.h, sel.h, None if si is None else si.ctypes.data, x.ctypes.data, n_x, None if xi is None else xi.ctypes.data, K, 0,
                                               out_host.ctypes.data, count)

    for call, word in ((lambda: dev(K=0), "K = 0"), (lambda: dev(K=9), "K = 9"), (lambda: host(K=0), "K = 0"), (lambda: host(K=9), "K = 9"),
                       (lambda: host(si=i32([[0], [16], [1]])), "sample 1: s_idx[0] = 16"), (lambda: host(si=i32([[0], [1], [-1]])), "sample 2: s_idx[0] = -1"),
                       (lambda: host(xi=i32([[0, 1], [2, 12]]), K=2, count=2), "sample 1: x_idx[1] = 12"),
                       (lambda: host(K=3, count=5), "x_idx NULL: sample 4"), (lambda: dev(K=3, count=5), "x_idx NULL: sample 4"),
                       (lambda: host(K=6, count=3, xi=i32([[0] * 6] * 3)), "s_idx NULL: sample 2"), (lambda: dev(K=8, count=3, xi=d_x.data_ptr()), "s_idx NULL: sample 2"),
                       (lambda: dev(n_x=0), "n_x = 0"), (lambda: dev(count=1 << 31), "count * K"), (lambda: dev(K=8, count=(1 << 31) // 8), "count * K"),
                       (lambda: dev(x=0), "null"), (lambda: dev(out=0), "null"), (lambda: dev(sel=None), "null selector set"),
                       (lambda: dev(x=d_both.data_ptr(), n_x=3, out=d_both[2].data_ptr()), "overlaps"),
                       (lambda: dev(x=d_both[2].data_ptr(), n_x=3, out=d_both.data_ptr()), "overlaps"),
                       (lambda: dev(x=d_both[3].data_ptr(), n_x=3, out=d_both[3].data_ptr() - 4), "overlaps"),
                       (lambda: dev(x=w.x.ctypes.data), "device pointers")):
        with pytest.raises(R.RtfheError) as ei:
            e._ck(call())
        assert ei.value.code == R._ffi.ERR_INVALID and word in str(ei.value), (word, str(ei.value))
    assert e.L.rtfhe_trlwe_mul_trgsw_batch_dev(None, w.sel.h, None, d_x.data_ptr(), N_X, None, 1, 0, d_out.data_ptr(), 3, None) == R._ffi.ERR_INVALID      # null context
    assert dev(count=0) == 0 and host(count=0) == 0
    assert e.timer_end()[1] == 0, "the checks come before any launch"
    e.sync()
    assert (d_out.cpu().numpy().view(np.uint32) == FILL).all() and (d_both.cpu().numpy().view(np.uint32) == FILL).all() and (out_host == FILL).all()
    # accepted exactly at each limit: K = 8 with NULL indices at n_sel = count * K = 16 and n_x = 12 >= 8; d_out right behind the rows does not
    # overlap them
    assert np.array_equal(e.trlwe_mul_trgsw_batch(w.sel, w.x, 8, None, i32([[0, 1, 2, 3, 4, 5, 6, 7], [4, 5, 6, 7, 8, 9, 10, 11]])),
                          w.oracle(O.REFERENCE, 8, None, i32([[0, 1, 2, 3, 4, 5, 6, 7], [4, 5, 6, 7, 8, 9, 10, 11]]), None, 2))
    assert np.array_equal(e.trlwe_mul_trgsw_batch(w.sel, w.x, 4, i32([[0, 1, 2, 3]] * 3), None), w.oracle(O.REFERENCE, 4, i32([[0, 1, 2, 3]] * 3), None, None, 3))
    d_both[:3].copy_(gk.to_device(w.x[:3], np.uint32))
    e.trlwe_mul_trgsw_batch_dev(w.sel, d_both[:3], 3, d_both[3:], 3, 1)
    e.sync()
    assert np.array_equal(d_both[3:].cpu().numpy().view(np.uint32), w.oracle(O.REFERENCE, 1, None, None, None, 3))
    # a set of another context, and a set whose context is gone
    other = R.Engine(w.rp, 0)
    sel_other = other.selectors(w.sel_t[:1])
    with pytest.raises(R.RtfheError) as ei:
        e._ck(dev(sel=sel_other))
    assert ei.value.code == R._ffi.ERR_INVALID and "another context" in str(ei.value)
    other.close()
    rc = e.L.rtfhe_trlwe_mul_trgsw_batch_dev(e.h, sel_other.h, None, d_x.data_ptr(), N_X, None, 1, 0, d_out.data_ptr(), 3, None)
    assert rc == R._ffi.ERR_STATE and b"destroyed" in e.L.rtfhe_last_error(e.h)
    sel_other.close()            # rtfhe_trgsw_destroy still frees the handle
    e.sync()
    assert (d_out.cpu().numpy().view(np.uint32) == FILL).all()


def test_a_destroyed_context_gives_err_state():
    """the context destroyed under a live selector set: both forms, called on another live context, return RTFHE_ERR_STATE and touch nothing,
    and rtfhe_trgsw_destroy still frees the handle"""
    import torch
    import rustfhe_amd as R
    N = 1024
    rp = R.Params(n=SMALL_N[N], N=N)
    e = R.Engine(rp, 0)
    sel = e.selectors(np.zeros((1, 2, 2 * rp.l, N), np.uint32))
    x = np.zeros((1, 2, N), np.uint32)
    out = np.full((1, 2, N), FILL, np.uint32)
    d_x = gk.to_device(x, np.uint32)
    d_out = torch.full((1, 2, N), FILL, dtype=torch.int32, device="cuda")
    e.close()
    live = R.Engine(rp, 0)
    try:
        L = live.L
        assert L.rtfhe_trlwe_mul_trgsw_batch(live.h, sel.h, None, x.ctypes.data, 1, None, 1, 0, out.ctypes.data, 1) == R._ffi.ERR_STATE
        assert b"destroyed" in L.rtfhe_last_error(live.h)
        assert L.rtfhe_trlwe_mul_trgsw_batch_dev(live.h, sel.h, None, d_x.data_ptr(), 1, None, 1, 0, d_out.data_ptr(), 1, None) == R._ffi.ERR_STATE
        live.sync()
    finally:
        live.close()
    sel.close()
    torch.cuda.synchronize()
    assert (out == FILL).all() and (d_out.cpu().numpy().view(np.uint32) == FILL).all()


@pytest.mark.parametrize("N", [1024, 2048])
def test_a_bad_device_index_skips_its_sample_and_sync_reports_once(worlds, N):
    w, R = worlds(N), worlds(N).R
    count, K = 5, 2
    s_idx = i32([[0, 1], [2, 16], [3, 4], [5, 6], [7, 0]])           # sample 1: a selector index out of range
    x_idx = i32([[0, 1], [2, 3], [4, 5], [6, 12], [8, 9]])           # sample 3: a row index out of range
    ok_s, ok_x = s_idx.copy(), x_idx.copy()
    ok_s[1, 1], ok_x[3, 1] = 0, 0
    want = w.oracle(O.REFERENCE, K, ok_s, ok_x, None, count)
    import torch
    st = torch.cuda.current_stream().cuda_stream
    d_out = torch.full((count * 2 * N + CANARY,), FILL, dtype=torch.int32, device="cuda")
    w.eng.trlwe_mul_trgsw_batch_dev(w.sel, gk.to_device(w.x, np.uint32), N_X, d_out, count, K, gk.to_device(s_idx, np.int32), gk.to_device(x_idx, np.int32), False, st)
    with pytest.raises(R.RtfheError) as ei:
        w.eng.sync(st)
    assert ei.value.code == R._ffi.ERR_INVALID
    w.eng.sync(st)              # reported once
    out = d_out.cpu().numpy().view(np.uint32)
    assert (out[count * 2 * N:] == FILL).all()
    out = out[:count * 2 * N].reshape(count, 2, N)
    assert (out[[1, 3]] == FILL).all(), "a skipped sample's row was written"
    assert np.array_equal(out[[0, 2, 4]], want[[0, 2, 4]])


@pytest.mark.parametrize("N", [1024, 2048])
def test_exact_backends_refuse_and_a_two_entry_context_runs(worlds, N):
    w, R = worlds(N), worlds(N).R
    count, K, s_idx, x_idx, _ = SHAPES[3]
    s_idx, x_idx = i32(s_idx), i32(x_idx)
    want = w.oracle(O.REFERENCE, K, s_idx, x_idx, None, count)
    e = R.Engine(w.rp, 0)            # nothing loaded
    try:
        with e.selectors(w.sel_t) as sel:
            for backend in (R._ffi.BACKEND_NTT_EXACT, R._ffi.BACKEND_FFT_SPLIT_EXACT):
                e.set_backend(backend)
                for call in (lambda: e.trlwe_mul_trgsw_batch(sel, w.x, K, s_idx, x_idx), lambda: _dev(e, sel, w.x, count, K, s_idx, x_idx)):
                    with pytest.raises(R.RtfheError) as ei:
                        call()
                    assert ei.value.code == R._ffi.ERR_INVALID and "mirror" in str(ei.value)
            e.set_backend(R._ffi.BACKEND_FFT64_MIRROR)
            assert np.array_equal(e.trlwe_mul_trgsw_batch(sel, w.x, K, s_idx, x_idx), want)      # the context works afterwards
    finally:
        e.close()
    multi = R.Engine(w.rp, devices=[0, 0])
    try:
        assert multi.device_count() == 2
        with multi.selectors(w.sel_t) as sel:
            assert np.array_equal(multi.trlwe_mul_trgsw_batch(sel, w.x, K, s_idx, x_idx), want)
            assert np.array_equal(_dev(multi, sel, w.x, count, K, s_idx, x_idx), want)
    finally:
        multi.close()
