"""GPU: lvl0 dense layers (rtfhe_dense_create, rtfhe_tlwe_dense_batch[_dev]; k_dense_build, k_tlwe_dense).  Every word against the numpy oracle
(tests/dense_oracle.py: W @ x in int64, masked) on rows of random words with the byte limbs' edge words planted -- the arithmetic does not care
what a row encrypts --: ragged shapes, the largest accumulator sums the bound admits, both launch paths as the host rule names them, bias and
accumulate, every backend setting, meaning with real keys through a sign bootstrap, agreement with a LUT circuit's weighted sums, capture and
replay, launch counts, refusals and the handle's lifetime.  Contexts hold no key unless a test bootstraps."""
import ctypes as C

import numpy as np
import pytest

import dense_oracle as D
import gpu_kit as gk
import lut_circuit_kit as lk
from gpu_kit import FILL
from kit import random_words

pytestmark = pytest.mark.gpu

N = 1024


class Shape(C.Structure):
    """rtfhe_dense_shape (rustfhe_amd/csrc/rtfhe_dense_plan.h)"""
    _fields_ = [(k, C.c_int32) for k in ("tiles", "groups", "cwgs", "ksteps", "slices", "steps")]


def slices_of(R, n, O, I, count):
    """how many slices the host rule cuts I into for this call on this device: 1 = plain stores, more = the atomic path"""
    L = R.load()
    L.rtfhe_dense_launch_shape.restype = None
    L.rtfhe_dense_launch_shape.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_size_t, C.c_int32, C.POINTER(Shape)]
    s = Shape()
    L.rtfhe_dense_launch_shape(n, O, I, count, gk.cus(), C.byref(s))
    return s.slices


@pytest.fixture(scope="module")
def worlds():
    """a context with nothing loaded per mask length n, built on first use"""
    import rustfhe_amd as R
    made = gk.Worlds(lambda n, ring=N: R.Engine(R.Params(n=n, N=ring), 0))
    yield made
    made.close()


def acc_words(kind, count, O, words):
    if kind is None:
        return None
    if kind == "fill":
        return np.full((count, O, words), FILL, np.uint32)
    return random_words(np.random.default_rng(count * O + words), (count, O, words))


def run_dev(eng, dense, x, bias=None, acc=None, stream=None):
    """the _dev form into a 0x5A-filled buffer (or a copy of acc) with canary words behind it, which are checked here; u32[count][O][n+1]"""
    import torch
    count, words = x.shape[0], x.shape[2]
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream
    d_out = gk.guarded_out(count * dense.O * words, init=acc)
    eng.tlwe_dense_batch_dev(dense, gk.to_device(x, np.uint32), d_out, count, bias, acc is not None, st)
    eng.sync(st)
    return gk.read_guarded(d_out, count * dense.O * words).reshape(count, dense.O, words)


def check_both_forms(eng, W, x, bias=None, acc=None):
    want = D.dense(W, x, bias, acc)
    with eng.dense(W) as dense:
        assert (dense.O, dense.I) == W.shape
        got = eng.tlwe_dense_batch(dense, x, bias, acc)
        dev = run_dev(eng, dense, x, bias, acc)
    assert got.shape == want.shape and got.dtype == np.uint32
    for name, words in (("host", got), ("dev", dev)):
        bad = np.argwhere(words != want)
        assert bad.size == 0, (name, len(bad), bad[:5], [hex(int(words[tuple(b)])) for b in bad[:3]], [hex(int(want[tuple(b)])) for b in bad[:3]])
    return want


# (n, I, O, count): n + 1 = 2, 16, 17, 41, 636, 768 (odd row strides, below / at / above a word tile); I below, at and above a K-step of 64 and
# several K-steps; O below, at and above an output tile of 16 and more than two tiles; count 1, 2, 3, 5.  Every value appears at least once.
SHAPES = [(1, 1, 1, 1), (767, 65, 33, 5), (1, 3, 15, 2), (15, 63, 16, 3), (15, 64, 17, 1), (16, 65, 1, 5), (16, 200, 33, 2), (40, 1, 33, 3),
          (40, 3, 16, 5), (40, 63, 17, 2), (40, 200, 15, 1), (635, 64, 1, 2), (635, 3, 17, 3), (635, 200, 33, 1), (767, 1, 15, 2), (767, 63, 1, 1),
          (1, 200, 16, 5), (15, 65, 15, 2), (16, 64, 16, 3), (635, 65, 16, 5)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d-I%d-O%d-c%d" % s)
def test_ragged_shapes_equal_the_oracle(worlds, shape):
    """host and _dev forms; bias and the accumulate kinds rotate over the shapes"""
    n, I, O, count = shape
    k = SHAPES.index(shape)
    W = D.weights(0xD0 + k, O, I)
    x = D.rows_with_edges(0xE0 + k, count, I, n + 1)
    bias = random_words(np.random.default_rng(k), O) if k % 2 == 0 else None
    acc = acc_words((None, "fill", "random")[k % 3], count, O, n + 1)
    check_both_forms(worlds(n), W, x, bias, acc)


def test_the_call_works_at_n2048(worlds):
    import rustfhe_amd as R
    e = R.Engine(R.Params(n=24, N=2048), 0)
    try:
        check_both_forms(e, D.weights(5, 17, 65), D.rows_with_edges(6, 2, 65, 25), random_words(np.random.default_rng(7), 17))
    finally:
        e.close()


WORST_I, WORST_O, WORST_N = 65536, 16, 40


@pytest.fixture(scope="module")
def worst_dense(worlds):
    """the widest layers at both weight ends and alternating, created once"""
    alt = np.where(np.arange(WORST_I) % 2 == 0, -128, 127).astype(np.int32)
    Ws = {"min": np.full((WORST_O, WORST_I), -128, np.int32), "max": np.full((WORST_O, WORST_I), 127, np.int32), "alt": np.tile(alt, (WORST_O, 1))}
    hs = {k: worlds(WORST_N).dense(W) for k, W in Ws.items()}
    yield Ws, hs
    for h in hs.values():
        h.close()


@pytest.mark.parametrize("which,word", [("min", 0x00000000), ("min", 0xFFFFFFFF), ("max", 0x80808080), ("alt", None)])
def test_the_largest_accumulator_sums(worlds, worst_dense, which, word):
    """I = 65,536, the kernel's limbs being byte - 128: weights -128 against bytes 0x00 (limb -128) drive every limb sum to I * 128 * 128 = 2^30,
    the bound itself; against bytes 0xFF (limb 127) to -I * 128 * 127, the most negative a layer reaches; weights 127 against 0x80 (limb 0) leave
    the sums at zero and the whole word to the correction term (for a scheme that fed the bytes as they are this would be the extreme);
    alternating weights against planted words mix the signs.  The call takes the atomic path (one workgroup of work, 1,024 K-steps)."""
    Ws, hs = worst_dense
    e = worlds(WORST_N)
    x = np.full((1, WORST_I, WORST_N + 1), word, np.uint32) if word is not None else D.rows_with_edges(0xA17, 1, WORST_I, WORST_N + 1)
    want = D.dense(Ws[which], x)
    import rustfhe_amd as R
    assert slices_of(R, WORST_N, WORST_O, WORST_I, 1) > 1
    dev = run_dev(e, hs[which], x)
    bad = np.argwhere(dev != want)
    assert bad.size == 0, (len(bad), bad[:5])
    if which == "alt":
        assert np.array_equal(e.tlwe_dense_batch(hs[which], x), want)


def test_both_launch_paths_as_the_host_rule_names_them(worlds):
    """the same layer (I = 200: four K-steps) on a batch of one -- the rule cuts I, the parts meet as atomics -- and on a batch of more than two
    workgroups per CU -- plain stores; with and without accumulate on both"""
    import rustfhe_amd as R
    n, I, O = 1, 200, 17
    e = worlds(n)
    W = D.weights(0x9A7, O, I)
    big = 2 * gk.cus() + 1                       # groups = cwgs = 1: that many workgroups
    assert slices_of(R, n, O, I, 1) > 1 and slices_of(R, n, O, I, 3) > 1 and slices_of(R, n, O, I, big) == 1
    bias = random_words(np.random.default_rng(1), O)
    with e.dense(W) as dense:
        for count in (1, 3, big):
            x = D.rows_with_edges(count, count, I, n + 1)
            for acc in (None, acc_words("random", count, O, n + 1)):
                assert np.array_equal(run_dev(e, dense, x, bias, acc), D.dense(W, x, bias, acc)), (count, acc is not None)


def test_bias_alone_and_accumulate_round_trips(worlds):
    n, I, O, count = 40, 65, 17, 3
    e = worlds(n)
    x = D.rows_with_edges(3, count, I, n + 1)
    bias = random_words(np.random.default_rng(4), O)
    with e.dense(np.zeros((O, I), np.int32)) as zero:
        out = run_dev(e, zero, x, bias)
        assert (out[:, :, :n] == 0).all() and np.array_equal(out[:, :, n], np.tile(bias, (count, 1))), "W = 0: the bias on word n, zeros elsewhere"
        assert (e.tlwe_dense_batch(zero, x) == 0).all()
    W = D.weights(5, O, I)
    W[W == -128] = -127                            # so that -W is a layer too
    for kind in ("fill", "random"):
        start = acc_words(kind, count, O, n + 1)
        with e.dense(W) as plus, e.dense(-W) as minus:
            once = run_dev(e, plus, x, None, start)
            assert np.array_equal(once, D.dense(W, x, None, start))
            assert np.array_equal(run_dev(e, minus, x, None, once), start), "accumulate with W, then with -W, returns the start"
    # the same at a shape that takes the atomic path
    I2 = 256
    x2, W2 = D.rows_with_edges(6, 1, I2, n + 1), np.clip(D.weights(7, O, I2), -127, 127)
    import rustfhe_amd as R
    assert slices_of(R, n, O, I2, 1) > 1
    start = acc_words("random", 1, O, n + 1)
    with e.dense(W2) as plus, e.dense(-W2) as minus:
        assert np.array_equal(run_dev(e, minus, x2, None, run_dev(e, plus, x2, None, start)), start)


def test_every_backend_gives_the_same_words(worlds):
    import rustfhe_amd as R
    n, I, O, count = 40, 200, 33, 2
    W, x = D.weights(11, O, I), D.rows_with_edges(12, count, I, n + 1)
    bias = random_words(np.random.default_rng(13), O)
    want = D.dense(W, x, bias)
    for backend in (R._ffi.BACKEND_FFT64_MIRROR, R._ffi.BACKEND_NTT_EXACT, R._ffi.BACKEND_FFT_SPLIT_EXACT):
        e = R.Engine(R.Params(n=n, N=N), 0)            # nothing loaded
        try:
            e.set_backend(backend)
            with e.dense(W) as dense:
                assert np.array_equal(e.tlwe_dense_batch(dense, x, bias), want), backend
                assert np.array_equal(run_dev(e, dense, x, bias), want), backend
        finally:
            e.close()


# ---- meaning: real keys, a sign bootstrap behind the layer ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def keyed():
    import rustfhe_amd as R
    rp = R.Params(n=40, N=N)
    key0, key1, bk, ksk = R.keygen(rp, 0xDE45E)
    e = gk.engine(R, rp, bk, ksk)
    yield R, rp, key0, e
    e.close()


def test_meaning_layer_then_sign_bootstrap(keyed):
    """+-1 messages at unit 2^-6, I = 15 inputs, weights in [-2, 2], a bias of half a unit: pre-activations (s + 1/2) / 64 with |s| <= 30 never
    reach 0 or 1/2.  The layer's phases are W @ m within 6 sqrt(sum W^2) 2^-15 + sum |W| 2^-25: the encryptor's sigma = 2^-15 per input scaled by
    the weights, plus half a step of the 2^-24 grid its f32-derived samples lie on as a common mean -- the layer adds nothing.  A sign table
    (constant test polynomial: +mu on [0, 1/2), -mu on [1/2, 1)) then gives the clear network's flags."""
    import torch
    R, rp, key0, e = keyed
    I, O, count, unit = 15, 5, 6, 1 << 26
    rng = np.random.default_rng(0x51)
    W = rng.integers(-2, 3, (O, I)).astype(np.int32)
    m = rng.choice([-1, 1], (count, I))
    x = R.encrypt_torus(rp, key0, ((m * unit) & 0xFFFFFFFF).astype(np.uint32).reshape(-1), seed=0x52).reshape(count, I, rp.n + 1)
    bias = np.full(O, unit // 2, np.uint32)
    clear = m @ W.T                                                          # [count][O]
    with e.dense(W) as dense:
        out = e.tlwe_dense_batch(dense, x, bias)
        assert np.array_equal(out, D.dense(W, x, bias))
        ph = R.phases(rp, key0, out).reshape(count, O).astype(np.int64)
        want = clear * unit + unit // 2
        err = np.abs(((ph - want + 2 ** 31) % 2 ** 32) - 2 ** 31) / 2.0 ** 32
        bound = 6 * np.sqrt((W.astype(np.float64) ** 2).sum(axis=1)) * 2.0 ** -15 + np.abs(W).sum(axis=1) * 2.0 ** -25
        print("largest |error| per output", err.max(axis=0), "bound", bound)
        assert (err <= bound[None, :]).all(), (err.max(axis=0), bound)
        mu = 1 << 29
        with e.lut(np.full(N, mu, np.uint32)) as sign:
            d_in = gk.to_device(x, np.uint32)
            d_mid = gk.guarded_out(count * O * (rp.n + 1))
            d_out = gk.guarded_out(count * O * (rp.n + 1))
            st = torch.cuda.current_stream().cuda_stream
            e.tlwe_dense_batch_dev(dense, d_in, d_mid, count, bias, False, st)
            e.pbs_batch_dev(sign, d_mid, d_out, count * O, None, st)
            e.sync(st)
            assert np.array_equal(gk.read_guarded(d_mid, out.size).reshape(out.shape), out)
            flags = R.phases(rp, key0, gk.read_guarded(d_out, out.size).reshape(-1, rp.n + 1)).reshape(count, O)
    assert np.array_equal(flags < (1 << 31), clear >= 0), (flags, clear)


def test_agrees_with_a_lut_circuits_weighted_sums(keyed):
    """I = 8, the circuits' fan-in: a one-wave LUT circuit whose nodes carry the layer's weights and biases, against dense -> pbs_many_batch with
    n_out = 1 -- the bootstrap outputs are equal word for word (random words: the arithmetic does not care)"""
    import torch
    R, rp, _, e = keyed
    I, O, count, n1 = 8, 3, 2, rp.n + 1
    rng = np.random.default_rng(0xC1C)
    W = D.weights(0xC1D, O, I)
    bias = random_words(rng, O)
    x = D.rows_with_edges(0xC1E, count, I, n1)
    per = I + O
    wires0 = random_words(rng, (count * per, n1))
    for g in range(count):
        wires0[g * per:g * per + I] = x[g]
    d = {"fan_in": I, "in_idx": np.array([[g * per + i for i in range(I)] for g in range(count) for _ in range(O)], np.int32),
         "weights": np.tile(W, (count, 1)).astype(np.int32), "cst": np.tile(bias, count), "lut_idx": None,
         "wave_offsets": np.array([0, count * O], np.int32), "wave_n_out": np.array([1], np.int32),
         "out_idx": np.array([g * per + I + o for g in range(count) for o in range(O)], np.int32), "num_wires": count * per}
    with e.lut(random_words(rng, (1, N))) as lut, e.dense(W) as dense:
        wires = torch.from_numpy(wires0.view(np.int32)).cuda()
        c = lk.create(e, lut, d, wires)
        try:
            got = lk.replay(e, c, wires)
        finally:
            e.circuit_destroy(c)
        sums = e.tlwe_dense_batch(dense, x, bias)
        want = e.pbs_many_batch(lut, sums.reshape(-1, n1), 1).reshape(count, O, n1)
    for g in range(count):
        assert np.array_equal(got[g * per + I:(g + 1) * per], want[g]), g


# ---- capture, launch counts, refusals, lifetimes --------------------------------------------------------------------------------------------
def test_capture_first_thing_on_a_fresh_stream_and_replay(worlds):
    """a call on the atomic path without accumulate (the clearing memset and the launch) and one on the plain path with accumulate, captured as
    the first things a new stream sees, replayed twice"""
    import torch
    import rustfhe_amd as R
    n, O = 40, 15
    e = worlds(n)
    bias = random_words(np.random.default_rng(2), O)
    for I, count, accumulate in ((200, 1, False), (65, 3, True)):
        assert (slices_of(R, n, O, I, count) > 1) == (I == 200)
        W, x = D.weights(I, O, I), D.rows_with_edges(I + 1, count, I, n + 1)
        acc = acc_words("random", count, O, n + 1) if accumulate else None
        want = D.dense(W, x, bias, acc)
        with e.dense(W) as dense:
            s = torch.cuda.Stream()
            d_x = gk.to_device(x, np.uint32)
            start = acc if accumulate else np.full((count, O, n + 1), FILL, np.uint32)
            d_out = gk.guarded_out(want.size, init=start)
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=s):      # nothing has run on s: the call allocates nothing
                    e.tlwe_dense_batch_dev(dense, d_x, d_out, count, bias, accumulate, s.cuda_stream)
                for _ in range(2):
                    d_out.copy_(gk.guarded_out(want.size, init=start))
                    g.replay()
                    torch.cuda.synchronize()
                    assert np.array_equal(gk.read_guarded(d_out, want.size).reshape(want.shape), want), (I, count)
            e.sync(s.cuda_stream)


def test_one_launch_per_call(worlds):
    import torch
    import rustfhe_amd as R
    n = 40
    e = worlds(n)
    st = torch.cuda.current_stream().cuda_stream
    for I, O, count in ((200, 15, 1), (65, 33, 3), (3, 1, 5)):          # the atomic path first, then plain stores
        W, x = D.weights(I + O, O, I), D.rows_with_edges(I, count, I, n + 1)
        bias = random_words(np.random.default_rng(O), O)
        with e.dense(W) as dense:
            d_x = gk.to_device(x, np.uint32)
            for b in (None, bias):
                d_out = gk.guarded_out(count * O * (n + 1))
                e.timer_begin(st)
                e.tlwe_dense_batch_dev(dense, d_x, d_out, count, b, False, st)
                assert e.timer_end(st)[1] == 1, (I, O, count, slices_of(R, n, O, I, count))
                assert np.array_equal(gk.read_guarded(d_out, count * O * (n + 1)).reshape(count, O, n + 1), D.dense(W, x, b))


def test_a_biased_call_over_512_outputs_whose_launches_differ_in_path(worlds):
    """O = 528 with a bias is two launches: outputs 0 .. 511, then the last 16.  At n = 1 and count = a quarter of the CUs the host rule gives the
    first launch plain stores (eight output groups per sample: two workgroups per CU) and cuts I = 256 into slices for the second (one group
    per sample).  The clearing of a call that does not accumulate must come before BOTH: every word against the oracle, host and _dev forms,
    accumulate off and on, and ceil(O / 512) = 2 launches counted; without a bias the same call is one launch."""
    import torch
    import rustfhe_amd as R
    n, I, O = 1, 256, 528
    count = (2 * gk.cus() + 7) // 8
    assert slices_of(R, n, 512, I, count) == 1 and slices_of(R, n, O - 512, I, count) > 1, "the shapes this test is about"
    e = worlds(n)
    W, x = D.weights(0xB1A5, O, I), D.rows_with_edges(0xB1A6, count, I, n + 1)
    bias = random_words(np.random.default_rng(0xB1A7), O)
    st = torch.cuda.current_stream().cuda_stream
    with e.dense(W) as dense:
        for acc in (None, acc_words("random", count, O, n + 1)):
            want = D.dense(W, x, bias, acc)
            assert np.array_equal(e.tlwe_dense_batch(dense, x, bias, acc), want), acc is not None
            assert np.array_equal(run_dev(e, dense, x, bias, acc), want), acc is not None
        d_x = gk.to_device(x, np.uint32)
        for b, launches in ((bias, 2), (None, 1)):
            d_out = gk.guarded_out(count * O * (n + 1))
            e.timer_begin(st)
            e.tlwe_dense_batch_dev(dense, d_x, d_out, count, b, False, st)
            assert e.timer_end(st)[1] == launches
            assert np.array_equal(gk.read_guarded(d_out, count * O * (n + 1)).reshape(count, O, n + 1), D.dense(W, x, b))


def test_refusals_leave_the_output_untouched(worlds):
    import torch
    import rustfhe_amd as R
    n, I, O, count = 40, 7, 2, 3
    words = n + 1
    e = worlds(n)
    INVALID = R._ffi.ERR_INVALID
    W = D.weights(1, O, I)
    x = D.rows_with_edges(2, count, I, words)
    dense = e.dense(W)
    d_x = gk.to_device(x, np.uint32)
    d_out = gk.guarded_out(count * O * words)
    d_both = torch.full((count * (I + O) * words,), FILL, dtype=torch.int32, device="cuda")      # rows and output in one allocation
    out_host = np.full((count, O, words), FILL, np.uint32)
    x_bytes, out_bytes = count * I * words * 4, count * O * words * 4
    e.timer_begin()

    def dev(h=dense.h, x=d_x.data_ptr(), out=d_out.data_ptr(), count=count, ctx=e.h):
        return e.L.rtfhe_tlwe_dense_batch_dev(ctx, h, x, None, 0, out, count, None)

    def host(x=x.ctypes.data, out=out_host.ctypes.data, count=count):
        return e.L.rtfhe_tlwe_dense_batch(e.h, dense.h, x, None, 0, out, count)

    both = d_both.data_ptr()
    for call, word in ((lambda: dev(x=0), "null"), (lambda: dev(out=0), "null"), (lambda: host(x=None), "null"), (lambda: host(out=None), "null"),
                       (lambda: dev(h=None), "null dense layer"), (lambda: dev(count=1 << 31), "below 2^31 words"),
                       (lambda: host(count=(1 << 31) // (I * words) + 1), "below 2^31 words"),
                       (lambda: dev(x=both, out=both), "overlaps"), (lambda: dev(x=both, out=both + x_bytes - 4), "overlaps"),
                       (lambda: dev(x=both + out_bytes - 4, out=both), "overlaps"), (lambda: dev(x=x.ctypes.data), "device pointers")):
        with pytest.raises(R.RtfheError) as ei:
            e._ck(call())
        assert ei.value.code == INVALID and word in str(ei.value), (word, str(ei.value))
    assert dev(ctx=None) == INVALID                                      # null context
    assert dev(count=0) == 0 and host(count=0) == 0
    h = C.c_void_p()
    for Wbad, Ob, Ib, word in ((W, 0, I, "O = 0"), (W, 65537, I, "O = 65537"), (W, O, 0, "I = 0"), (W, O, 65537, "I = 65537"), (None, O, I, "null")):
        rc = e.L.rtfhe_dense_create(e.h, None if Wbad is None else Wbad.ctypes.data, Ob, Ib, C.byref(h))
        assert rc == INVALID and not h.value and word.encode() in e.L.rtfhe_last_error(e.h), word
    for v, at in ((128, (1, 3)), (-129, (0, 6))):
        bad = W.copy()
        bad[at] = v
        with pytest.raises(R.RtfheError) as ei:
            e.dense(bad)
        assert ei.value.code == INVALID and "W[%d][%d] = %d" % (at[0], at[1], v) in str(ei.value), str(ei.value)
    assert e.L.rtfhe_dense_create(e.h, W.ctypes.data, O, I, None) == INVALID
    assert e.timer_end()[1] == 0, "the checks come before any launch"
    e.sync()
    assert (gk.words_of(d_out) == FILL).all() and (gk.words_of(d_both) == FILL).all() and (out_host == FILL).all()
    # d_out right behind the rows does not overlap them
    d_both[:count * I * words].copy_(gk.to_device(x, np.uint32).reshape(-1))
    e.tlwe_dense_batch_dev(dense, both, both + x_bytes, count)
    e.sync()
    assert np.array_equal(gk.words_of(d_both)[count * I * words:].reshape(count, O, words), D.dense(W, x))
    dense.close()


def test_foreign_orphaned_null_and_early_closed_handles():
    """the lifetime rule of tests/test_gpu_handle_lifetimes.py for the dense layer: two contexts on device 0, n = 4, no keys"""
    import torch
    import rustfhe_amd as R
    INVALID, STATE = R._ffi.ERR_INVALID, R._ffi.ERR_STATE
    p = R.Params(n=4, N=N)
    mine, other = R.Engine(p, 0), R.Engine(p, 0)
    W = np.array([[1, -2, 3]], np.int32)
    try:
        d_x = torch.zeros((1, 3, 5), dtype=torch.int32, device="cuda")
        d_out = torch.full((1, 1, 5), FILL, dtype=torch.int32, device="cuda")

        def call(h):
            return mine.L.rtfhe_tlwe_dense_batch_dev(mine.h, h, d_x.data_ptr(), None, 0, d_out.data_ptr(), 1, None)

        def refused(rc, code, word):
            with pytest.raises(R.RtfheError) as ei:
                mine._ck(rc)
            assert ei.value.code == code and word in str(ei.value), (code, word, str(ei.value))

        late = other.dense(W)
        mine.timer_begin()
        refused(call(late.h), INVALID, "another context")
        refused(call(None), INVALID, "null")
        other.close()
        refused(call(late.h), STATE, "destroyed")
        assert mine.timer_end()[1] == 0, "a refused call launched something"
        mine.sync()
        assert (gk.words_of(d_out) == FILL).all()
        late.close()            # only frees the handle
        late.close()            # ... and a second close has nothing left to do
        first = mine.dense(W)   # closed before its context: the context goes on
        first.close()
        second = mine.dense(W)
        mine.tlwe_dense_batch_dev(second, d_x, d_out, 1)
        mine.sync()
        assert (gk.words_of(d_out) == 0).all()
        second.close()
        second.close()
    finally:
        other.close()
        mine.close()
