"""CPU: the lvl0 dense layer (include/rtfhe.h: rtfhe_tlwe_dense_batch) without a device -- the numpy oracle the GPU tests compare every word to
against a loop over Python integers, the host-only plan (rustfhe_amd/csrc/rtfhe_dense_plan.cpp) through ctypes: its refusals, its correction
words against the oracle's, the launch rule; and linear.dense_bias."""
import ctypes as C

import numpy as np
import pytest

import dense_oracle as D


class Shape(C.Structure):
    """rtfhe_dense_shape"""
    _fields_ = [(k, C.c_int32) for k in ("tiles", "groups", "cwgs", "ksteps", "slices", "steps")]


@pytest.fixture(scope="module")
def lib():
    import rustfhe_amd as R
    L = R.load()
    L.rtfhe_dense_weights_plan.restype = C.c_int
    L.rtfhe_dense_weights_plan.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_char_p, C.c_size_t]
    L.rtfhe_dense_plan.restype = C.c_int
    L.rtfhe_dense_plan.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_size_t, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
    L.rtfhe_dense_launch_shape.restype = None
    L.rtfhe_dense_launch_shape.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_size_t, C.c_int32, C.POINTER(Shape)]
    return L


def _weights(lib, W, O=None, I=None, corr="own"):
    """(rc, message, corr) of rtfhe_dense_weights_plan"""
    W = None if W is None else np.ascontiguousarray(W, np.int32)
    O, I = (W.shape[0] if O is None else O), (W.shape[1] if I is None else I)
    out = np.full(max(1, min(O, 65536)), 0xAAAAAAAA, np.uint32) if corr == "own" else corr
    err = C.create_string_buffer(256)
    rc = lib.rtfhe_dense_weights_plan(None if W is None else W.ctypes.data, O, I, None if out is None else out.ctypes.data, err, len(err))
    return rc, err.value.decode(), out


def _plan(lib, n, O, I, count, x=0x10000000, out=0x4000000000):
    err = C.create_string_buffer(256)
    return lib.rtfhe_dense_plan(n, O, I, count, x, out, err, len(err)), err.value.decode()


def test_oracle_equals_a_python_integer_loop():
    assert D.self_test()


def test_planted_edge_words_are_there():
    x = D.rows_with_edges(9, 3, 7, 41)
    for g in range(3):
        assert set(D.EDGE_WORDS) <= set(x[g].reshape(-1).tolist())
        assert set(x[g, :, 0].tolist()) & set(D.EDGE_WORDS) and set(x[g, :, -1].tolist()) & set(D.EDGE_WORDS)
    W = D.weights(4, 5, 9)
    assert W.min() == -128 and W.max() == 127 and W.dtype == np.int32


def test_correction_words_equal_the_oracles(lib):
    for seed, (O, I) in enumerate([(1, 1), (3, 5), (17, 200), (33, 65), (2, 65536)]):
        W = D.weights(seed, O, I)
        rc, msg, corr = _weights(lib, W)
        assert rc == 0 and msg == "" and np.array_equal(corr, D.correction(W)), (O, I)
    for fill in (-128, 127):          # the widest rows: |sum| = 2^23
        W = np.full((1, 65536), fill, np.int32)
        assert np.array_equal(_weights(lib, W)[2], D.correction(W))
    # what the correction is for: limbs of (byte - 128) plus it give the plain wrapping sum
    W, x = D.weights(7, 4, 9), D.rows_with_edges(8, 1, 9, 5)[0]
    limbs = sum(((W.astype(np.int64) @ (((x.astype(np.int64) >> (8 * j)) & 0xFF) - 128)) << (8 * j)) for j in range(4))
    assert np.array_equal(((limbs + D.correction(W).astype(np.int64)[:, None]) & D.MASK).astype(np.uint32), D.dense(W, x[None])[0])


def test_the_plan_refuses_bad_matrices(lib):
    import rustfhe_amd as R
    W = np.zeros((3, 5), np.int32)
    for v, at in ((128, (1, 2)), (-129, (2, 4)), (1 << 20, (0, 0))):
        bad = W.copy()
        bad[at] = v
        bad[2, 4] = bad[2, 4] or 999        # a later offender too: the FIRST is named
        rc, msg, corr = _weights(lib, bad)
        first = (0, 0) if v == 1 << 20 else at
        assert rc == R._ffi.ERR_INVALID and "W[%d][%d] = %d" % (first[0], first[1], bad[first]) in msg, msg
        assert (corr == 0xAAAAAAAA).all(), "nothing is written on a refusal"
    for O, I, word in ((0, 5, "O = 0"), (65537, 5, "O = 65537"), (3, 0, "I = 0"), (3, 65537, "I = 65537"), (-1, 5, "O = -1")):
        rc, msg, _ = _weights(lib, W, O, I)          # the limits come before W is read
        assert rc == R._ffi.ERR_INVALID and word in msg, msg
    assert _weights(lib, None, 3, 5)[0] == R._ffi.ERR_INVALID and "null" in _weights(lib, None, 3, 5)[1]
    assert _weights(lib, W, corr=None)[0] == R._ffi.ERR_INVALID
    assert _weights(lib, np.full((2, 3), -128, np.int32))[0] == 0 and _weights(lib, np.full((2, 3), 127, np.int32))[0] == 0


def test_the_plan_refuses_bad_calls(lib):
    import rustfhe_amd as R
    assert _plan(lib, 1, 1, 1, 1) == (0, "")
    assert _plan(lib, 767, 65536, 65536, 42)[0] == 0 and _plan(lib, 635, 32, 784, 0)[0] == 0
    x, words = 0x10000000, 41
    assert _plan(lib, 40, 2, 7, 3, x, x + 3 * 7 * words * 4)[0] == 0 and _plan(lib, 40, 2, 7, 3, x, x - 3 * 2 * words * 4)[0] == 0
    for args, word in (((40, 0, 7, 3), "O = 0"), ((40, 65537, 7, 3), "O = 65537"), ((40, 2, 0, 3), "I = 0"), ((40, 2, 65537, 3), "I = 65537"),
                       ((0, 2, 7, 3), "n = 0"), ((767, 65536, 1, 43), "below 2^31 words"), ((767, 1, 65536, 43), "below 2^31 words"),
                       ((1, 1, 1, 1 << 30), "below 2^31 words"), ((40, 2, 7, 3, 0), "null"), ((40, 2, 7, 3, x, 0), "null"),
                       ((40, 2, 7, 3, x, x), "overlaps"), ((40, 2, 7, 3, x, x + 3 * 7 * words * 4 - 4), "overlaps"),
                       ((40, 2, 7, 3, x, x - 3 * 2 * words * 4 + 4), "overlaps")):
        rc, msg = _plan(lib, *args)
        assert rc == R._ffi.ERR_INVALID and word in msg, (args, msg)


def test_the_launch_rule(lib):
    def shape(n, O, I, count, cus=256):
        s = Shape()
        lib.rtfhe_dense_launch_shape(n, O, I, count, cus, C.byref(s))
        return s.tiles, s.groups, s.cwgs, s.ksteps, s.slices, s.steps
    assert shape(635, 32, 784, 1024) == (2, 1, 5, 13, 1, 13)          # a full batch: plain stores, one pass over x
    assert shape(635, 512, 784, 256) == (4, 8, 5, 13, 1, 13)          # eight passes
    assert shape(40, 16, 65536, 1) == (1, 1, 1, 1024, 512, 2)         # one workgroup of work: I cut into 512 slices
    assert shape(635, 32, 784, 1) == (2, 1, 5, 13, 5, 3)              # one sample: 13 K-steps cut into 5 slices of at most 3
    assert shape(1, 1, 1, 1) == (1, 1, 1, 1, 1, 1) and shape(767, 33, 65, 5)[4] == 1      # too few K-steps to cut
    for n, O, I, count in ((40, 17, 200, 2), (767, 1, 784, 3), (16, 33, 65536, 5)):
        t, g, cw, ks, sl, st = shape(n, O, I, count)
        assert sl * st >= ks > (sl - 1) * st and (sl == 1 or st >= 2)


def test_dense_bias():
    import rustfhe_amd as R
    unit = 1 << 27
    got = R.dense_bias([0, 1, -1, 16, -17, 40], unit)
    assert got.dtype == np.uint32 and got.tolist() == [0, unit, (1 << 32) - unit, 1 << 31, ((-17 * unit) % (1 << 32)), (40 * unit) % (1 << 32)]
    assert R.dense_bias(np.zeros(0, np.int64), unit).shape == (0,)
    with pytest.raises(AssertionError):
        R.dense_bias([0.5], unit)


def test_the_sign_network_examples_clear_arithmetic():
    """examples/dense_sign_network.py without a device: noisy templates decode to their templates' labels, exactly one hidden neuron fires, and
    every clear pre-activation, scaled by its unit, stays inside (-1/2, 1/2) and away from both boundaries of the sign"""
    from kit import load_example
    ex = load_example("dense_sign_network")
    templates, labels, W1, b1, W2, b2 = ex.network(5)
    assert np.abs(W1).max() <= 127 and np.abs(W2).max() <= 127 and len(set(labels.tolist())) == ex.O1
    rng = np.random.default_rng(6)
    which = rng.integers(0, ex.O1, 64)
    x = templates[which] * np.where(rng.random((64, ex.I1)) < 0.1, -1, 1)
    pre1, h, pre2, flags = ex.clear_forward(W1, b1, W2, b2, x)
    assert ((h > 0).sum(axis=1) == 1).all() and np.array_equal(np.argmax(h, axis=1), which)
    assert np.array_equal(((flags > 0).astype(np.int64) << np.arange(ex.O2)).sum(axis=1), labels[which])
    for pre, unit in ((pre1, ex.U1), (pre2, ex.U2)):
        frac = np.abs(pre) * unit / 2.0 ** 32
        assert frac.max() < 0.5 and np.minimum(frac, 0.5 - frac).min() >= 0.02, (frac.min(), frac.max())
    assert np.array_equal(np.abs(pre2), np.full(pre2.shape, 2))
