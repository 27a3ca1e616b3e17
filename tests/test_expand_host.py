"""CPU: the host-only part of the device-side expansion of compressed rows (rtfhe_tlwe_expand_batch_dev, rtfhe_trlwe_expand_batch_dev): the
inverse map of a coefficient list (rtfhe_expand_inverse_map, rustfhe_amd/csrc/rtfhe_compress_plan.cpp) against a numpy restatement, that the
map is what the CPU twin rtfhe_trlwe_expand does with the same list, the two new symbols, and the argument handling of the Python helpers
Engine.upload_tlwe_compressed / upload_trlwe_compressed, which is done before a device is touched."""
import ctypes as C

import numpy as np
import pytest

import compress_oracle as O


def _lib():
    import rustfhe_amd as R
    L = R.load()
    L.rtfhe_expand_inverse_map.restype = C.c_int
    L.rtfhe_expand_inverse_map.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    return R, L


def _restated(N, idx):
    """inv[j] = the last p with idx[p] == j, or -1 -- by search, not by overwriting"""
    idx = np.asarray(idx)
    return np.array([max(np.flatnonzero(idx == j), default=-1) for j in range(N)], np.int16)


def _lists(N):
    rng = np.random.default_rng(N)
    dup = rng.integers(0, N, 33)
    dup[5] = dup[4] = dup[30] = dup[0]
    return [[N - 1], [0], [N - 1, 0, N // 2], list(range(N - 1, -1, -1)), list(range(N)), [3, 3, N - 1, 3, 0], dup.tolist(),
            rng.integers(0, N, N).tolist(), [7] * 40]


@pytest.mark.parametrize("N", [1, 16, 1024, 2048])
def test_inverse_map_equals_the_restatement(N):
    R, L = _lib()
    for lst in _lists(N):
        idx = np.array(lst[:N], np.int32) % N
        inv = np.full(N + 2, 0x5A5A, np.int16)                                       # a guard word either side
        assert L.rtfhe_expand_inverse_map(N, idx.size, idx.ctypes.data, inv[1:].ctypes.data) == 0
        assert inv[0] == 0x5A5A and inv[-1] == 0x5A5A
        assert np.array_equal(inv[1:-1], _restated(N, idx)), (N, idx[:8])


def test_inverse_map_is_what_the_cpu_twin_does_with_the_list():
    """b[j] of rtfhe_trlwe_expand is value N + inv[j] where inv[j] >= 0 and zero elsewhere"""
    R, L = _lib()
    N, k = 1024, 12
    for lst in _lists(N):
        idx = np.array(lst, np.int32)
        P = idx.size
        vals = np.random.default_rng(P).integers(0, 1 << k, (2, N + P))
        full = R.trlwe_expand(N, k, O.pack_rows(vals, k), P, idx)
        inv = np.empty(N, np.int16)
        assert L.rtfhe_expand_inverse_map(N, P, idx.ctypes.data, inv.ctypes.data) == 0
        want = np.where(inv >= 0, vals[:, N + np.maximum(inv, 0)] << (32 - k), 0).astype(np.uint32)
        assert np.array_equal(full[:, 0], want) and np.array_equal(full[:, 1], (vals[:, :N] << (32 - k)).astype(np.uint32))


def test_inverse_map_refusals_write_nothing():
    R, L = _lib()
    INV = R._ffi.ERR_INVALID
    N = 1024
    idx = np.array([0, 5, N - 1], np.int32)
    inv = np.full(N, 0x5A5A, np.int16)
    f = L.rtfhe_expand_inverse_map
    assert f(N, 3, None, inv.ctypes.data) == INV and f(N, 3, idx.ctypes.data, None) == INV
    assert f(0, 1, idx.ctypes.data, inv.ctypes.data) == INV and f(-1, 1, idx.ctypes.data, inv.ctypes.data) == INV
    assert f(32769, 1, idx.ctypes.data, inv.ctypes.data) == INV                       # p would not fit an int16
    assert f(N, 0, idx.ctypes.data, inv.ctypes.data) == INV and f(2, 3, idx.ctypes.data, inv.ctypes.data) == INV
    for bad in ([0, -1, 5], [0, 1, N]):
        b = np.array(bad, np.int32)
        assert f(N, 3, b.ctypes.data, inv.ctypes.data) == INV
    assert (inv == 0x5A5A).all()


def test_the_library_exports_the_device_calls():
    R, L = _lib()
    assert L.rtfhe_tlwe_expand_batch_dev and L.rtfhe_trlwe_expand_batch_dev
    INV = R._ffi.ERR_INVALID
    assert L.rtfhe_tlwe_expand_batch_dev(None, 10, None, None, 0, None) == INV        # a null context, refused before any device is asked for
    assert L.rtfhe_trlwe_expand_batch_dev(None, 12, None, 1, None, 1, None, 0, None) == INV
    for name in ("tlwe_expand_dev", "trlwe_expand_dev", "upload_tlwe_compressed", "upload_trlwe_compressed"):
        assert callable(getattr(R.Engine, name))


def test_packed_rows_takes_what_read_compressed_returns(tmp_path):
    """the helpers' host half: rows as read_compressed returns them go through untouched; a flat array is cut into rows; a wrong row length, a
    ragged size and a bad k raise RtfheError -- all before any device call"""
    import rustfhe_amd as R
    from rustfhe_amd.engine import packed_rows
    n, N, k = 635, 1024, 10
    rng = np.random.default_rng(5)
    t = R.tlwe_compress(n, k, rng.integers(0, 1 << 32, (5, n + 1), dtype=np.uint64).astype(np.uint32))
    path = str(tmp_path / "lvl0.rtfhe")
    R.write_compressed(path, t, k, n=n)
    words, k2, n2, _, _ = R.read_compressed(path)
    got = packed_rows(words, n2 + 1, k2)
    assert got.dtype == np.uint32 and got.flags.c_contiguous and np.array_equal(got, t)
    assert np.array_equal(packed_rows(t.reshape(-1), n + 1, k), t)
    assert packed_rows(t[:0], n + 1, k).shape == (0, O.words(n + 1, k))
    coef = np.array([N - 1, 0, 512, 0, 7], np.int32)
    c = R.trlwe_compress(N, 12, rng.integers(0, 1 << 32, (3, 2, N), dtype=np.uint64).astype(np.uint32), 5, coef)
    tpath = str(tmp_path / "trlwe.rtfhe")
    R.write_compressed(tpath, c, 12, N=N, coef=coef)
    words, k2, _, N2, coef2 = R.read_compressed(tpath)
    assert np.array_equal(packed_rows(words, N2 + len(coef2), k2), c)
    INV = R._ffi.ERR_INVALID
    for bad in (lambda: packed_rows(t, n + 1, 1), lambda: packed_rows(t, n + 1, 33), lambda: packed_rows(t, n + 2, k),
                lambda: packed_rows(t.reshape(-1)[:-1], n + 1, k), lambda: packed_rows(t[:, :-1], n + 1, k), lambda: packed_rows(t, 0, k)):
        with pytest.raises(R.RtfheError) as ei:
            bad()
        assert ei.value.code == INV


def test_upload_helpers_check_their_arguments_without_a_device():
    """on an Engine object that has no context behind it: every refusal below is raised before the helper reaches the library or torch"""
    import rustfhe_amd as R
    e = object.__new__(R.Engine)
    e.p, e.h, e.device = R.Params(), None, 0
    W0, W1 = O.words(636, 10), O.words(1024 + 3, 12)
    for bad in (lambda: e.upload_tlwe_compressed(np.zeros((2, W0 + 1), np.uint32), 10), lambda: e.upload_tlwe_compressed(np.zeros((2, W0), np.uint32), 1),
                lambda: e.upload_tlwe_compressed(np.zeros(2 * W0 - 1, np.uint32), 10),
                lambda: e.upload_trlwe_compressed(np.zeros((2, W1), np.uint32), 12, 0), lambda: e.upload_trlwe_compressed(np.zeros((2, W1), np.uint32), 12, 1025),
                lambda: e.upload_trlwe_compressed(np.zeros((2, W1), np.uint32), 12, 8), lambda: e.upload_trlwe_compressed(np.zeros((2, W1), np.uint32), 40, 3)):
        with pytest.raises(R.RtfheError) as ei:
            bad()
        assert ei.value.code == R._ffi.ERR_INVALID
    with pytest.raises(AssertionError):                                              # one coefficient per kept value, as in trlwe_compress_dev
        e.upload_trlwe_compressed(np.zeros((2, W1), np.uint32), 12, 3, [0, 1])
