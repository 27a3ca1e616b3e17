"""The lifetime rule of the four handle kinds behind a context (rtfhe_lut, rtfhe_trgsw, rtfhe_packing_key, rtfhe_plain), each through one _dev
call whose handle check comes before any key check -- pbs_batch_dev, trgsw_rotate_batch_dev, pack_batch_dev, trlwe_mul_plain_batch_dev -- and,
for tables, through the three row calls of an encrypted table:
  a handle of another context         ERR_INVALID, "another context"
  a handle whose context is gone      ERR_STATE, "destroyed" (the row calls and Selectors.update too); closing it, twice, then does nothing
  a null handle                       ERR_INVALID, "null"
  a handle closed before its context  the context goes on: a second handle of the kind is created and closed
Every refusal comes before any launch (the timer counts none) and leaves the output buffers as they were.
N = 1024, n = 4, no keys loaded (a packing key is 768 KiB), count = 1, depth = 1, n_lut = 2, n_sel = 1, n_w = 1, two contexts on device 0."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, SMALL_N, N_LUT = 1024, 4, 2
FILL = 0x5A5A5A5A
KINDS = ("table", "selector set", "packing key", "plain set")


def _make(R, eng, kind):
    """a handle of `kind` on `eng`, from words that need not decrypt to anything: no call here gets as far as reading them"""
    rng = np.random.default_rng(22)
    p = eng.p
    if kind == "table":
        return eng.lut_encrypted(rng.integers(0, 1 << 32, (N_LUT, 2, N), dtype=np.uint64).astype(np.uint32))
    if kind == "selector set":
        return eng.selectors(rng.integers(0, 1 << 32, (1, 2, 2 * p.l, N), dtype=np.uint64).astype(np.uint32))
    if kind == "packing key":
        return eng.packing_key(rng.integers(0, 1 << 32, R.engine.packing_key_words(p), dtype=np.uint64).astype(np.uint32))
    w = np.zeros((1, N), np.int32)
    w[0, :3] = (1, -2, 3)
    return eng.plain_polys(w)


def _refused(R, eng, rc, code, word):
    with pytest.raises(R.RtfheError) as ei:
        eng._ck(rc)
    assert ei.value.code == code and word in str(ei.value), (code, word, str(ei.value))


@pytest.mark.parametrize("kind", KINDS)
def test_foreign_orphaned_null_and_early_closed_handles(kind):
    import torch
    import rustfhe_amd as R
    INVALID, STATE = R._ffi.ERR_INVALID, R._ffi.ERR_STATE
    p = R.Params(n=SMALL_N, N=N)
    mine, other = R.Engine(p, 0), R.Engine(p, 0)
    try:
        L = mine.L
        d_tlwe = torch.zeros((1, SMALL_N + 1), dtype=torch.int32, device="cuda")
        d_row = torch.zeros((1, 2, N), dtype=torch.int32, device="cuda")
        d_out = torch.full((1, 2, N), FILL, dtype=torch.int32, device="cuda")          # large enough for every call's output
        d_rows_out = torch.full((1, 2, N), FILL, dtype=torch.int32, device="cuda")     # ... and for read_dev's
        tlwe, row, out = d_tlwe.data_ptr(), d_row.data_ptr(), d_out.data_ptr()

        def call(h):      # the kind's _dev call on `mine` with the handle h (None: a null handle), count = 1
            if kind == "table":
                return L.rtfhe_pbs_batch_dev(mine.h, h, None, tlwe, out, 1, None)
            if kind == "selector set":
                return L.rtfhe_trgsw_rotate_batch_dev(mine.h, h, None, 1, None, row, out, 1, None)
            if kind == "packing key":
                return L.rtfhe_pack_batch_dev(mine.h, h, tlwe, 1, None, 1, out, 1, None)
            return L.rtfhe_trlwe_mul_plain_batch_dev(mine.h, h, None, row, 1, None, 1, 0, out, 1, None)

        late = _make(R, other, kind)
        mine.timer_begin()
        _refused(R, mine, call(late.h), INVALID, "another context")
        _refused(R, mine, call(None), INVALID, "null")
        other.close()
        _refused(R, mine, call(late.h), STATE, "destroyed")
        if kind == "table":
            for row_call in (lambda: late.update_dev(d_row, 0, 1), lambda: late.accumulate_dev(d_row, 0, 1, 1), lambda: late.read_dev(d_rows_out, 0, 1)):
                with pytest.raises(R.RtfheError) as ei:
                    row_call()
                assert ei.value.code == STATE and "destroyed" in str(ei.value), str(ei.value)
            for rc in (L.rtfhe_lut_update_dev(None, row, 0, 1, None), L.rtfhe_lut_accumulate_dev(None, row, 0, 1, 1, None),
                       L.rtfhe_lut_read_dev(None, d_rows_out.data_ptr(), 0, 1, None)):
                assert rc == INVALID and b"null" in L.rtfhe_last_error(None)
        if kind == "selector set":
            with pytest.raises(R.RtfheError) as ei:
                late.update(np.zeros((1, 2, 2 * p.l, N), np.uint32))
            assert ei.value.code == STATE, str(ei.value)
        assert mine.timer_end()[1] == 0, "a refused call launched something"
        mine.sync()
        assert (d_out.cpu().numpy().view(np.uint32) == FILL).all() and (d_rows_out.cpu().numpy().view(np.uint32) == FILL).all()
        late.close()            # only frees the handle
        late.close()            # ... and a second close has nothing left to do
        # closed before its context: the context goes on
        first = _make(R, mine, kind)
        first.close()
        second = _make(R, mine, kind)
        second.close()
        second.close()
        mine.sync()
    finally:
        other.close()
        mine.close()


def test_a_refused_create_leaves_no_handle_and_the_context_goes_on():
    """Each of the five data handle types (the four above and rtfhe_dense), through the C entry points themselves: a create that its argument checks
    refuse returns ERR_INVALID and leaves *out null; a valid create and destroy on the same context then work, and the context destroys cleanly.
    n = 8, N = 1024: one table row, one selector, a packing key of n * 8 * 3 rows (1.5 MB), one plain polynomial, a 1 x 1 matrix."""
    import ctypes as C
    import rustfhe_amd as R
    p = R.Params(n=8, N=N)
    eng = R.Engine(p, 0)
    try:
        L, ctx = eng.L, eng.h
        rng = np.random.default_rng(31)
        words = lambda *shape: rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)
        tv, trgsw, pk = words(1, N), words(1, 2, 2 * p.l, N), words(*np.atleast_1d(R.engine.packing_key_words(p)))
        assert pk.size == p.n * 8 * 3 * 2 * N
        poly, one, wide = np.zeros((1, N), np.int32), np.ones((1, 1), np.int32), np.full((1, 1), 128, np.int32)
        poly[0, :3] = (1, -2, 3)
        ptr = lambda a: a.ctypes.data
        # (create, destroy, [(arguments its checks refuse, a word of the message)], valid arguments)
        kinds = [
            (L.rtfhe_lut_create, L.rtfhe_lut_destroy, [((ptr(tv), 0), "n_lut < 1"), ((None, 1), "null argument")], (ptr(tv), 1)),
            (L.rtfhe_trgsw_create, L.rtfhe_trgsw_destroy, [((ptr(trgsw), 0), "n_sel < 1"), ((ptr(trgsw), 1 << 28), "n_sel too large")], (ptr(trgsw), 1)),
            (L.rtfhe_packing_key_create, L.rtfhe_packing_key_destroy, [((None,), "null argument")], (ptr(pk),)),
            (L.rtfhe_plain_create, L.rtfhe_plain_destroy, [((ptr(poly), 0), "n_w = 0"), ((None, 1), "null argument")], (ptr(poly), 1)),
            (L.rtfhe_dense_create, L.rtfhe_dense_destroy, [((ptr(one), 0, 1), "O = 0"), ((ptr(wide), 1, 1), "W[0][0] = 128")], (ptr(one), 1, 1)),
        ]
        for create, destroy, refusals, valid in kinds:
            for args, word in refusals:
                h = C.c_void_p()
                _refused(R, eng, create(ctx, *args, C.byref(h)), R._ffi.ERR_INVALID, word)
                assert h.value is None, (create.__name__, args)
            h = C.c_void_p()
            eng._ck(create(ctx, *valid, C.byref(h)))
            assert h.value
            destroy(h)
        eng.sync()
    finally:
        eng.close()
