"""GPU: the TRLWE key switch on buffers past 2 GiB, 4 GiB and 8 GiB ("Address arithmetic"; the row of k_trlwe_auto), written with
tests/large_kit.py as tests/test_gpu_large_buffers.py is: the big buffers are made, filled, compared and probed on the device; every word of the
big call against the same call on slices of the same inputs, and the probe rows -- both ends of the call and either side of every boundary it
crosses -- against the restatement (tests/auto_oracle.py).  One replace step per row, out of place at N = 1024 and in place at N = 2048."""
import numpy as np
import pytest

import auto_oracle as A
import gpu_kit as gk
import large_kit as lk
from kit import SMALL_N

pytestmark = pytest.mark.gpu


def _switch(orc, N, count, in_place, label):
    """one step (entry 1 of a two-exponent key of random words, t = N + 1) per row: rows [count][2][N] in, the same shape out"""
    import torch
    import rustfhe_amd as R
    row = 2 * N
    lk.need(4 * count * row * 2 + (2 << 30))
    rp, p = R.Params(n=SMALL_N[N], N=N), orc.Params(n=SMALL_N[N], N=N)
    t = [3, N + 1]
    words = np.random.default_rng(0x1A0 + N).integers(0, 1 << 32, (len(t), rp.l, 2, N), dtype=np.uint64).astype(np.uint32)
    key_f = A.spectra(p, orc.Plan(N), words)
    e = R.Engine(rp, 0)
    key = e.trlwe_switch_key(words, t)
    try:
        st = torch.cuda.current_stream().cuda_stream
        d_in = lk.device_words(count * row, 0x1A1 + N)
        d_out = lk.guarded_device(count * row)
        if in_place:
            d_out[:count * row] = d_in                      # d_in keeps the rows the call reads: the in-place buffer is d_out
            e.trlwe_auto_batch_dev(key, d_out, d_out, count, [1], None, st)
        else:
            e.trlwe_auto_batch_dev(key, d_in, d_out, count, [1], None, st)
        e.sync(st)
        lk.report(label, e)

        def call(s, d_chunk, cnt):
            if in_place:
                d_chunk[:cnt * row] = s[0]
            e.trlwe_auto_batch_dev(key, d_chunk if in_place else s[0], d_chunk, cnt, [1], None, st)
            e.sync(st)
        lk.same_as_chunks(call, [(d_in, row)], (d_out, row), count, (1 << 30) // (4 * row))
        pick = lk.probe_items(count, 4 * row)
        x = lk.rows_of(d_in, row, pick)
        exp = gk.pmap(lambda k: A.step(p, gk.oracle_plan(orc, N), key_f, 1, t[1], x[k].reshape(2, N), False, A.REFERENCE).reshape(-1), range(len(pick)))
        diff = np.flatnonzero((lk.rows_of(d_out, row, pick) != np.stack(exp)).any(axis=1))
        assert diff.size == 0, ("rows that differ from the restatement", pick[diff][:16].tolist())
        lk.check_canary(d_out, count * row)
        torch.cuda.synchronize()
    finally:
        key.close()
        e.close()
        d_in = d_out = None
        lk.release()


def test_trlwe_auto_out_of_place_past_4_gib(orc):
    """524,288 + 3 rows at N = 1024: input and output rows past byte offsets 2^31 and 2^32"""
    _switch(orc, 1024, 524288 + 3, False, "trlwe_auto_batch_dev out of place")


def test_trlwe_auto_in_place_past_8_gib(orc):
    """524,288 + 3 rows at N = 2048, d_out == d_x: one 8.6 GB buffer, past byte offsets 2^31, 2^32 and 2^33 (a copy of the rows stands beside it
    for the restatement and the slices)"""
    _switch(orc, 2048, 524288 + 3, True, "trlwe_auto_batch_dev in place")
