"""GPU: the device-side expansion of compressed rows on outputs past 2 GiB and 4 GiB (DESIGN.md 5.23, 6.2 "Address arithmetic").  The plan
bounds count * L, the PACKED values, by 2^31; the full rows a call writes are up to 3.2 times as many words, so the output passes byte offset
2^32 from an input far below it and count * 2 N comes close to 2^32 words.  Built on tests/large_kit.py as tests/test_gpu_large_buffers.py is:
every output word against the same entry point on slices (same_as_chunks), the rows of probe_items -- both ends, 32 items either side of every
boundary crossed, 128 at random -- against the numpy restatement, and the canary behind the output.  No tolerance.  The inputs are random words:
every bit pattern is a valid packed row, and the padding bits of the TRLWE rows (385 words hold 12,300 bits of 12,320) are random with them."""
import numpy as np
import pytest

import compress_oracle as co
import large_kit as lk

pytestmark = pytest.mark.gpu


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _bare_engine(N, n=2):
    import rustfhe_amd as R
    return R.Engine(R.Params(n=n, N=N), 0)


def test_tlwe_expand_far_output():
    """1,398,102 + 3 lvl0 rows at n = 767 (3,072 bytes each), k = 10: a 4.3 GB output (B31, B32) from a 1.3 GB input"""
    n, k, count = 767, 10, 1398102 + 3
    W = co.words(n + 1, k)
    lk.need(4 * count * (n + 1 + W) + (2 << 30))
    e = _bare_engine(1024, n)
    try:
        st = _stream()
        assert lk.crossed(count, 4 * (n + 1)) == ["B31", "B32"]
        d_in = lk.device_words(count * W, 2310)
        d_out = lk.guarded_device(count * (n + 1))
        e.tlwe_expand_dev(d_in, k, d_out, count, st)
        e.sync(st)
        lk.report("tlwe_expand_dev far output", e)

        def call(s, d_chunk, cnt):
            e.tlwe_expand_dev(s[0], k, d_chunk, cnt, st)
            e.sync(st)
        lk.same_as_chunks(call, [(d_in, W)], (d_out, n + 1), count, (1 << 30) // (4 * (n + 1)))
        pick = lk.probe_items(count, 4 * (n + 1))
        exp = co.tlwe_expand(lk.rows_of(d_in, W, pick), n, k)
        diff = np.flatnonzero((lk.rows_of(d_out, n + 1, pick) != exp).any(axis=1))
        assert diff.size == 0, ("rows that differ from the oracle", pick[diff][:16].tolist())
        lk.check_canary(d_out, count * (n + 1))
    finally:
        e.close()
        d_in = d_out = None
        lk.release()


@pytest.mark.parametrize("count,coef", [(524288 + 3, None), (524288 + 3, [1023]), ((2 ** 31 - 1) // 1025, None)], ids=["null", "list", "most"])
def test_trlwe_expand_far_output(count, coef):
    """524,288 + 3 TRLWEs at N = 1024, P = 1, k = 12: 4.3 GB of output (B31, B32; count * 2 N = 2^30 + 6,144 words) from 0.8 GB of input, with a
    NULL list (the kept coefficient is computed) and with a list (it is looked up in the inverse map).  "most": the largest count the plan
    accepts at this shape, 2,095,103 rows -- count * 2 N = 2^32 - 4,196,352 output words, so lane indices pass 2^31 and end just below 2^32,
    the output is 17.2 GB (B31, B32, W31) and the input 3.2 GB (B31)"""
    N, k, P = 1024, 12, 1
    W = co.words(N + P, k)
    lk.need(4 * count * (2 * N + W) + (2 << 30))
    e = _bare_engine(N)
    try:
        st = _stream()
        assert lk.crossed(count, 8 * N) == (["B31", "B32"] if count < (1 << 20) else ["B31", "B32", "W31"])
        d_in = lk.device_words(count * W, 2311)
        d_out = lk.guarded_device(count * 2 * N)
        e.trlwe_expand_dev(d_in, k, P, d_out, count, coef, 1, st)
        e.sync(st)
        lk.report("trlwe_expand_dev far output", e)

        def call(s, d_chunk, cnt):
            e.trlwe_expand_dev(s[0], k, P, d_chunk, cnt, coef, 1, st)
            e.sync(st)
        lk.same_as_chunks(call, [(d_in, W)], (d_out, 2 * N), count, (1 << 30) // (8 * N))
        pick = lk.probe_items(count, 8 * N)
        exp = co.trlwe_expand(lk.rows_of(d_in, W, pick), N, k, P, coef).reshape(-1, 2 * N)
        diff = np.flatnonzero((lk.rows_of(d_out, 2 * N, pick) != exp).any(axis=1))
        assert diff.size == 0, ("rows that differ from the oracle", pick[diff][:16].tolist())
        lk.check_canary(d_out, count * 2 * N)
    finally:
        e.close()
        d_in = d_out = None
        lk.release()
