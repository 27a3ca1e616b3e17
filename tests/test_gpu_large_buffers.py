"""GPU: device entry points on buffers past 2 GiB, 4 GiB and 8 GiB -- WHERE in memory a row lies ("Address arithmetic").

Every test makes one big call whose far array crosses byte offset 2^31 (B31), 2^32 (B32) and, where stated, word index 2^31 (W31, byte 2^33)
and 2^32 (W32, byte 2^34), on a context of its own with the smallest arithmetic that still reaches the span (n = 2 or 8 where a key is
needed).  Then (a) large_kit.same_as_chunks compares EVERY output word with the same entry point run on slices of the same inputs, no buffer
of a slice call above 2^30 bytes, the key-switching tests on a second context whose sample buffer stays that small; (b) the rows of
large_kit.probe_items -- both ends of the call, 32 items either side of every boundary crossed and of every key-switch segment edge, 128 drawn
at random -- are compared word for word with the family's oracle; (c) the canary behind the output is checked.  There is no tolerance in this
file.  The rows of the table in DESIGN.md 6.2 that this module runs: all 22 of the issue and the two the reading added (23, 24); the numbers in the test names are that table's.

Tests 1-6 assert that the batch took the split path (rtfhe_timer_end_detail reports key-switch time, which only launch_key_switch_mm
brackets) and that the context's sample buffer passed 2^31 bytes (rtfhe_ctx_memory_bytes), i.e. that the key switch ran in more than one
segment: a batch that fell back to the fused kernel would prove nothing here.  Durations and peak memory: profiles/r32/README.md."""
import numpy as np
import pytest

import compress_oracle as co
import dense_oracle as do
import gpu_kit as gk
import large_kit as lk
import leveled_kit as lv
import lut_circuit_kit as lck
import pack_oracle as po
import plain_mul_oracle as pmo
import round_oracle as ro
import seeded_oracle as so
import tlwe_seeded_oracle as tso
import trgsw_mac_oracle as tmo
from extract_helpers import extract_formula
from kit import random_words
from large_kit import _chunk_samples, _split_path_taken, _stream, _tile_bytes
from leveled_oracle import as_trlwe, oracle_cmux_net, oracle_cmux_tree, oracle_demux_tree, oracle_trgsw_rotate
from pbs_oracle import oracle_pbs_many

pytestmark = pytest.mark.gpu

IN_ROWS = 64          # input rows of the netlist wave's wire table


class World:
    """one key set of the oracle's keygen at a tiny n, and contexts with it loaded"""

    def __init__(self, orc, N, n):
        import rustfhe_amd as R
        self.orc, self.N, self.n = orc, N, n
        self.P = orc.Params(n=n, N=N)
        self.K = orc.Keys(self.P, 3200 + N + n)
        self.p = R.Params(n=n, N=N)

    def engine(self, backend=None):
        import rustfhe_amd as R
        e = gk.engine(R, self.p, self.K.bk_t, self.K.ksk)
        if backend is not None:
            e.set_backend(backend)
        return e


@pytest.fixture(scope="module")
def worlds(orc):
    return gk.Worlds(lambda N, n: World(orc, N, n), close=lambda w: None)


# ---- 1-3: plain gate batches, the split path in two and three key-switch segments --------------------------------------------------------
def _gate_batch(worlds, N, count, backend, exact, label):
    import rustfhe_amd as R
    import torch
    lk.need(-(-count // 16) * _tile_bytes(N) + (1 << 30) + 4 * 12 * count)
    w = worlds(N, 2)
    orc, n = w.orc, w.n
    e, e_small = w.engine(backend), w.engine(backend)
    try:
        st = _stream()
        d0, d1 = lk.device_words(count * (n + 1), 31 * N + 1), lk.device_words(count * (n + 1), 31 * N + 2)
        d_out = lk.guarded_device(count * (n + 1))
        keys_only = e_small.memory_bytes()
        e.timer_begin(st)
        e.gate_batch_dev(R.NAND, d0, d1, d_out, count, st)
        detail = e.timer_end_detail(st)
        _split_path_taken(e, detail, count, N, label, keys_only)

        def call(s, d_chunk, cnt):
            e_small.gate_batch_dev(R.NAND, s[0], s[1], d_chunk, cnt, st)
            e_small.sync(st)
        lk.same_as_chunks(call, [(d0, n + 1), (d1, n + 1)], (d_out, n + 1), count, _chunk_samples(N))
        assert e_small.memory_bytes() - keys_only <= 1 << 30, "the slice calls' sample buffer stayed below 2^30 bytes"
        pick = lk.probe_items(count, (N + 1) * 4, lk.ks_segment(N))
        c0, c1 = lk.rows_of(d0, n + 1, pick), lk.rows_of(d1, n + 1, pick)
        if exact:
            exp = orc.gate_batch_mt(w.P, orc.NAND, None, w.K.bk_t, w.K.ksk, c0, c1, nthreads=gk.THREADS, backend=orc.BACKEND_EXACT)[0]
        else:
            exp = orc.gate_batch_mt(w.P, orc.NAND, w.K.bk_f, None, w.K.ksk, c0, c1, nthreads=gk.THREADS)[0]
        got = lk.rows_of(d_out, n + 1, pick)
        bad = np.flatnonzero((got != exp).any(axis=1))
        assert bad.size == 0, ("gates that differ from the oracle", pick[bad][:16].tolist())
        lk.check_canary(d_out, count * (n + 1))
        torch.cuda.synchronize()
    finally:
        e.close()
        e_small.close()
        d0 = d1 = d_out = None
        lk.release()


def test_01_gate_batch_three_key_switch_segments_n1024(worlds):
    """row 1: 1,047,552 + 2,048 + 37 gates at N = 1024, n = 2 on the mirror: a 4.3 GB sample buffer, tiles past B31 and B32"""
    _gate_batch(worlds, 1024, 1047552 + 2048 + 37, None, False, "01 gate_batch_dev N=1024")


def test_02_gate_batch_three_key_switch_segments_n2048(worlds):
    """row 2: 524,032 + 512 + 37 gates at N = 2048, n = 2 on the mirror: the same span in tiles of 131,136 bytes"""
    _gate_batch(worlds, 2048, 524032 + 512 + 37, None, False, "02 gate_batch_dev N=2048")


@pytest.mark.parametrize("backend", ["NTT_EXACT", "FFT_SPLIT_EXACT"])
def test_03_gate_batch_two_key_switch_segments_exact_backends(worlds, backend):
    """row 3: 523,776 + 1,061 gates at N = 1024, n = 2 on both exact backends, against the exact-integer oracle: their own ext_first + gate
    tiling of the sample buffer past B31"""
    import rustfhe_amd as R
    _gate_batch(worlds, 1024, 523776 + 1061, getattr(R._ffi, "BACKEND_" + backend), True, "03 gate_batch_dev " + backend)


# ---- 4: a netlist wave, skipped gates in the second segment ---------------------------------------------------------------------------------
def test_04_netlist_wave_second_segment_with_skipped_gates(worlds):
    """row 4: one wave of 523,776 + 1,061 gates, gate g writing wire 64 + g, five invalid gates in the second key-switch segment: the
    ops / idx + off path of launch_key_switch_mm over an unshifted wire table.  The skipped gates keep their old rows and the next sync
    reports them once."""
    import rustfhe_amd as R
    import torch
    N, count = 1024, 523776 + 1061
    lk.need(-(-count // 16) * _tile_bytes(N) + (1 << 30) + (64 << 20))
    w = worlds(N, 2)
    orc, n = w.orc, w.n
    w1 = n + 1
    seg = lk.ks_segment(N)
    e, e_small = w.engine(), w.engine()
    try:
        st = _stream()
        keys_only = e_small.memory_bytes()
        rng = np.random.default_rng(404)
        inputs = random_words(rng, (IN_ROWS, w1))
        ops = rng.integers(0, orc.ANDNY + 1, count).astype(np.int32)
        i0, i1 = rng.integers(0, IN_ROWS, count).astype(np.int32), rng.integers(0, IN_ROWS, count).astype(np.int32)
        io = (IN_ROWS + np.arange(count)).astype(np.int32)
        W = IN_ROWS + count
        bad = seg + np.array([0, 7, 500, 1000, 1060])
        b = {"ops": ops.copy(), "i0": i0.copy(), "i1": i1.copy(), "io": io.copy()}
        for g, (field, v) in zip(bad.tolist(), [("i0", -1), ("i1", W), ("io", -1), ("ops", 99), ("io", W)]):
            b[field][g] = v
        d_ops, d_i0, d_i1, d_io = (gk.to_device(b[k]) for k in ("ops", "i0", "i1", "io"))
        wires = lk.guarded_device(W * w1)
        wires[:IN_ROWS * w1] = gk.to_device(inputs, np.uint32).reshape(-1)
        e.timer_begin(st)
        e.circuit_wave_dev(d_ops, d_i0, d_i1, d_io, wires, W, count, st)
        detail = e.timer_end_detail(st)
        with pytest.raises(R.RtfheError) as ei:
            e.sync(st)
        assert ei.value.code == R._ffi.ERR_INVALID
        e.sync(st)                                   # reported once
        _split_path_taken(e, detail, count, N, "04 circuit_wave_dev", keys_only)

        small = lk.guarded_device((IN_ROWS + _chunk_samples(N)) * w1)
        small[:IN_ROWS * w1] = wires[:IN_ROWS * w1]
        fill = int(np.uint32(gk.FILL).view(np.int32))
        raised = []

        def call(s, d_chunk, cnt):
            small[IN_ROWS * w1:].fill_(fill)
            local = torch.arange(IN_ROWS, IN_ROWS + cnt, dtype=torch.int32, device="cuda")
            d_lio = torch.where((s[3] >= IN_ROWS) & (s[3] < W), local, s[3])          # a bad index (-1 or W) stays bad in the smaller table
            e_small.circuit_wave_dev(s[0], s[1], s[2], d_lio, small, IN_ROWS + cnt, cnt, st)
            try:
                e_small.sync(st)
            except R.RtfheError as err:
                assert err.code == R._ffi.ERR_INVALID
                raised.append(cnt)
            d_chunk[:cnt * w1] = small[IN_ROWS * w1:(IN_ROWS + cnt) * w1]
        chunk = _chunk_samples(N)
        lk.same_as_chunks(call, [(d_ops, 1), (d_i0, 1), (d_i1, 1), (d_io, 1)], (wires[IN_ROWS * w1:], w1), count, chunk)
        assert len(raised) == len({int(g) // chunk for g in bad}), "exactly the slices with a skipped gate reported one"

        pick = np.unique(np.concatenate([lk.probe_items(count, (N + 1) * 4, seg), bad - 1, bad, bad + 1]))
        pick = pick[pick < count]                    # (the last skipped gate is the wave's last)
        good = ~np.isin(pick, bad)
        got = lk.rows_of(wires, w1, pick, IN_ROWS * w1)
        assert (got[~good] == gk.FILL).all(), "a skipped gate's wire row keeps its old words"
        gp = pick[good]
        exp = gk.pmap(lambda g: orc.gate(w.P, gk.oracle_plan(orc, N), int(ops[g]), w.K.bk_f, None, w.K.ksk, inputs[i0[g]], inputs[i1[g]]), gp.tolist())
        diff = np.flatnonzero((got[good] != np.stack(exp)).any(axis=1))
        assert diff.size == 0, ("gates that differ from the oracle", gp[diff][:16].tolist())
        assert np.array_equal(lk.rows_of(wires, w1, np.arange(IN_ROWS)), inputs), "the input rows are unchanged"
        lk.check_canary(wires, W * w1)
    finally:
        e.close()
        e_small.close()
        wires = small = None
        lk.release()


# ---- 5: many-LUT PBS, count << 3 rows of samples -----------------------------------------------------------------------------------------
def test_05_pbs_many_eight_outputs(worlds):
    """row 5: 131,072 + 300 gates with n_out = 8 at N = 1024, n = 2: sample rows (gate << 3) + j up to 1,050,975, three key-switch segments"""
    import torch
    N, count, n_out = 1024, 131072 + 300, 8
    lk.need(-(-count * n_out // 16) * _tile_bytes(N) + (1 << 30) + (64 << 20))
    w = worlds(N, 2)
    orc, n = w.orc, w.n
    rows, ow = count * n_out, n_out * (n + 1)
    e, e_small = w.engine(), w.engine()
    try:
        st = _stream()
        keys_only = e_small.memory_bytes()
        tv = random_words(np.random.default_rng(505), (3, N))
        d_ct = lk.device_words(count * (n + 1), 505)
        d_idx = torch.randint(0, 3, (count,), dtype=torch.int32, device="cuda", generator=torch.Generator(device="cuda").manual_seed(506))
        d_out = lk.guarded_device(count * ow)
        with e.lut(tv) as lut, e_small.lut(tv) as lut_small:
            e.timer_begin(st)
            e.pbs_many_batch_dev(lut, d_ct, d_out, count, n_out, d_idx, st)
            detail = e.timer_end_detail(st)
            e.sync(st)
            _split_path_taken(e, detail, rows, N, "05 pbs_many_batch_dev", keys_only)

            def call(s, d_chunk, cnt):
                e_small.pbs_many_batch_dev(lut_small, s[0], d_chunk, cnt, n_out, s[1], st)
                e_small.sync(st)
            lk.same_as_chunks(call, [(d_ct, n + 1), (d_idx, 1)], (d_out, ow), count, _chunk_samples(N) // n_out)
        gates = np.unique(lk.probe_items(rows, (N + 1) * 4, lk.ks_segment(N)) // n_out)
        ct, idx = lk.rows_of(d_ct, n + 1, gates), lk.rows_of(d_idx, 1, gates).view(np.int32).reshape(-1)
        exp = gk.pmap(lambda k: oracle_pbs_many(orc, w.P, gk.oracle_plan(orc, N), w.K.bk_f, w.K.ksk, tv[idx[k]], ct[k], n_out).reshape(-1), range(len(gates)))
        diff = np.flatnonzero((lk.rows_of(d_out, ow, gates) != np.stack(exp)).any(axis=1))
        assert diff.size == 0, ("gates that differ from the oracle", gates[diff][:16].tolist())
        lk.check_canary(d_out, count * ow)
    finally:
        e.close()
        e_small.close()
        d_ct = d_idx = d_out = None
        lk.release()


# ---- 6-8: TRLWE sample extraction ------------------------------------------------------------------------------------------------------------
def test_06_trlwe_extract_with_key_switch(worlds):
    """row 6: 1,026 TRLWEs, all N = 1024 coefficients each, at n = 8: 1,050,624 samples in the sample buffer (two coefficient launches of 512,
    three key-switch segments)"""
    N, count = 1024, 1026
    lk.need(-(-count * N // 16) * _tile_bytes(N) + (1 << 30) + 8 * count * N + 4 * count * N * 9)
    w = worlds(N, 8)
    orc, n = w.orc, w.n
    M, ow = count * N, N * (n + 1)
    e, e_small = w.engine(), w.engine()
    try:
        st = _stream()
        keys_only = e_small.memory_bytes()
        d_in = lk.device_words(count * 2 * N, 606)
        d_out = lk.guarded_device(count * ow)
        e.timer_begin(st)
        e.trlwe_extract_batch_dev(d_in, N, d_out, count, None, 1, st)
        detail = e.timer_end_detail(st)
        e.sync(st)
        _split_path_taken(e, detail, M, N, "06 trlwe_extract_batch_dev", keys_only)

        def call(s, d_chunk, cnt):
            e_small.trlwe_extract_batch_dev(s[0], N, d_chunk, cnt, None, 1, st)
            e_small.sync(st)
        lk.same_as_chunks(call, [(d_in, 2 * N)], (d_out, ow), count, _chunk_samples(N) // N)
        pick = lk.probe_items(M, (N + 1) * 4, lk.ks_segment(N))
        gs = np.unique(pick // N)
        x = dict(zip(gs.tolist(), lk.rows_of(d_in, 2 * N, gs)))
        exp = gk.pmap(lambda s: orc.key_switch(w.P, w.K.ksk, orc.sample_extract(w.P, x[s // N], s % N)), pick.tolist())
        diff = np.flatnonzero((lk.rows_of(d_out, n + 1, pick) != np.stack(exp)).any(axis=1))
        assert diff.size == 0, ("samples that differ from the oracle", pick[diff][:16].tolist())
        lk.check_canary(d_out, count * ow)
    finally:
        e.close()
        e_small.close()
        d_in = d_out = None
        lk.release()


def _bare_engine(N, n=2):
    import rustfhe_amd as R
    return R.Engine(R.Params(n=n, N=N), 0)


def _extract_lvl1(N, count, P, coef, label):
    """the lvl1 form: no key, no scratch; output [count * P][N + 1]"""
    M, w1 = count * P, N + 1
    lk.need(4 * (count * 2 * N + M * w1) + (2 << 30))
    e = _bare_engine(N)
    try:
        st = _stream()
        d_in = lk.device_words(count * 2 * N, 700 + N)
        d_out = lk.guarded_device(M * w1)
        e.trlwe_extract_lvl1_batch_dev(d_in, P, d_out, count, coef, 1, st)
        e.sync(st)
        lk.report(label, e)

        def call(s, d_chunk, cnt):
            e.trlwe_extract_lvl1_batch_dev(s[0], P, d_chunk, cnt, coef, 1, st)
            e.sync(st)
        lk.same_as_chunks(call, [(d_in, 2 * N)], (d_out, P * w1), count, (1 << 30) // max(8 * N, 4 * P * w1))
        # the far array may be the input (rows of 8 N bytes) or the output (samples of 4 (N + 1) bytes): the probes of both
        pick = np.unique(np.concatenate([lk.probe_items(M, 4 * w1), lk.probe_items(count, 8 * N) * P, lk.probe_items(count, 8 * N) * P + P - 1]))
        gs = np.unique(pick // P)
        x = dict(zip(gs.tolist(), lk.rows_of(d_in, 2 * N, gs)))
        cf = np.arange(P) if coef is None else np.asarray(coef)
        exp = np.stack([extract_formula(x[s // P], N, int(cf[s % P])) for s in pick.tolist()])
        diff = np.flatnonzero((lk.rows_of(d_out, w1, pick) != exp).any(axis=1))
        assert diff.size == 0, ("samples that differ from sample_extract_index", pick[diff][:16].tolist())
        lk.check_canary(d_out, M * w1)
    finally:
        e.close()
        d_in = d_out = None
        lk.release()


def test_07_trlwe_extract_lvl1_far_output():
    """row 7: 2,050 TRLWEs, all 1,024 coefficients each: the output [2,099,200][1,025] is 8.6 GB -- B31, B32 and W31"""
    _extract_lvl1(1024, 2050, 1024, None, "07 trlwe_extract_lvl1_batch_dev far output")


def test_08_trlwe_extract_lvl1_far_input():
    """row 8: 1,048,576 + 3 TRLWEs at N = 2048, coefficient N - 1 of each: the input is 17.2 GB -- all four boundaries -- and the output, one
    sample of 2,049 words per row, another 8.6 GB (B31, B32, W31)"""
    _extract_lvl1(2048, 1048576 + 3, 1, [2047], "08 trlwe_extract_lvl1_batch_dev far input")


# ---- 9, 10: compressed results -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [10, 3])
def test_09_trlwe_compress_far_input(k):
    """row 9: 524,288 + 3 TRLWEs at N = 2048, P = 1: an 8.6 GB input (B31, B32, W31; the count * L < 2^31 rule stops below W32)"""
    N, count, P = 2048, 524288 + 3, 1
    W = co.words(N + P, k)
    lk.need(4 * count * (2 * N + W) + (2 << 30))
    e = _bare_engine(N)
    try:
        st = _stream()
        d_in = lk.device_words(count * 2 * N, 900 + k)
        d_out = lk.guarded_device(count * W)
        e.trlwe_compress_dev(d_in, k, P, d_out, count, None, 1, st)
        e.sync(st)
        lk.report("09 trlwe_compress_dev k=%d" % k, e)

        def call(s, d_chunk, cnt):
            e.trlwe_compress_dev(s[0], k, P, d_chunk, cnt, None, 1, st)
            e.sync(st)
        lk.same_as_chunks(call, [(d_in, 2 * N)], (d_out, W), count, (1 << 30) // (8 * N))
        pick = lk.probe_items(count, 8 * N)
        exp = co.trlwe_compress(lk.rows_of(d_in, 2 * N, pick).reshape(-1, 2, N), k, P)
        diff = np.flatnonzero((lk.rows_of(d_out, W, pick) != exp).any(axis=1))
        assert diff.size == 0, ("rows that differ from the oracle", pick[diff][:16].tolist())
        lk.check_canary(d_out, count * W)
    finally:
        e.close()
        d_in = d_out = None
        lk.release()


def test_10_tlwe_compress_far_input():
    """row 10: 1,398,102 + 3 lvl0 rows at n = 767 (3,072 bytes each), k = 10: a 4.3 GB input (B31, B32)"""
    n, k, count = 767, 10, 1398102 + 3
    W = co.words(n + 1, k)
    lk.need(4 * count * (n + 1 + W) + (2 << 30))
    e = _bare_engine(1024, n)
    try:
        st = _stream()
        d_in = lk.device_words(count * (n + 1), 1010)
        d_out = lk.guarded_device(count * W)
        e.tlwe_compress_dev(d_in, k, d_out, count, st)
        e.sync(st)
        lk.report("10 tlwe_compress_dev", e)

        def call(s, d_chunk, cnt):
            e.tlwe_compress_dev(s[0], k, d_chunk, cnt, st)
            e.sync(st)
        lk.same_as_chunks(call, [(d_in, n + 1)], (d_out, W), count, (1 << 30) // (4 * (n + 1)))
        pick = lk.probe_items(count, 4 * (n + 1))
        exp = co.tlwe_compress(lk.rows_of(d_in, n + 1, pick), k)
        diff = np.flatnonzero((lk.rows_of(d_out, W, pick) != exp).any(axis=1))
        assert diff.size == 0, ("rows that differ from the oracle", pick[diff][:16].tolist())
        lk.check_canary(d_out, count * W)
    finally:
        e.close()
        d_in = d_out = None
        lk.release()


# ---- 18, 19: seeded expansion --------------------------------------------------------------------------------------------------------------
def test_18_seeded_expand_far_output():
    """row 18: 524,288 + 3 TRLWE rows at N = 1024, group = 1: the output [rows][2][1][N] is 4.3 GB (B31, B32), the b halves 2.1 GB (B31)"""
    N, rows, first = 1024, 524288 + 3, (1 << 32) - 100000
    lk.need(4 * rows * 3 * N + (2 << 30))
    e = _bare_engine(N)
    try:
        st = _stream()
        seed = random_words(np.random.default_rng(1818), 8)
        d_b = lk.device_words(rows * N, 1818)
        d_out = lk.guarded_device(rows * 2 * N)
        e.seeded_expand_dev(seed, d_b, 1, d_out, rows, first, st)
        e.sync(st)
        lk.report("18 seeded_expand_dev", e)

        def call(s, d_chunk, cnt):
            off = (s[0].data_ptr() - d_b.data_ptr()) // (4 * N)
            e.seeded_expand_dev(seed, s[0], 1, d_chunk, cnt, first + off, st)
            e.sync(st)
        lk.same_as_chunks(call, [(d_b, N)], (d_out, 2 * N), rows, (1 << 30) // (8 * N))
        pick = np.unique(np.concatenate([lk.probe_items(rows, 8 * N), lk.probe_items(rows, 4 * N)]))
        b = lk.rows_of(d_b, N, pick)
        exp = np.stack([so.expand(N, seed, first + int(r), b[i], 1).reshape(-1) for i, r in enumerate(pick.tolist())])
        diff = np.flatnonzero((lk.rows_of(d_out, 2 * N, pick) != exp).any(axis=1))
        assert diff.size == 0, ("rows that differ from the oracle", pick[diff][:16].tolist())
        lk.check_canary(d_out, rows * 2 * N)
    finally:
        e.close()
        d_b = d_out = None
        lk.release()


def test_19_tlwe_seeded_expand_far_output():
    """row 19: 1,398,102 + 3 lvl0 rows at n = 767: the output [rows][768] is 4.3 GB (B31, B32)"""
    n, rows, first = 767, 1398102 + 3, (1 << 32) - 700000
    lk.need(4 * rows * (n + 2) + (2 << 30))
    e = _bare_engine(1024, n)
    try:
        st = _stream()
        seed = random_words(np.random.default_rng(1919), 8)
        d_b = lk.device_words(rows, 1919)
        d_out = lk.guarded_device(rows * (n + 1))
        e.tlwe_seeded_expand_dev(seed, d_b, d_out, rows, first, st)
        e.sync(st)
        lk.report("19 tlwe_seeded_expand_dev", e)

        def call(s, d_chunk, cnt):
            off = (s[0].data_ptr() - d_b.data_ptr()) // 4
            e.tlwe_seeded_expand_dev(seed, s[0], d_chunk, cnt, first + off, st)
            e.sync(st)
        lk.same_as_chunks(call, [(d_b, 1)], (d_out, n + 1), rows, (1 << 30) // (4 * (n + 1)))
        pick = lk.probe_items(rows, 4 * (n + 1))
        b = lk.rows_of(d_b, 1, pick).reshape(-1)
        exp = np.stack([tso.expand(n, seed, first + int(r), b[i:i + 1])[0] for i, r in enumerate(pick.tolist())])
        diff = np.flatnonzero((lk.rows_of(d_out, n + 1, pick) != exp).any(axis=1))
        assert diff.size == 0, ("rows that differ from the oracle", pick[diff][:16].tolist())
        lk.check_canary(d_out, rows * (n + 1))
    finally:
        e.close()
        d_b = d_out = None
        lk.release()


# ---- 11, 12, 16: the leveled kernels over a selector set (no key) ----------------------------------------------------------------------------
N_SEL = 8


class Leveled:
    """a selector set of N_SEL random bits under a key of the product's keygen, the oracle's spectra of it, and contexts that hold it"""

    def __init__(self, orc, N):
        self.w, _ = lv.selector_world(orc, N, 0x1A26E + N, 11 * N, N_SEL, 0x5E1 + N, n=8)
        self.orc, self.N = orc, N

    def engine(self):
        e = self.w.R.Engine(self.w.rp, 0)
        return e, e.selectors(self.w.sel_t)


@pytest.fixture(scope="module")
def leveled(orc):
    return gk.Worlds(lambda N: Leveled(orc, N), close=lambda w: None)


def _random_idx(shape, high, seed):
    import torch
    return torch.randint(0, high, shape, dtype=torch.int32, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed))


def _rotate(leveled, N, count, in_place, label):
    """one step of k_trgsw_rotate per row (depth 1, X^-1): rows [count][2][N] in, the same shape out"""
    import torch
    lk.need(4 * count * 2 * N * 2 + (2 << 30))
    L = leveled(N)
    w, orc, row = L.w, L.orc, 2 * N
    e, sel = L.engine()
    try:
        st = _stream()
        d_in = lk.device_words(count * row, 1100 + N)
        d_idx = _random_idx((count, 1), N_SEL, 1101 + N)
        if in_place:
            d_out = lk.guarded_device(count * row)
            d_out[:count * row] = d_in                      # d_in keeps the rows the call reads: the in-place buffer is d_out
            e.trgsw_rotate_batch_dev(sel, d_out, 1, d_out, count, d_idx, None, st)
        else:
            d_out = lk.guarded_device(count * row)
            e.trgsw_rotate_batch_dev(sel, d_in, 1, d_out, count, d_idx, None, st)
        e.sync(st)
        lk.report(label, e)

        def call(s, d_chunk, cnt):
            if in_place:
                d_chunk[:cnt * row] = s[0]
            e.trgsw_rotate_batch_dev(sel, d_chunk if in_place else s[0], 1, d_chunk, cnt, s[1], None, st)
            e.sync(st)
        lk.same_as_chunks(call, [(d_in, row), (d_idx, 1)], (d_out, row), count, (1 << 30) // (4 * row))
        pick = lk.probe_items(count, 4 * row)
        x, idx = lk.rows_of(d_in, row, pick), lk.rows_of(d_idx, 1, pick).view(np.int32)
        exp = gk.pmap(lambda k: oracle_trgsw_rotate(orc, w.P, gk.oracle_plan(orc, N), w.sel_f, idx[k], None, x[k]).reshape(-1), range(len(pick)))
        diff = np.flatnonzero((lk.rows_of(d_out, row, pick) != np.stack(exp)).any(axis=1))
        assert diff.size == 0, ("rows that differ from the oracle", pick[diff][:16].tolist())
        lk.check_canary(d_out, count * row)
        torch.cuda.synchronize()
    finally:
        sel.close()
        e.close()
        d_in = d_out = d_idx = None
        lk.release()


def test_11_trgsw_rotate_out_of_place(leveled):
    """row 11: 524,288 + 3 rows at N = 1024, depth 1: input and output rows past B31 and B32"""
    _rotate(leveled, 1024, 524288 + 3, False, "11 trgsw_rotate_batch_dev out of place")


def test_12_trgsw_rotate_in_place(leveled):
    """row 12: 524,288 + 3 rows at N = 2048, depth 1, d_out == d_trlwe: one 8.6 GB buffer, B31, B32 and W31 (a copy of the rows stands
    beside it for the oracle and the slices)"""
    _rotate(leveled, 2048, 524288 + 3, True, "12 trgsw_rotate_batch_dev in place")


def test_16_demux_tree_far_leaves(leveled):
    """row 16: 2,048 + 3 lookups of depth 8 at N = 1024: 256 leaves each, the output [count][256][2][N] is 4.3 GB (B31, B32); the level
    buffers of the big call hold count * 128 nodes, 2.1 GB each"""
    N, count, depth = 1024, 2048 + 3, 8
    lk.need(4 * count * (1 << depth) * 2 * N * 2 + (3 << 30))
    L = leveled(N)
    w, orc, row = L.w, L.orc, 2 * N
    leaves = 1 << depth
    e, sel = L.engine()
    e_small, sel_small = L.engine()
    try:
        st = _stream()
        d_x = lk.device_words(count * row, 1600)
        d_idx = _random_idx((count, depth), N_SEL, 1601)
        d_out = lk.guarded_device(count * leaves * row)
        e.demux_tree_batch_dev(sel, d_x, depth, d_out, count, d_idx, st)
        e.sync(st)
        lk.report("16 demux_tree_batch_dev", e)

        def call(s, d_chunk, cnt):
            e_small.demux_tree_batch_dev(sel_small, s[0], depth, d_chunk, cnt, s[1], st)
            e_small.sync(st)
        lk.same_as_chunks(call, [(d_x, row), (d_idx, depth)], (d_out, leaves * row), count, (1 << 30) // (4 * leaves * row))
        rows = lk.probe_items(count * leaves, 4 * row)
        gs = np.unique(rows // leaves)
        x, idx = lk.rows_of(d_x, row, gs), lk.rows_of(d_idx, depth, gs).view(np.int32)
        exp = gk.pmap(lambda k: oracle_demux_tree(orc, w.P, gk.oracle_plan(orc, N), w.sel_f, idx[k], x[k]).reshape(-1), range(len(gs)))
        diff = np.flatnonzero((lk.rows_of(d_out, leaves * row, gs) != np.stack(exp)).any(axis=1))
        assert diff.size == 0, ("lookups that differ from the oracle", gs[diff][:16].tolist())
        lk.check_canary(d_out, count * leaves * row)
    finally:
        for h in (sel, sel_small, e, e_small):
            h.close()
        d_x = d_out = d_idx = None
        lk.release()


# ---- 13, 14: the two sums of products over TRLWE rows ---------------------------------------------------------------------------------------
N_W = 4


def _products(leveled, N, kind):
    """(engine, the small operand's handle, launch(d_x, n_x, d_out, count, K, d_small_idx, d_x_idx, accumulate, st), oracle(x rows, small idx,
    x idx, acc) -> u32[count][2][N])"""
    L = leveled(N)
    w, orc = L.w, L.orc
    if kind == "plain":
        e = w.R.Engine(w.rp, 0)
        wts = pmo.weights(1300 + N, N, N_W, 3 * N)
        h = e.plain_polys(wts)
        launch = lambda d_x, n_x, d_out, count, K, d_s, d_xi, acc, st: e.trlwe_mul_plain_batch_dev(h, d_x, n_x, d_out, count, K, d_s, d_xi, acc, st)  # noqa: E731
        oracle = lambda x, s_idx, x_idx, acc: pmo.mul_plain(wts, x, s_idx.shape[1], s_idx, x_idx, acc)  # noqa: E731
        return e, h, launch, oracle, N_W
    e, h = L.engine()
    launch = lambda d_x, n_x, d_out, count, K, d_s, d_xi, acc, st: e.trlwe_mul_trgsw_batch_dev(h, d_x, n_x, d_out, count, K, d_s, d_xi, acc, st)  # noqa: E731
    oracle = lambda x, s_idx, x_idx, acc: tmo.mac(w.P, gk.oracle_plan(orc, N), w.sel_f, s_idx, x, x_idx, acc, ro.REFERENCE)  # noqa: E731
    return e, h, launch, oracle, N_SEL


@pytest.mark.parametrize("kind", ["plain", "trgsw"])
def test_13_sums_of_products_far_x(leveled, kind):
    """row 13: x of 1,048,576 + 4 rows at N = 2048 (17.2 GB: all four boundaries), 64 samples of K = 2 whose x_idx name row 0, the last row
    and the rows either side of every boundary.  The second opinion is the same call on the named rows gathered into a small x."""
    import torch
    N, n_x, count, K = 2048, 1048576 + 4, 64, 2
    row = 2 * N
    lk.need(4 * n_x * row + (2 << 30))
    e, h, launch, oracle, n_small = _products(leveled, N, kind)
    try:
        st = _stream()
        d_x = lk.device_words(n_x * row, 1313)
        b = lk.boundaries(4 * row)
        named = sorted({0, n_x - 1} | {b[k] - 1 for k in lk.NAMES} | {b[k] for k in lk.NAMES})
        assert len(named) == 10 and lk.crossed(n_x, 4 * row) == list(lk.NAMES)
        rng = np.random.default_rng(1314)
        pool = np.array(named + rng.integers(0, n_x, 22).tolist(), np.int64)
        x_idx = pool[rng.integers(0, pool.size, (count, K))]
        x_idx[:10, 0], x_idx[:10, 1] = named, named[1:] + named[:1]
        s_idx = rng.integers(0, n_small, (count, K))
        d_s, d_xi = gk.to_device(s_idx), gk.to_device(x_idx)
        d_out = lk.guarded_device(count * row)
        launch(d_x, n_x, d_out, count, K, d_s, d_xi, False, st)
        e.sync(st)
        lk.report("13 %s far x" % kind, e)
        used, local = np.unique(x_idx, return_inverse=True)
        d_small = d_x.view(n_x, row)[torch.from_numpy(used).cuda()].contiguous()
        d_again = lk.guarded_device(count * row)
        launch(d_small, used.size, d_again, count, K, d_s, gk.to_device(local.reshape(count, K)), False, st)
        e.sync(st)
        assert torch.equal(d_out, d_again), "the far rows give other words than the same rows gathered into a small x"
        exp = oracle(gk.words_of(d_small).reshape(-1, 2, N), s_idx, local.reshape(count, K), None)
        assert np.array_equal(lk.rows_of(d_out, row, np.arange(count)), exp.reshape(count, row))
        lk.check_canary(d_out, count * row)
    finally:
        h.close()
        e.close()
        d_x = d_out = d_small = d_again = None
        lk.release()


@pytest.mark.parametrize("accumulate", [False, True], ids=["store", "accumulate"])
@pytest.mark.parametrize("kind", ["plain", "trgsw"])
def test_14_sums_of_products_far_output(leveled, kind, accumulate):
    """row 14: 524,288 + 3 samples of K = 1 at N = 1024 reading 64 rows of x: the output rows pass B31 and B32; accumulate off and on (on: the
    output starts as random words, kept in a second buffer for the slices and the oracle)"""
    N, n_x, count, K = 1024, 64, 524288 + 3, 1
    row = 2 * N
    lk.need(4 * count * row * (2 if accumulate else 1) + (2 << 30))
    e, h, launch, oracle, n_small = _products(leveled, N, kind)
    try:
        st = _stream()
        d_x = lk.device_words(n_x * row, 1414)
        d_s, d_xi = _random_idx((count, K), n_small, 1415), _random_idx((count, K), n_x, 1416)
        d_out = lk.guarded_device(count * row)
        d_acc = lk.device_words(count * row, 1417) if accumulate else None
        if accumulate:
            d_out[:count * row] = d_acc
        launch(d_x, n_x, d_out, count, K, d_s, d_xi, accumulate, st)
        e.sync(st)
        lk.report("14 %s far output%s" % (kind, ", accumulate" if accumulate else ""), e)

        def call(s, d_chunk, cnt):
            if accumulate:
                d_chunk[:cnt * row] = s[2]
            launch(d_x, n_x, d_chunk, cnt, K, s[0], s[1], accumulate, st)
            e.sync(st)
        lk.same_as_chunks(call, [(d_s, K), (d_xi, K), (d_acc, row) if accumulate else None], (d_out, row), count, (1 << 30) // (4 * row))
        pick = lk.probe_items(count, 4 * row)
        s_idx, x_idx = lk.rows_of(d_s, K, pick).view(np.int32), lk.rows_of(d_xi, K, pick).view(np.int32)
        acc = lk.rows_of(d_acc, row, pick).reshape(-1, 2, N) if accumulate else None
        exp = oracle(gk.words_of(d_x).reshape(n_x, 2, N), s_idx, x_idx, acc)
        diff = np.flatnonzero((lk.rows_of(d_out, row, pick) != exp.reshape(len(pick), row)).any(axis=1))
        assert diff.size == 0, ("samples that differ from the oracle", pick[diff][:16].tolist())
        lk.check_canary(d_out, count * row)
    finally:
        h.close()
        e.close()
        d_x = d_out = d_acc = None
        lk.release()


# ---- 20, 21: dense layers, table accumulation ------------------------------------------------------------------------------------------------
def test_20_dense_far_x():
    """row 20: 21,900 samples of I = 64 inputs, O = 16 outputs at n = 767: x is 4.3 GB (B31, B32), the output 1.07 GB"""
    n, I, O, count = 767, 64, 16, 21900
    w1 = n + 1
    lk.need(4 * count * (I + O) * w1 + (2 << 30))
    e = _bare_engine(1024, n)
    W = do.weights(2020, O, I)
    d = e.dense(W)
    try:
        st = _stream()
        d_x = lk.device_words(count * I * w1, 2021)
        d_out = lk.guarded_device(count * O * w1)
        e.tlwe_dense_batch_dev(d, d_x, d_out, count, None, False, st)
        e.sync(st)
        lk.report("20 tlwe_dense_batch_dev", e)

        def call(s, d_chunk, cnt):
            e.tlwe_dense_batch_dev(d, s[0], d_chunk, cnt, None, False, st)
            e.sync(st)
        lk.same_as_chunks(call, [(d_x, I * w1)], (d_out, O * w1), count, (1 << 30) // (4 * I * w1))
        pick = lk.probe_items(count, 4 * I * w1)
        exp = do.dense(W, lk.rows_of(d_x, I * w1, pick).reshape(-1, I, w1))
        diff = np.flatnonzero((lk.rows_of(d_out, O * w1, pick) != exp.reshape(len(pick), -1)).any(axis=1))
        assert diff.size == 0, ("samples that differ from the oracle", pick[diff][:16].tolist())
        lk.check_canary(d_out, count * O * w1)
    finally:
        d.close()
        e.close()
        d_x = d_out = None
        lk.release()


def test_21_accumulate_far_source():
    """row 21: 8,192 + 3 sources of 64 rows added into rows 0 .. 63 of an encrypted table at N = 1024: the source [count][64][2][N] is 4.3 GB.
    Every source word enters one sum, so the reference is the wrapping sum itself, made on the device in 64-bit integers piece by piece, and
    the second opinion the same table filled by slices of the source."""
    import torch
    N, rows, count = 1024, 64, 8192 + 3
    words = rows * 2 * N
    lk.need(4 * count * words + (3 << 30))
    e = _bare_engine(N)
    start = random_words(np.random.default_rng(2121), (rows, 2, N))
    try:
        st = _stream()
        d_src = lk.device_words(count * words, 2122)
        assert lk.crossed(count, 4 * words) == ["B31", "B32"]
        d_got, d_again = lk.guarded_device(words), lk.guarded_device(words)
        with e.lut_encrypted(start) as table, e.lut_encrypted(start) as sliced:
            table.accumulate_dev(d_src, 0, rows, count, st)
            table.read_dev(d_got, 0, rows, st)
            chunk = (1 << 30) // (4 * words)
            for off in range(0, count, chunk):
                cnt = min(chunk, count - off)
                sliced.accumulate_dev(d_src[off * words:(off + cnt) * words], 0, rows, cnt, st)
            sliced.read_dev(d_again, 0, rows, st)
            e.sync(st)
        lk.report("21 accumulate_dev", e)
        assert torch.equal(d_got, d_again), "the far sources give another sum than the same sources added slice by slice"
        total = gk.to_device(start, np.uint32).reshape(-1).to(torch.int64)
        for off in range(0, count, 512):
            total += d_src[off * words:min(off + 512, count) * words].view(-1, words).sum(dim=0, dtype=torch.int64)
        want = (total & 0xFFFFFFFF).cpu().numpy().astype(np.uint32)
        assert np.array_equal(gk.words_of(d_got[:words]), want), "the table rows are not start + the wrapping sum of every source"
        # the far end alone, word for word on the host: the last 32 sources, and 32 around every boundary the source crosses (a window that would
        # pass the end of the source is moved back: it still holds its boundary)
        marks = [lk.boundaries(4 * words)[name] for name in lk.crossed(count, 4 * words)]
        for first, mark in [(count - 32, count - 1)] + [(min(m - 16, count - 32), m) for m in marks]:
            assert 0 <= first <= mark < first + 32 <= count
            part = lk.rows_of(d_src, words, np.arange(first, first + 32))
            with e.lut_encrypted(start) as t:
                t.accumulate_dev(d_src[first * words:], 0, rows, 32, st)
                t.read_dev(d_again, 0, rows, st)
                e.sync(st)
            assert np.array_equal(gk.words_of(d_again[:words]), (start.reshape(-1) + part.sum(axis=0, dtype=np.uint32)).astype(np.uint32)), first
        lk.check_canary(d_got, words)
    finally:
        e.close()
        d_src = d_got = d_again = None
        lk.release()


# ---- 17: the packing key switch ----------------------------------------------------------------------------------------------------------------
def test_17_pack_far_output():
    """row 17: 524,288 + 3 lvl0 ciphertexts at n = 8 packed one per row (P = 1) at N = 1024: the output rows, and the key-switched samples
    S[count][2 N] between the two launches in the context, pass B31 and B32"""
    import rustfhe_amd as R
    N, n, count = 1024, 8, 524288 + 3
    row = 2 * N
    lk.need(4 * count * row * 2 + (3 << 30))
    rp = R.Params(n=n, N=N)
    key0, key1, _, _ = R.keygen(rp, 0x17AC, want_bk=False)
    pk = R.packing_keygen(rp, key0, key1, 0x17AD)
    e, e_small = R.Engine(rp, 0), R.Engine(rp, 0)
    key, key_small = e.packing_key(pk), e_small.packing_key(pk)
    try:
        st = _stream()
        d_in = lk.device_words(count * (n + 1), 1717)
        d_out = lk.guarded_device(count * row)
        e.pack_batch_dev(key, d_in, 1, d_out, count, 1, None, st)
        e.sync(st)
        lk.report("17 pack_batch_dev", e)

        def call(s, d_chunk, cnt):
            e_small.pack_batch_dev(key_small, s[0], 1, d_chunk, cnt, 1, None, st)
            e_small.sync(st)
        lk.same_as_chunks(call, [(d_in, n + 1)], (d_out, row), count, (1 << 30) // (4 * row))
        pick = lk.probe_items(count, 4 * row)
        exp = po.pack(rp, pk, lk.rows_of(d_in, n + 1, pick).reshape(-1, 1, n + 1), 1)
        diff = np.flatnonzero((lk.rows_of(d_out, row, pick) != exp.reshape(len(pick), row)).any(axis=1))
        assert diff.size == 0, ("rows that differ from the oracle", pick[diff][:16].tolist())
        lk.check_canary(d_out, count * row)
    finally:
        for h in (key, key_small, e, e_small):
            h.close()
        d_in = d_out = None
        lk.release()


# ---- 15, 22: the CMUX tree's level buffers, a recorded netlist's node buffer -----------------------------------------------------------------
@pytest.mark.parametrize("extract", [False, True], ids=["trlwe", "extract"])
def test_15_cmux_tree_far_level_buffers(leveled, extract):
    """row 15: 4,096 + 5 lookups of depth 8 into a 256-row table at N = 1024, n = 8: the output is small, the far arrays are the context's
    ping-pong level buffers -- count * 128 nodes, 4.3 GB, after level 0 (B31, B32) -- and, in the extract form, nothing more than 4,101 samples"""
    import torch
    N, count, depth = 1024, 4096 + 5, 8
    lk.need(2 * 4 * count * 128 * 2 * N + (3 << 30))
    L = leveled(N)
    w, orc = L.w, L.orc
    ow = w.rp.n + 1 if extract else 2 * N
    tv = random_words(np.random.default_rng(1515), (1 << depth, N))
    e, sel = L.engine()
    e_small, sel_small = L.engine()
    if extract:
        e.load_ksk(w.ksk)
        e_small.load_ksk(w.ksk)
    lut, lut_small = e.lut(tv), e_small.lut(tv)
    try:
        st = _stream()
        d_idx = _random_idx((count, depth), N_SEL, 1516)
        d_coef = _random_idx((count,), N, 1517)
        d_out = lk.guarded_device(count * ow)

        def run(eng, s, t, d_o, cnt, idx, coef):
            if extract:
                eng.cmux_tree_extract_batch_dev(s, t, depth, d_o, cnt, idx, None, coef, st)
            else:
                eng.cmux_tree_batch_dev(s, t, depth, d_o, cnt, idx, None, st)
            eng.sync(st)
        run(e, sel, lut, d_out, count, d_idx, d_coef)
        held = lk.report("15 cmux_tree%s_batch_dev" % ("_extract" if extract else ""), e)
        print("[large] 15: the two level buffers hold %.2f GB each (not counted by the context's figure %.2f GB)" % (4 * count * 128 * 2 * N / 1e9, held / 1e9))
        lk.same_as_chunks(lambda s, d_chunk, cnt: run(e_small, sel_small, lut_small, d_chunk, cnt, s[0], s[1]), [(d_idx, depth), (d_coef, 1)], (d_out, ow), count,
                          (1 << 30) // (4 * 128 * 2 * N))
        pick = lk.probe_items(count, 4 * 128 * 2 * N)
        idx, coef = lk.rows_of(d_idx, depth, pick).view(np.int32), lk.rows_of(d_coef, 1, pick).view(np.int32).reshape(-1)
        rows = as_trlwe(tv, N)
        exp = gk.pmap(lambda k: oracle_cmux_tree(orc, w.P, gk.oracle_plan(orc, N), w.sel_f, idx[k], rows, int(coef[k]) if extract else None, w.ksk).reshape(-1),
                      range(len(pick)))
        diff = np.flatnonzero((lk.rows_of(d_out, ow, pick) != np.stack(exp)).any(axis=1))
        assert diff.size == 0, ("lookups that differ from the oracle", pick[diff][:16].tolist())
        lk.check_canary(d_out, count * ow)
        torch.cuda.synchronize()
    finally:
        for h in (lut, lut_small, sel, sel_small, e, e_small):
            h.close()
        d_out = d_idx = d_coef = None
        lk.release()


def test_22_recorded_cmux_netlist_far_node_buffer(leveled):
    """row 22: 34,953 replicas of the depth-4 tree netlist (15 nodes) at N = 1024 recorded into one graph: count * n_nodes = 524,295 nodes, the
    node buffer is 4.3 GB (B31, B32).  The slices are circuits of their own over at most 8,192 replicas."""
    import torch
    N, depth = 1024, 4
    import rustfhe_amd as R
    net = R.cmux_tree_netlist(depth)
    count = -(-(524288 + 3) // net.n_nodes)
    row = 2 * N
    assert net.n_nodes == 15 and count * net.n_nodes >= 524288 + 3 and lk.crossed(count * net.n_nodes, 4 * row) == ["B31", "B32"]
    lk.need(4 * count * net.n_nodes * row + (3 << 30))
    L = leveled(N)
    w, orc = L.w, L.orc
    tv = random_words(np.random.default_rng(2222), (1 << depth, N))
    e, sel = L.engine()
    lut = e.lut(tv)
    try:
        st = _stream()
        d_idx = _random_idx((count, depth), N_SEL, 2223)
        d_out = lk.guarded_device(count * row)
        with e.cmux_circuit(net, sel, lut, d_out, count, d_idx, None) as c:
            c.launch(st)
            e.sync(st)
            lk.report("22 cmux_circuit", e)

        def call(s, d_chunk, cnt):
            with e.cmux_circuit(net, sel, lut, d_chunk, cnt, s[0], None) as small:
                small.launch(st)
                e.sync(st)
        lk.same_as_chunks(call, [(d_idx, depth)], (d_out, row), count, (1 << 30) // (4 * net.n_nodes * row))
        pick = lk.probe_items(count, 4 * net.n_nodes * row)
        idx = lk.rows_of(d_idx, depth, pick).view(np.int32)
        rows = as_trlwe(tv, N)
        exp = gk.pmap(lambda k: oracle_cmux_net(orc, w.P, gk.oracle_plan(orc, N), w.sel_f, idx[k], rows, net).reshape(-1), range(len(pick)))
        diff = np.flatnonzero((lk.rows_of(d_out, row, pick) != np.stack(exp)).any(axis=1))
        assert diff.size == 0, ("replicas that differ from the oracle", pick[diff][:16].tolist())
        lk.check_canary(d_out, count * row)
        torch.cuda.synchronize()
    finally:
        for h in (lut, sel, e):
            h.close()
        d_out = d_idx = None
        lk.release()


# ---- 23, 24: a far WIRE TABLE -- the caller's own array of lvl0 rows, under a netlist wave and under a LUT-circuit wave --------------------------
FAR_N, FAR_n = 1024, 127          # rows of 512 bytes: 8.4 million wires are 4.3 GB, and a LUT circuit's host-side checks stay at 34 MB


def _far_wires():
    """(W, the wires a wave reads, the 128 distinct wires it may write) in a table of W = B32 + 69 rows of FAR_n + 1 words: read are wire 0,
    the last wire, the wires either side of B31 and of B32 and ten more; written are 32 below and 32 above B31, 32 below B32 and the 32 before
    the last wire, none of them read"""
    b = lk.boundaries(4 * (FAR_n + 1))
    b31, b32 = b["B31"], b["B32"]
    W = b32 + 69
    assert lk.crossed(W, 4 * (FAR_n + 1)) == ["B31", "B32"]
    read = [0, W - 1, b31 - 1, b31, b32 - 1, b32] + np.random.default_rng(2300).integers(100, b31 - 1000, 10).tolist()
    write = list(range(b31 - 40, b31 - 8)) + list(range(b31 + 8, b31 + 40)) + list(range(b32 - 40, b32 - 8)) + list(range(W - 33, W - 1))
    assert len(set(write)) == 128 and not set(read) & set(write) and max(write) < W
    return W, np.array(read, np.int64), np.array(write, np.int64)


def _small_table(wires, w1, used):
    """the rows `used` (sorted, distinct) of the big table gathered into a table of their own behind canaries, and the map wire -> small row"""
    import torch
    small = lk.guarded_device(used.size * w1)
    small[:used.size * w1] = wires.reshape(-1)[:(wires.numel() // w1) * w1].view(-1, w1)[torch.from_numpy(used).cuda()].reshape(-1)
    return small, {int(u): k for k, u in enumerate(used.tolist())}


def _rest_unchanged(wires, before, w1, written):
    """every word of the big table but the rows `written` still equals its copy `before`; compared on the device"""
    import torch
    idx = torch.from_numpy(np.asarray(written, np.int64)).cuda()
    rows = wires.numel() // w1
    a, b = wires.reshape(-1)[:rows * w1].view(rows, w1), before.reshape(-1)[:rows * w1].view(rows, w1)
    keep = b[idx].clone()
    b[idx] = a[idx]
    same = torch.equal(wires, before)
    b[idx] = keep
    return same


def test_23_netlist_wave_far_wire_table(worlds):
    """row 23 (added by the reading: gate_io's (size_t)i0 * w over the CALLER's wire table, which tests 1-5 keep at 12 MB): a wave of 64 gates
    over a wire table of 4.3 GB at n = 127 whose idx0 / idx1 name wire 0, the last wire and the wires either side of B31 and B32 and whose
    idx_out lies around both boundaries and at the end.  Compared with the same wave on those wires gathered into a small table, with the
    oracle, and the rest of the table with its copy."""
    N, n, G = FAR_N, FAR_n, 64
    w1 = n + 1
    W, read, write = _far_wires()
    lk.need(3 * 4 * W * w1 + (1 << 30))          # the table, its copy, and the random words on their way into it
    w = worlds(N, n)
    orc = w.orc
    e = w.engine()
    try:
        st = _stream()
        wires = lk.guarded_device(W * w1)
        wires[:W * w1] = lk.device_words(W * w1, 2323)
        before = wires.clone()
        rng = np.random.default_rng(2324)
        ops = rng.integers(0, orc.ANDNY + 1, G).astype(np.int32)
        i0, i1 = read[rng.integers(0, read.size, G)], read[rng.integers(0, read.size, G)]
        i0[:6], i1[:6] = read[:6], np.roll(read[:6], 1)            # every named wire is read through both index arrays
        io = write[::2].copy()
        e.circuit_wave_dev(gk.to_device(ops), gk.to_device(i0), gk.to_device(i1), gk.to_device(io), wires, W, G, st)
        e.sync(st)
        lk.report("23 circuit_wave_dev far wire table", e)
        used = np.unique(np.concatenate([i0, i1, io]))
        small, at = _small_table(before, w1, used)
        loc = lambda a: np.array([at[int(v)] for v in a], np.int32)  # noqa: E731
        e.circuit_wave_dev(gk.to_device(ops), gk.to_device(loc(i0)), gk.to_device(loc(i1)), gk.to_device(loc(io)), small, used.size, G, st)
        e.sync(st)
        got = lk.rows_of(wires, w1, io)
        assert np.array_equal(got, lk.rows_of(small, w1, loc(io))), "the far wires give other words than the same wires gathered into a small table"
        x = lk.rows_of(before, w1, used)
        exp = gk.pmap(lambda g: orc.gate(w.P, gk.oracle_plan(orc, N), int(ops[g]), w.K.bk_f, None, w.K.ksk, x[at[int(i0[g])]], x[at[int(i1[g])]]), range(G))
        assert np.array_equal(got, np.stack(exp)), "gates that differ from the oracle"
        assert _rest_unchanged(wires, before, w1, io), "a wire that no gate writes changed (or the canary did)"
        lk.check_canary(small, used.size * w1)
    finally:
        e.close()
        wires = before = small = None
        lk.release()


def test_24_lut_circuit_wave_far_wire_table(worlds):
    """row 24 (added by the reading: the LUT-circuit wire table, k_lut_gather's and k_lut_scatter's own (size_t)i * n1): one wave of 64 nodes,
    fan-in 2, n_out = 2 over the same 4.3 GB table (n + 1 = 128: the 16-byte path): in_idx names wire 0, the last wire and the wires either
    side of B31 and B32, the 128 output rows are scattered around both boundaries and to the end.  Compared with the same circuit on those
    wires gathered into a small table, with the oracle (weighted sums in numpy, then oracle_pbs_many), and the rest of the table with its copy."""
    N, n, G, F, n_out = FAR_N, FAR_n, 64, 2, 2
    w1 = n + 1
    W, read, write = _far_wires()
    lk.need(3 * 4 * W * w1 + (1 << 30))          # the table, its copy, and the random words on their way into it
    w = worlds(N, n)
    orc = w.orc
    e = w.engine()
    try:
        st = _stream()
        wires = lk.guarded_device(W * w1)
        wires[:W * w1] = lk.device_words(W * w1, 2424)
        before = wires.clone()
        rng = np.random.default_rng(2425)
        tv = random_words(rng, (3, N))
        in_idx = read[rng.integers(0, read.size, (G, F))]
        in_idx[:6, 0], in_idx[:6, 1] = read[:6], np.roll(read[:6], 1)
        in_idx[6, 1] = -1                                              # an unused slot
        d = {"fan_in": F, "in_idx": in_idx.astype(np.int32), "weights": rng.integers(-(1 << 31), 1 << 31, (G, F)).astype(np.int32),
             "cst": random_words(rng, G), "lut_idx": rng.integers(0, 3, G).astype(np.int32), "wave_offsets": np.array([0, G], np.int32),
             "wave_n_out": np.array([n_out], np.int32), "out_idx": write.astype(np.int32), "num_wires": W}
        with e.lut(tv) as lut:
            c = lck.create(e, lut, d, wires)
            e.circuit_launch(c, st)
            e.sync(st)
            e.circuit_destroy(c)
            lk.report("24 lut_circuit far wire table", e)
            used = np.unique(np.concatenate([in_idx[in_idx >= 0], write]))
            small, at = _small_table(before, w1, used)
            loc = lambda a: np.array([at[int(v)] if v >= 0 else -1 for v in np.asarray(a).reshape(-1)], np.int32).reshape(np.shape(a))  # noqa: E731
            c = lck.create(e, lut, dict(d, in_idx=loc(in_idx), out_idx=loc(write), num_wires=int(used.size)), small)
            e.circuit_launch(c, st)
            e.sync(st)
            e.circuit_destroy(c)
        got = lk.rows_of(wires, w1, write)
        assert np.array_equal(got, lk.rows_of(small, w1, loc(write))), "the far wires give other words than the same wires gathered into a small table"
        x = lk.rows_of(before, w1, used)
        t = np.zeros((G, w1), np.uint32)
        for k in range(F):
            on = in_idx[:, k] >= 0
            t[on] += d["weights"][on, k].astype(np.uint32)[:, None] * x[[at[int(v)] for v in in_idx[on, k]]]
        t[:, -1] += d["cst"]
        exp = gk.pmap(lambda g: oracle_pbs_many(orc, w.P, gk.oracle_plan(orc, N), w.K.bk_f, w.K.ksk, tv[d["lut_idx"][g]], t[g], n_out), range(G))
        assert np.array_equal(got, np.stack(exp).reshape(G * n_out, w1)), "nodes that differ from the oracle"
        assert _rest_unchanged(wires, before, w1, write), "a wire that no node writes changed (or the canary did)"
        lk.check_canary(small, used.size * w1)
    finally:
        e.close()
        wires = before = small = None
        lk.release()
