"""GPU: the CMUX demultiplexer tree and the table accumulation (rtfhe_demux_tree_batch[_dev], rtfhe_lut_accumulate_dev, rtfhe_lut_read_dev;
k_demux_tree, k_trlwe_accumulate).  Every word against the oracle's demultiplexer (tests/leveled_oracle.py: oracle_demux_tree) at both N,
depths 1 .. 3 and counts 1, 5 and 37, in both leveled decomposition modes; a second opinion built from rtfhe_external_product_batch alone; the
inverse of the CMUX tree on the device; the accumulation word for word; skipped lookups; refusals; the capture rule; the histogram example.
Small TLWE dimensions as the tree's tests use: n = 40 at N = 1024, n = 24 at N = 2048."""
import contextlib

import numpy as np
import pytest

import gpu_kit as gk
import round_oracle as ro
from kit import random_words
from leveled_kit import selector_world
from leveled_oracle import oracle_demux_tree

pytestmark = pytest.mark.gpu

MAX_DEPTH, MAX_COUNT = 3, 37
N_SEL = MAX_COUNT * MAX_DEPTH          # sel_idx = NULL at depth 3 and 37 lookups reads selectors 0 .. 110


@contextlib.contextmanager
def _leveled(eng, rounded=True):
    """the engine's leveled decomposition mode set for the block and restored after it"""
    import rustfhe_amd as R
    before = eng.leveled_decomposition()
    eng.set_leveled_decomposition(R._ffi.DECOMP_ROUNDED if rounded else R._ffi.DECOMP_REFERENCE)
    try:
        yield eng
    finally:
        eng.set_leveled_decomposition(before)


@pytest.fixture(scope="module", params=[1024, 2048], ids=lambda N: "N%d" % N)
def world(request, orc):
    """Per N: keys from the product's keygen on an engine, N_SEL selectors of known random bits (device handle, torus words and the oracle's
    spectra of them), MAX_COUNT inputs x of random words."""
    N = request.param
    w, rng = selector_world(orc, N, 0xDE7 + N, N + 13, N_SEL, 0x5E1ED3 + N)
    w.x = random_words(rng, (MAX_COUNT, 2, N))
    w.eng = gk.engine(w.R, w.rp, w.bk, w.ksk)
    w.sel = w.eng.selectors(w.sel_t)
    w.memo = {}
    yield w
    w.sel.close()
    w.eng.close()


def _oracle(orc, w, depth, sel_idx, x, mode=ro.REFERENCE):
    """the oracle's demultiplexer of every lookup: sel_idx [count][depth], x [count][2][N]; computed once per world and arguments, shared by the
    tests that ask for the same lookups, and read-only"""
    return gk.memo(w.memo, (depth, mode, sel_idx, x),
                   lambda: np.stack([oracle_demux_tree(orc, w.P, w.plan, w.sel_f, sel_idx[g], x[g], mode) for g in range(len(x))]))


def _demux_dev(w, x, depth, sel_idx, on=None, stream=None):
    """the _dev form on the world's engine and selectors, or on=(engine, selectors)"""
    import torch
    eng, sel = on or (w.eng, w.sel)
    st = stream or torch.cuda.current_stream().cuda_stream
    count = len(x)
    d_out = torch.zeros((count, 1 << depth, 2, w.N), dtype=torch.int32, device="cuda")
    eng.demux_tree_batch_dev(sel, gk.to_device(x, np.uint32), depth, d_out, count, gk.to_device(sel_idx), st)
    eng.sync(st)
    return gk.words_of(d_out)


def _lookups(depth, count):
    """(sel_idx, what it means to the oracle) twice: six selectors shared between the lookups; then sel_idx = NULL"""
    rng = np.random.default_rng(100 * depth + count)
    shared = rng.integers(0, 6, (count, depth)).astype(np.int32)
    return (shared, shared), (None, np.arange(count * depth, dtype=np.int32).reshape(count, depth))


@pytest.mark.parametrize("mode", [ro.REFERENCE, ro.ROUNDED], ids=["reference", "rounded"])
@pytest.mark.parametrize("count", [1, 5, 37])
@pytest.mark.parametrize("depth", [1, 2, 3])
def test_every_word_equals_the_oracle_demux(orc, world, depth, count, mode):
    """Selectors shared between lookups, then sel_idx = NULL; the host form against the oracle and the _dev form against the host form, in
    both leveled decomposition modes.  Depth 1 has no ping-pong buffer, depths 2 and 3 one and two buffer hand-overs.  Depth 3 at 37 lookups is
    148 last-level input nodes: 37 workgroups and no idle wave; depth 1 at 5 lookups leaves three idle waves in the second workgroup."""
    w = world
    x = w.x[:count]
    with _leveled(w.eng, mode == ro.ROUNDED):
        for sel_idx, exp_idx in _lookups(depth, count):
            want = _oracle(orc, w, depth, exp_idx, x, mode)
            got = w.eng.demux_tree_batch(w.sel, x, depth, sel_idx)
            assert got.shape == (count, 1 << depth, 2, w.N)
            assert np.array_equal(got, want), (sel_idx is None, np.argwhere((got != want).any(axis=(2, 3)))[:8])
            assert np.array_equal(_demux_dev(w, x, depth, sel_idx), got), sel_idx is None


def test_switching_back_to_reference_mode_reproduces_the_first_words(orc, world):
    w, R = world, world.R
    depth, count = 3, 5
    x = w.x[:count]
    sel_idx = _lookups(depth, count)[0][0]
    first = w.eng.demux_tree_batch(w.sel, x, depth, sel_idx)
    assert np.array_equal(first, _oracle(orc, w, depth, sel_idx, x))
    with _leveled(w.eng):
        assert w.eng.leveled_decomposition() == R._ffi.DECOMP_ROUNDED
        rounded = w.eng.demux_tree_batch(w.sel, x, depth, sel_idx)
    assert w.eng.leveled_decomposition() == R._ffi.DECOMP_REFERENCE
    assert not np.array_equal(rounded, first) and np.array_equal(rounded, _oracle(orc, w, depth, sel_idx, x, ro.ROUNDED))
    assert np.array_equal(w.eng.demux_tree_batch(w.sel, x, depth, sel_idx), first)
    assert np.array_equal(_demux_dev(w, x, depth, sel_idx), first)


def test_second_opinion_from_external_products_alone(world):
    """No oracle: a context with Params(n = depth) takes the selector set as its bootstrapping key, and the demultiplexer is run level by level
    as hi = external_product_batch(idx, node), lo = node - hi in numpy.  Every word equals the call's -- on that context, and on one with no key
    at all (only the selector set is needed)."""
    w, R = world, world.R
    depth, count = 3, 5
    rng = np.random.default_rng(w.N + 41)
    p = R.Params(n=depth, N=w.N)
    sel_idx = rng.integers(0, depth, (count, depth)).astype(np.int32)
    x = w.x[:count]
    e = R.Engine(p, 0)
    bare = R.Engine(p, 0)
    try:
        e.load_bk_torus(w.sel_t[:depth].reshape(-1))
        nodes = x[:, None]                                                                    # [count][1][2][N]
        for t in range(depth):
            idx = np.repeat(sel_idx[:, R.demux_level_selector(depth, t)], nodes.shape[1])
            hi = e.external_product_batch(idx, nodes.reshape(-1, 2, w.N)).reshape(nodes.shape)
            nodes = np.stack([nodes - hi, hi], axis=2).reshape(count, -1, 2, w.N)             # children 2j, 2j + 1
        for eng in (e, bare):
            with eng.selectors(w.sel_t[:depth]) as sel:
                assert np.array_equal(eng.demux_tree_batch(sel, x, depth, sel_idx), nodes)
    finally:
        e.close()
        bare.close()


def _addressed(w, depth, addrs):
    """sel_idx [len(addrs)][depth] over the world's selectors: entry k encrypts bit k of the address"""
    by_bit = [np.flatnonzero(w.bits == 0), np.flatnonzero(w.bits == 1)]
    return np.array([[by_bit[(a >> k) & 1][(3 * a + k) % len(by_bit[(a >> k) & 1])] for k in range(depth)] for a in addrs], np.int32)


def test_inverse_of_the_tree_on_the_device(world):
    """Compared as messages.  Every address of a depth-3 demultiplexer of a row of N random 2-bit messages, trivial and encrypted: the
    addressed leaf decodes to the row and every other leaf to 0; the leaves as an encrypted table (Engine.lut_encrypted) under
    cmux_tree_batch with the same selectors decode to the row, and with one address bit flipped to 0."""
    w, R = world, world.R
    depth = 3
    addrs = np.arange(1 << depth)
    rng = np.random.default_rng(w.N + 51)
    msgs = rng.integers(0, 4, w.N)
    plain = R.encode_msgs(msgs, 2)
    sel_idx = _addressed(w, depth, addrs)
    flipped = _addressed(w, depth, addrs ^ (1 << (addrs % depth)))                           # bit (addr mod 3) flipped
    row0 = (addrs << depth).astype(np.int32)
    for kind, x in (("trivial", np.stack([plain, np.zeros_like(plain)])), ("encrypted", R.encrypt_lut(w.rp, w.key1, plain, seed=0xADE + w.N)[0])):
        leaves = w.eng.demux_tree_batch(w.sel, np.repeat(x[None], len(addrs), axis=0), depth, sel_idx)
        want = np.zeros((len(addrs), 1 << depth, w.N), np.int64)
        want[addrs, addrs] = msgs
        got = R.decode_msgs(R.trlwe_phase(w.rp, w.key1, leaves.reshape(-1, 2, w.N)), 2).reshape(want.shape)
        assert np.array_equal(got, want), kind
        with w.eng.lut_encrypted(leaves.reshape(-1, 2, w.N)) as lut:
            back = w.eng.cmux_tree_batch(w.sel, lut, depth, len(addrs), sel_idx, row0)
            wrong = w.eng.cmux_tree_batch(w.sel, lut, depth, len(addrs), flipped, row0)
        assert np.array_equal(R.decode_msgs(R.trlwe_phase(w.rp, w.key1, back), 2), np.tile(msgs, (len(addrs), 1))), kind
        assert not R.decode_msgs(R.trlwe_phase(w.rp, w.key1, wrong), 2).any(), kind


def test_accumulate_adds_the_leaves_into_the_tables_rows(world):
    """5 lookups x 8 leaves added into rows 3 .. 10 of a 16-row encrypted table: every word of the table, read back with Lut.read_dev, equals
    the numpy wrapping sum; rows 0 .. 2 and 11 .. 15 keep their bytes.  A second accumulation adds again.  A plain table, bad ranges, count 0
    and host pointers are refused, and the refusals launch nothing."""
    import torch
    w, R = world, world.R
    depth, count = 3, 5
    st = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(w.N + 61)
    rows = random_words(rng, (16, 2, w.N))
    leaves = w.eng.demux_tree_batch(w.sel, w.x[:count], depth, _lookups(depth, count)[0][0])
    d_leaves = gk.to_device(leaves, np.uint32)
    want = rows.copy()
    want[3:11] += leaves.sum(axis=0, dtype=np.uint32)
    d_back = torch.zeros((16, 2, w.N), dtype=torch.int32, device="cuda")
    with w.eng.lut_encrypted(rows) as table, w.eng.lut(rows[:, 0]) as plain:
        table.accumulate_dev(d_leaves, 3, 8, count, st)
        table.read_dev(d_back, 0, 16, st)
        w.eng.sync(st)
        assert np.array_equal(gk.words_of(d_back), want), np.flatnonzero((gk.words_of(d_back) != want).any(axis=(1, 2)))
        table.accumulate_dev(d_leaves[:2], 8, 8, 2, st)                      # the last row of the table is the range's last
        want[8:16] += leaves[:2].sum(axis=0, dtype=np.uint32)
        part = torch.zeros((9, 2, w.N), dtype=torch.int32, device="cuda")
        table.read_dev(part[:8], 8, 8, st)
        w.eng.sync(st)
        assert np.array_equal(gk.words_of(part)[:8], want[8:]) and not gk.words_of(part)[8].any()
        w.eng.timer_begin()
        for call, word in ((lambda: plain.accumulate_dev(d_leaves, 3, 8, count), "plain"), (lambda: plain.read_dev(d_back, 0, 1), "plain"),
                           (lambda: table.accumulate_dev(d_leaves, -1, 8, count), "outside"), (lambda: table.accumulate_dev(d_leaves, 9, 8, count), "outside"),
                           (lambda: table.accumulate_dev(d_leaves, 0, -1, count), "outside"), (lambda: table.read_dev(d_back, 1, 16), "outside"),
                           (lambda: table.accumulate_dev(d_leaves, 3, 8, 0), "count"),
                           (lambda: table.accumulate_dev(leaves.ctypes.data, 3, 8, count), "device pointer"),
                           (lambda: table.read_dev(rows.ctypes.data, 0, 1), "device pointer")):
            with pytest.raises(R.RtfheError) as ei:
                call()
            assert ei.value.code == R._ffi.ERR_INVALID and word in str(ei.value), str(ei.value)
        assert w.eng.timer_end()[1] == 0, "the checks come before any launch"
        table.accumulate_dev(d_leaves, 16, 0, count)                        # an empty range is no error
        table.read_dev(d_back, 0, 16, st)
        w.eng.sync(st)
        assert np.array_equal(gk.words_of(d_back), want)


@pytest.mark.parametrize("depth", [1, 3])
def test_a_lookup_with_a_bad_device_index_is_skipped_whole(orc, world, depth):
    """One bad device-resident index among 5 lookups (-1 at depth 1, N_SEL in the last entry at depth 3): that lookup's 2^d output rows and the
    guard rows around `out` keep every byte of a sentinel, the other lookups' rows equal the oracle's, sync fails once and then succeeds."""
    import torch
    w, R = world, world.R
    count, leaves, GUARD = 5, 1 << depth, 4
    st = torch.cuda.current_stream().cuda_stream
    x = w.x[:count]
    good = _lookups(depth, count)[0][0]
    bad = good.copy()
    bad[3, depth - 1] = -1 if depth == 1 else N_SEL
    clean = _oracle(orc, w, depth, good, x)
    n_rows = count * leaves + 2 * GUARD
    sentinel = (0xA5000000 + 0x1001 * np.arange(n_rows, dtype=np.uint32)[:, None] + np.arange(2 * w.N, dtype=np.uint32)[None, :]).astype(np.uint32)
    buf = gk.to_device(sentinel, np.uint32)
    w.eng.demux_tree_batch_dev(w.sel, gk.to_device(x, np.uint32), depth, buf[GUARD:GUARD + count * leaves], count, gk.to_device(bad), st)
    with pytest.raises(R.RtfheError) as ei:
        w.eng.sync(st)
    assert ei.value.code == R._ffi.ERR_INVALID
    w.eng.sync(st)                                           # reported once
    want = sentinel.copy()
    for g in (0, 1, 2, 4):
        want[GUARD + g * leaves:GUARD + (g + 1) * leaves] = clean[g].reshape(leaves, 2 * w.N)
    got = gk.words_of(buf)
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))
    assert np.array_equal(_demux_dev(w, x, depth, good), clean)


def test_bad_arguments_are_refused_before_anything_is_launched(world):
    import torch
    w, R = world, world.R
    depth, count = 2, 6
    x = w.x[:count]
    sel_idx = np.tile(np.array([[0, 1]], np.int32), (count, 1))
    bad_sel = sel_idx.copy()
    bad_sel[3, 1] = N_SEL
    d_x = gk.to_device(x, np.uint32)
    d_big = torch.zeros((count * 4 + 1, 2, w.N), dtype=torch.int32, device="cuda")
    host_out = np.zeros((count, 4, 2, w.N), np.uint32)
    w.eng.timer_begin()
    for call, names in ((lambda: w.eng.demux_tree_batch(w.sel, x, depth, bad_sel), "lookup 3: sel_idx[1]"),
                        (lambda: w.eng.demux_tree_batch(w.sel, x, 0), "depth"),
                        (lambda: w.eng.demux_tree_batch(w.sel, x, 17), "depth"),
                        (lambda: w.eng.demux_tree_batch_dev(w.sel, d_x, 0, d_big, count), "depth"),
                        (lambda: w.eng.demux_tree_batch_dev(w.sel, d_x, 17, d_big, count), "depth"),
                        (lambda: w.eng.demux_tree_batch(w.sel, np.tile(x, (7, 1, 1))[:38], 3), "lookup 37"),        # sel_idx NULL: 114 selectors of 111
                        (lambda: w.eng.demux_tree_batch_dev(w.sel, d_big, depth, d_big, count), "overlaps"),
                        (lambda: w.eng.demux_tree_batch_dev(w.sel, d_big[3:4], depth, d_big, 1), "overlaps"),          # x inside the four leaves
                        (lambda: w.eng.demux_tree_batch_dev(w.sel, d_x, depth, None, count), "null argument"),
                        (lambda: w.eng.demux_tree_batch_dev(w.sel, None, depth, d_big, count), "null argument"),
                        (lambda: w.eng._ck(w.eng.L.rtfhe_demux_tree_batch_dev(w.eng.h, None, None, depth, d_x.data_ptr(), d_big.data_ptr(), count, None)), "null selector"),
                        (lambda: w.eng._ck(w.eng.L.rtfhe_demux_tree_batch_dev(w.eng.h, w.sel.h, None, depth, x.ctypes.data, host_out.ctypes.data, count, None)),
                         "device pointers")):
        with pytest.raises(R.RtfheError) as ei:
            call()
        assert ei.value.code == R._ffi.ERR_INVALID and names in str(ei.value), str(ei.value)
    assert w.eng.timer_end()[1] == 0, "the checks come before any launch"
    # d_out right behind d_x does not overlap it
    w.eng.demux_tree_batch_dev(w.sel, d_big[:1], depth, d_big[1:5], 1, gk.to_device(sel_idx[:1]))
    w.eng.sync()
    assert np.array_equal(gk.words_of(d_big[1:5])[None], w.eng.demux_tree_batch(w.sel, np.zeros((1, 2, w.N), np.uint32), depth, sel_idx[:1]))


def test_exact_backends_refuse_and_mirror_recovers(world):
    w, R = world, world.R
    x = w.x[:5]
    ref = w.eng.demux_tree_batch(w.sel, x, 2)
    try:
        for b in (R._ffi.BACKEND_NTT_EXACT, R._ffi.BACKEND_FFT_SPLIT_EXACT):
            w.eng.set_backend(b)
            with pytest.raises(R.RtfheError) as ei:
                w.eng.demux_tree_batch(w.sel, x, 2)
            assert ei.value.code == R._ffi.ERR_INVALID and "mirror" in str(ei.value)
    finally:
        w.eng.set_backend(R._ffi.BACKEND_FFT64_MIRROR)
    assert np.array_equal(w.eng.demux_tree_batch(w.sel, x, 2), ref)


def test_capture_rule_and_replay(orc, world):
    """A fresh engine and a fresh stream: a capture with no prior eager call is refused at depth 2 (RTFHE_ERR_STATE, the capture goes on) and
    taken at depth 1, which needs no buffer; after one eager call of that size the depth-3 call is captured and replays to the eager words."""
    import torch
    w, R = world, world.R
    count = 37
    x = w.x[:count]
    idx = {d: _lookups(d, count)[0][0] for d in (1, 2, 3)}
    want1, want3 = _oracle(orc, w, 1, idx[1], x), _oracle(orc, w, 3, idx[3], x)
    e = R.Engine(w.rp, 0)                                     # no key of the context is needed
    try:
        with e.selectors(w.sel_t) as sel:
            s = torch.cuda.Stream()
            d_x = gk.to_device(x, np.uint32)
            d_idx = {d: gk.to_device(i) for d, i in idx.items()}
            out1 = torch.zeros((count, 2, 2, w.N), dtype=torch.int32, device="cuda")
            out2 = torch.zeros((count, 4, 2, w.N), dtype=torch.int32, device="cuda")
            out3 = torch.zeros((count, 8, 2, w.N), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            refused = []
            with torch.cuda.stream(s):
                g0 = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g0, stream=s):
                    e.demux_tree_batch_dev(sel, d_x, 1, out1, count, d_idx[1], s.cuda_stream)
                    try:
                        e.demux_tree_batch_dev(sel, d_x, 2, out2, count, d_idx[2], s.cuda_stream)
                    except R.RtfheError as err:
                        refused.append(err)
                assert len(refused) == 1 and refused[0].code == R._ffi.ERR_STATE and "capture" in str(refused[0])
                g0.replay()
                torch.cuda.synchronize()
                assert np.array_equal(gk.words_of(out1), want1) and not gk.words_of(out2).any()
                e.demux_tree_batch_dev(sel, d_x, 3, out3, count, d_idx[3], s.cuda_stream)      # the eager call the capture rule asks for
                e.sync(s.cuda_stream)
                assert np.array_equal(gk.words_of(out3), want3)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=s):
                    e.demux_tree_batch_dev(sel, d_x, 3, out3, count, d_idx[3], s.cuda_stream)
                for _ in range(2):
                    out3.zero_()
                    g.replay()
                    torch.cuda.synchronize()
                    assert np.array_equal(gk.words_of(out3), want3)
                e.sync(s.cuda_stream)
    finally:
        e.close()


def test_private_histogram_example(params, keys):
    """examples/private_histogram.py at the full parameter set on an engine without keys, at 64 clients: the decoded counts are the clear
    histogram, and the engine's mode is restored."""
    import importlib.util
    import os
    import rustfhe_amd as R
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("private_histogram", os.path.join(root, "examples", "private_histogram.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    e = R.Engine(R.Params(n=params.n, N=params.N), 0)
    try:
        want, got, bits = ex.run(e, keys.key1, 64, seed=0x6B19)
        assert want.sum() == 64 and bits == 6 and np.array_equal(got, want)
        assert e.leveled_decomposition() == R._ffi.DECOMP_REFERENCE
    finally:
        e.close()
