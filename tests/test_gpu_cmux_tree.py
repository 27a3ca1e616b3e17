"""GPU: CMUX-tree table lookup with caller-supplied TRGSW selectors (rtfhe_trgsw_create, rtfhe_cmux_tree_batch[_dev],
rtfhe_cmux_tree_extract_batch[_dev]; the k_cmux_tree kernels).  Every word against the oracle's tree (tests/leveled_oracle.py:
oracle_cmux_tree) at both N, every depth 1 .. 4 and counts 1, 5 and 37; the extract form; a second opinion built from
rtfhe_external_product_batch alone; what the tree means; its composition with the PBS from encrypted tables; refusals and the capture rule.
Small TLWE dimensions as the other stage tests use: n = 40 at N = 1024, n = 24 at N = 2048."""
import numpy as np
import pytest

import gpu_kit as gk
from kit import random_words
from leveled_kit import TREE_N_ROWS, TREE_N_SEL, selector_world, tree_dev, tree_lookups, tree_oracle
from leveled_oracle import as_trlwe

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=[1024, 2048], ids=lambda N: "N%d" % N)
def world(request, orc):
    """Per N: keys from the product's keygen on an engine, TREE_N_SEL selectors of known random bits (device handle, torus words and the oracle's
    spectra of them), one plain and one really encrypted table of TREE_N_ROWS random rows."""
    N = request.param
    w, rng = selector_world(orc, N, 0x7EE + N, N + 11, TREE_N_SEL, 0x5E1EC7 + N)
    w.rows = {"plain": random_words(rng, (TREE_N_ROWS, N)), "encrypted": w.R.encrypt_lut(w.rp, w.key1, random_words(rng, (TREE_N_ROWS, N)), seed=0x7AB + N)}
    w.eng = gk.engine(w.R, w.rp, w.bk, w.ksk)
    w.sel = w.eng.selectors(w.sel_t)
    w.lut = {"plain": w.eng.lut(w.rows["plain"]), "encrypted": w.eng.lut_encrypted(w.rows["encrypted"])}
    w.oracle_memo = {}
    yield w
    for h in (w.sel, w.lut["plain"], w.lut["encrypted"]):
        h.close()
    w.eng.close()


@pytest.mark.parametrize("count", [1, 5, 37])
@pytest.mark.parametrize("depth", [1, 2, 3, 4])
def test_every_word_equals_the_oracle_tree(orc, world, depth, count):
    """Plain and really encrypted tables; selectors shared between lookups with row0 non-zero and differing per lookup, then sel_idx = NULL and
    row0 = NULL; the host form against the oracle and the _dev form against the host form.  Depths 1 .. 4 cover the single-level case and odd
    and even numbers of buffer swaps; 37 lookups of depth 4 are 296 level-0 nodes, more than one workgroup, and 74 and 37 nodes at the last
    two levels: no multiple of a wave count."""
    w = world
    for kind in ("plain", "encrypted"):
        for sel_idx, row0, exp_idx, exp_row0 in tree_lookups(depth, count):
            want = tree_oracle(orc, w, kind, depth, exp_idx, exp_row0)
            got = w.eng.cmux_tree_batch(w.sel, w.lut[kind], depth, count, sel_idx, row0)
            assert got.shape == (count, 2, w.N)
            assert np.array_equal(got, want), (kind, sel_idx is None, np.flatnonzero((got != want).any(axis=(1, 2)))[:8])
            assert np.array_equal(tree_dev(w, kind, depth, count, sel_idx, row0), got), (kind, sel_idx is None)


def test_extract_form_equals_the_oracle(orc, world):
    """identity_key_switch(sample_extract_index(result, coef)) at coef 0, 1 and N - 1, and coef = NULL; host and _dev forms."""
    w = world
    depth, count = 3, 7
    rng = np.random.default_rng(w.N + 31)
    sel_idx = rng.integers(0, TREE_N_SEL, (count, depth)).astype(np.int32)
    row0 = rng.integers(0, TREE_N_ROWS - 8 + 1, count).astype(np.int32)
    coef = np.array([0, 1, w.N - 1, w.N - 1, 1, 0, w.N // 2 + 3], np.int32)
    for kind in ("plain", "encrypted"):
        for cf, exp in ((coef, coef), (None, np.zeros(count, np.int32))):
            want = tree_oracle(orc, w, kind, depth, sel_idx, row0, exp)
            got = w.eng.cmux_tree_extract_batch(w.sel, w.lut[kind], depth, count, sel_idx, row0, cf)
            assert got.shape == (count, w.rp.n + 1) and np.array_equal(got, want), (kind, cf is None)
            assert np.array_equal(tree_dev(w, kind, depth, count, sel_idx, row0, cf, extract=True), got), (kind, cf is None)


def test_extract_form_of_a_single_level(orc, world):
    """Depth 1 has no ping-pong buffers: level 0 reads the table and, in the extract form, writes the lvl1 samples itself (no node is stored
    anywhere).  Plain and encrypted tables, coef given and NULL, host and _dev forms -- first thing on a fresh engine, whose streams own no
    tree buffers yet."""
    w = world
    depth, count = 1, 5
    sel_idx = np.array([[0], [1], [1], [7], [0]], np.int32)
    row0 = np.array([0, TREE_N_ROWS - 2, 3, 3, 8], np.int32)
    coef = np.array([0, 1, w.N - 1, w.N // 2 + 3, 0], np.int32)
    e = gk.engine(w.R, w.rp, w.bk, w.ksk)
    try:
        with e.selectors(w.sel_t[:8]) as sel:
            for kind in ("plain", "encrypted"):
                with (e.lut(w.rows[kind]) if kind == "plain" else e.lut_encrypted(w.rows[kind])) as lut:
                    for cf, exp in ((coef, coef), (None, np.zeros(count, np.int32))):
                        want = tree_oracle(orc, w, kind, depth, sel_idx, row0, exp)
                        got = e.cmux_tree_extract_batch(sel, lut, depth, count, sel_idx, row0, cf)
                        assert got.shape == (count, w.rp.n + 1) and np.array_equal(got, want), (kind, cf is None)
                        assert np.array_equal(tree_dev(w, kind, depth, count, sel_idx, row0, cf, extract=True, on=(e, sel, lut)), got), (kind, cf is None)
    finally:
        e.close()


def test_extract_form_with_the_wave_per_sample_key_switch(orc, world, monkeypatch):
    """RTFHE_KS_MM_MIN=0: a context without the matrix form of the key-switching key runs k_key_switch_ext after the tree; the same words."""
    w = world
    e = gk.engine(w.R, w.rp, w.bk, w.ksk, monkeypatch, {"RTFHE_KS_MM_MIN": "0"})
    try:
        depth, count = 2, 5
        sel_idx = np.array([[0, 1], [1, 0], [2, 3], [5, 5], [1, 1]], np.int32)
        row0 = np.array([0, 3, 7, 19, 1], np.int32)
        coef = np.array([0, 1, w.N - 1, 17, 0], np.int32)
        with e.selectors(w.sel_t[:6]) as sel, e.lut_encrypted(w.rows["encrypted"]) as lut:
            got = e.cmux_tree_extract_batch(sel, lut, depth, count, sel_idx, row0, coef)
        assert np.array_equal(got, tree_oracle(orc, w, "encrypted", depth, sel_idx, row0, coef))
    finally:
        e.close()


def test_second_opinion_from_external_products_alone(world):
    """No oracle: a context with Params(n = depth) takes the selector set as its bootstrapping key, and the tree is run level by level as
    external_product_batch(idx, r1 - r0) + r0 in numpy.  Every word equals the tree call's -- on that context, and on one with no key at all
    (a selector set does not depend on the context's keys), where the extract form is refused for want of the key-switching key."""
    w, R = world, world.R
    depth, count = 3, 5
    rng = np.random.default_rng(w.N + 41)
    p = R.Params(n=depth, N=w.N)
    sel_idx = rng.integers(0, depth, (count, depth)).astype(np.int32)
    row0 = rng.integers(0, TREE_N_ROWS - 8 + 1, count).astype(np.int32)
    e = R.Engine(p, 0)
    bare = R.Engine(p, 0)
    try:
        e.load_bk_torus(w.sel_t[:depth].reshape(-1))
        for kind in ("plain", "encrypted"):
            table = as_trlwe(w.rows[kind], w.N)
            nodes = np.stack([table[r:r + 8] for r in row0])                                # [count][8][2][N]
            for k in range(depth):
                r0, r1 = nodes[:, 0::2], nodes[:, 1::2]
                idx = np.repeat(sel_idx[:, k], r0.shape[1])
                nodes = e.external_product_batch(idx, (r1 - r0).reshape(-1, 2, w.N)).reshape(r0.shape) + r0
            for eng in (e, bare):
                with eng.selectors(w.sel_t[:depth]) as sel, (eng.lut(w.rows[kind]) if kind == "plain" else eng.lut_encrypted(w.rows[kind])) as lut:
                    assert np.array_equal(eng.cmux_tree_batch(sel, lut, depth, count, sel_idx, row0), nodes[:, 0]), kind
                    if eng is bare:
                        with pytest.raises(R.RtfheError) as ei:
                            eng.cmux_tree_extract_batch(sel, lut, depth, count, sel_idx, row0)
                        assert ei.value.code == R._ffi.ERR_STATE and "key-switching key" in str(ei.value)
    finally:
        e.close()
        bare.close()


def _addressed(w, depth, addrs):
    """sel_idx [len(addrs)][depth] over the world's selectors: entry k encrypts bit k of the address"""
    by_bit = [np.flatnonzero(w.bits == 0), np.flatnonzero(w.bits == 1)]
    return np.array([[by_bit[(a >> k) & 1][(3 * a + k) % len(by_bit[(a >> k) & 1])] for k in range(depth)] for a in addrs], np.int32)


def test_every_address_decodes_to_its_row(world):
    """Every address 0 .. 15 of a depth-4 tree over encrypted rows of N random 2-bit messages: the selected TRLWE decrypts to the addressed row
    at every coefficient, and the extract form to that row's coefficient coef."""
    w, R = world, world.R
    rng = np.random.default_rng(w.N + 51)
    msgs = rng.integers(0, 4, (16, w.N))
    addrs = np.arange(16)
    sel_idx = _addressed(w, 4, addrs)
    coef = rng.integers(0, w.N, 16).astype(np.int32)
    with w.eng.lut_encrypted(R.encrypt_lut(w.rp, w.key1, R.encode_msgs(msgs, 2), seed=0xADD + w.N)) as lut:
        out = w.eng.cmux_tree_batch(w.sel, lut, 4, 16, sel_idx)
        ext = w.eng.cmux_tree_extract_batch(w.sel, lut, 4, 16, sel_idx, None, coef)
    assert np.array_equal(R.decode_msgs(R.trlwe_phase(w.rp, w.key1, out), 2), msgs[addrs])
    assert np.array_equal(R.decode_msgs(R.phases(w.rp, w.key0, ext), 2), msgs[addrs, coef])


def test_selected_row_composes_with_the_pbs(world):
    """Vertical packing: the high address bits select one of 16 rows by CMUX tree, the low 2-bit digit goes through a PBS whose encrypted table
    (Engine.lut_encrypted) is the selected row.  For a trivially encrypted table (tv, 0) the selected row is no longer trivial -- every CMUX
    adds its product's a-part -- so the outputs are compared as messages: they equal the same PBS on the row selected in the clear, and f_addr(m)."""
    w, R = world, world.R
    rng = np.random.default_rng(w.N + 61)
    funcs = rng.integers(0, 4, (16, 4))
    tv = np.stack([R.lut_polynomial([int(v) for v in f], w.N, 2) for f in funcs])
    addrs = np.array([0, 5, 10, 15, 3, 12], np.int64)
    m = np.array([0, 1, 2, 3, 2, 1])
    ct = R.encrypt_torus(w.rp, w.key0, R.encode_msgs(m, 2), seed=0xC0 + w.N)
    with w.eng.lut_encrypted(as_trlwe(tv, w.N)) as table:
        picked = w.eng.cmux_tree_batch(w.sel, table, 4, len(addrs), _addressed(w, 4, addrs))
    with w.eng.lut_encrypted(picked) as lut, w.eng.lut(tv) as clear:
        got = w.eng.pbs_batch(lut, ct, np.arange(len(addrs)))
        ref = w.eng.pbs_batch(clear, ct, addrs)
    dec = lambda c: R.decode_msgs(R.phases(w.rp, w.key0, c), 2)  # noqa: E731
    assert np.array_equal(dec(got), dec(ref)) and np.array_equal(dec(got), funcs[addrs, m])


def test_bad_arguments_host_and_device(world):
    """Host-side arrays are checked before anything is launched, the message names the lookup; device-side arrays are checked by the kernel: the
    lookup is skipped and the next sync reports it."""
    import torch
    w, R = world, world.R
    depth, count = 2, 6
    lut = w.lut["encrypted"]
    sel_idx = np.tile(np.array([[0, 1]], np.int32), (count, 1))
    row0 = np.arange(count, dtype=np.int32)
    ref = w.eng.cmux_tree_batch(w.sel, lut, depth, count, sel_idx, row0)
    ref_x = w.eng.cmux_tree_extract_batch(w.sel, lut, depth, count, sel_idx, row0)
    bad_sel, bad_row, bad_coef = sel_idx.copy(), row0.copy(), np.zeros(count, np.int32)
    bad_sel[3, 1] = TREE_N_SEL
    bad_row[3] = TREE_N_ROWS - 3
    bad_coef[3] = w.N
    w.eng.timer_begin()
    for call, names in ((lambda: w.eng.cmux_tree_batch(w.sel, lut, depth, count, bad_sel, row0), "lookup 3: sel_idx[1]"),
                        (lambda: w.eng.cmux_tree_batch(w.sel, lut, depth, count, sel_idx, bad_row), "lookup 3: row0"),
                        (lambda: w.eng.cmux_tree_extract_batch(w.sel, lut, depth, count, sel_idx, row0, bad_coef), "lookup 3: coef"),
                        (lambda: w.eng.cmux_tree_batch(w.sel, lut, 0, count), "depth"),
                        (lambda: w.eng.cmux_tree_batch(w.sel, lut, 17, count), "depth"),
                        (lambda: w.eng.cmux_tree_batch(w.sel, lut, 5, 1), "32 rows"),              # of a 23-row table
                        (lambda: w.eng.cmux_tree_batch(w.sel, lut, 4, 38), "lookup 37")):          # sel_idx NULL: 152 selectors of 148
        with pytest.raises(R.RtfheError) as ei:
            call()
        assert ei.value.code == R._ffi.ERR_INVALID and names in str(ei.value), str(ei.value)
    assert w.eng.timer_end()[1] == 0, "the checks come before any launch"
    keep = np.ones(count, bool)
    keep[3] = False
    st = torch.cuda.current_stream().cuda_stream
    for kw in ({"d_sel_idx": gk.to_device(bad_sel), "d_row0": gk.to_device(row0)}, {"d_sel_idx": gk.to_device(sel_idx), "d_row0": gk.to_device(bad_row)}):
        d_out = torch.zeros((count, 2, w.N), dtype=torch.int32, device="cuda")
        w.eng.cmux_tree_batch_dev(w.sel, lut, depth, d_out, count, stream=st, **kw)
        with pytest.raises(R.RtfheError) as ei:
            w.eng.sync(st)
        assert ei.value.code == R._ffi.ERR_INVALID
        got = d_out.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[keep], ref[keep]) and not got[3].any()
    d_out = torch.zeros((count, w.rp.n + 1), dtype=torch.int32, device="cuda")
    w.eng.cmux_tree_extract_batch_dev(w.sel, lut, depth, d_out, count, gk.to_device(sel_idx), gk.to_device(row0), gk.to_device(bad_coef), st)
    with pytest.raises(R.RtfheError):
        w.eng.sync(st)
    assert np.array_equal(d_out.cpu().numpy().view(np.uint32)[keep], ref_x[keep])
    w.eng.sync(st)                                           # reported once
    assert np.array_equal(tree_dev(w, "encrypted", depth, count, sel_idx, row0), ref)


def test_exact_backends_refuse_and_mirror_recovers(world):
    w, R = world, world.R
    lut = w.lut["plain"]
    ref = w.eng.cmux_tree_batch(w.sel, lut, 2, 5)
    try:
        for b in (R._ffi.BACKEND_NTT_EXACT, R._ffi.BACKEND_FFT_SPLIT_EXACT):
            w.eng.set_backend(b)
            for call in (lambda: w.eng.cmux_tree_batch(w.sel, lut, 2, 5), lambda: w.eng.cmux_tree_extract_batch(w.sel, lut, 2, 5)):
                with pytest.raises(R.RtfheError) as ei:
                    call()
                assert ei.value.code == R._ffi.ERR_INVALID and "mirror" in str(ei.value)
    finally:
        w.eng.set_backend(R._ffi.BACKEND_FFT64_MIRROR)
    assert np.array_equal(w.eng.cmux_tree_batch(w.sel, lut, 2, 5), ref)


def test_graph_capture_replays_eager_words(world):
    """Inside torch.cuda.graph nothing may be allocated: after one eager call of that size on the stream both _dev forms are captured and
    replay to the eager words."""
    import torch
    w = world
    depth, count = 3, 37
    rng = np.random.default_rng(w.N + 71)
    sel_idx = gk.to_device(rng.integers(0, TREE_N_SEL, (count, depth)))
    row0 = gk.to_device(rng.integers(0, TREE_N_ROWS - 8 + 1, count))
    coef = gk.to_device(rng.integers(0, w.N, count))
    lut = w.lut["encrypted"]
    s = torch.cuda.Stream()
    out = torch.zeros((count, 2, w.N), dtype=torch.int32, device="cuda")
    out_x = torch.zeros((count, w.rp.n + 1), dtype=torch.int32, device="cuda")

    def both():
        w.eng.cmux_tree_batch_dev(w.sel, lut, depth, out, count, sel_idx, row0, s.cuda_stream)
        w.eng.cmux_tree_extract_batch_dev(w.sel, lut, depth, out_x, count, sel_idx, row0, coef, s.cuda_stream)

    with torch.cuda.stream(s):
        both()                                               # the eager calls the capture rule asks for
        w.eng.sync(s.cuda_stream)
        eager, eager_x = out.clone(), out_x.clone()
        assert eager.any() and eager_x.any()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            both()
        for _ in range(2):
            out.zero_()
            out_x.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, eager) and torch.equal(out_x, eager_x)
        w.eng.sync(s.cuda_stream)


def test_larger_eager_call_retires_the_buffers_a_graph_holds(orc, world):
    """A fresh stream: an eager depth-2 tree of 5 lookups, the same call captured, then an eager depth-3 tree of 37 lookups on that stream, which
    replaces the stream's ping-pong buffers.  The graph holds the old pair's addresses: it is kept, not freed, so the replays still give the
    small call's eager words (the oracle's), and the large call gives the oracle's."""
    import torch
    w = world
    lut = w.lut["encrypted"]
    idx2, row2, _, _ = tree_lookups(2, 5)[0]
    idx3, row3, _, _ = tree_lookups(3, 37)[0]
    d_idx2, d_row2, d_idx3, d_row3 = gk.to_device(idx2), gk.to_device(row2), gk.to_device(idx3), gk.to_device(row3)
    s = torch.cuda.Stream()
    out = torch.zeros((5, 2, w.N), dtype=torch.int32, device="cuda")
    big = torch.zeros((37, 2, w.N), dtype=torch.int32, device="cuda")
    with torch.cuda.stream(s):
        w.eng.cmux_tree_batch_dev(w.sel, lut, 2, out, 5, d_idx2, d_row2, s.cuda_stream)
        w.eng.sync(s.cuda_stream)
        eager = out.clone()
        assert np.array_equal(eager.cpu().numpy().view(np.uint32), tree_oracle(orc, w, "encrypted", 2, idx2, row2))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            w.eng.cmux_tree_batch_dev(w.sel, lut, 2, out, 5, d_idx2, d_row2, s.cuda_stream)
        w.eng.cmux_tree_batch_dev(w.sel, lut, 3, big, 37, d_idx3, d_row3, s.cuda_stream)
        w.eng.sync(s.cuda_stream)
        assert np.array_equal(big.cpu().numpy().view(np.uint32), tree_oracle(orc, w, "encrypted", 3, idx3, row3))
        for _ in range(2):
            out.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, eager)
        w.eng.sync(s.cuda_stream)


def test_wide_lut_example(engine, keys):
    """examples/wide_lut.py at the full parameter set: 24 six-bit lookups, four address bits by CMUX tree and two by PBS."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("wide_lut", os.path.join(root, "examples", "wide_lut.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    addr, got, want = ex.run(engine, keys.key0, keys.key1, 24, seed=0x6B17)
    assert len(addr) == 24 and np.array_equal(got, want)
