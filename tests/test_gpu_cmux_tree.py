"""GPU: CMUX-tree table lookup with caller-supplied TRGSW selectors (rtfhe_trgsw_create, rtfhe_cmux_tree_batch[_dev],
rtfhe_cmux_tree_extract_batch[_dev]; the k_cmux_tree kernels).  Every word against the oracle's tree (tests/test_cmux_tree_host.py:
oracle_cmux_tree) at both N, every depth 1 .. 4 and counts 1, 5 and 37; the extract form; a second opinion built from
rtfhe_external_product_batch alone; what the tree means; its composition with the PBS from encrypted tables; refusals and the capture rule.
Small TLWE dimensions as the other stage tests use: n = 40 at N = 1024, n = 24 at N = 2048."""
import types

import numpy as np
import pytest

from test_cmux_tree_host import as_trlwe, oracle_cmux_tree
from test_gpu_pbs import _engine, _random_words
from test_pbs_host import bk_fft

pytestmark = pytest.mark.gpu

SMALL_N = {1024: 40, 2048: 24}
N_SEL = 37 * 4          # sel_idx = NULL at depth 4 and 37 lookups reads selectors 0 .. 147
N_ROWS = 16 + 7         # row0 up to 7 at depth 4


@pytest.fixture(scope="module", params=[1024, 2048], ids=lambda N: "N%d" % N)
def world(request, orc):
    """Per N: keys from the product's keygen on an engine, N_SEL selectors of known random bits (device handle, torus words and the oracle's
    spectra of them), one plain and one really encrypted table of N_ROWS random rows."""
    import rustfhe_amd as R
    N = request.param
    rp = R.Params(n=SMALL_N[N], N=N)
    key0, key1, bk, ksk = R.keygen(rp, 0x7EE + N)
    w = types.SimpleNamespace(R=R, N=N, rp=rp, key0=key0, key1=key1, bk=bk, ksk=ksk)
    w.P = orc.Params(n=rp.n, N=N)
    w.plan = orc.Plan(N)
    rng = np.random.default_rng(N + 11)
    w.bits = rng.integers(0, 2, N_SEL).astype(np.uint8)
    w.bits[:2] = (0, 1)
    w.sel_t = R.encrypt_selectors(rp, key1, w.bits, seed=0x5E1EC7 + N)
    w.sel_f = bk_fft(orc, w.P, w.plan, w.sel_t.reshape(-1))
    w.rows = {"plain": _random_words(rng, (N_ROWS, N)), "encrypted": R.encrypt_lut(rp, key1, _random_words(rng, (N_ROWS, N)), seed=0x7AB + N)}
    w.eng = _engine(R, rp, bk, ksk)
    w.sel = w.eng.selectors(w.sel_t)
    w.lut = {"plain": w.eng.lut(w.rows["plain"]), "encrypted": w.eng.lut_encrypted(w.rows["encrypted"])}
    w.oracle_memo = {}
    yield w
    for h in (w.sel, w.lut["plain"], w.lut["encrypted"]):
        h.close()
    w.eng.close()


def _oracle(orc, w, kind, depth, sel_idx, row0, coef=None):
    """the oracle's tree of every lookup: sel_idx [count][depth], row0 [count], coef [count] or None; computed once per world and arguments,
    shared by the tests that ask for the same lookups, and read-only"""
    key = (kind, depth, sel_idx.tobytes(), row0.tobytes(), None if coef is None else coef.tobytes())
    if key not in w.oracle_memo:
        rows = as_trlwe(w.rows[kind], w.N)
        want = np.stack([oracle_cmux_tree(orc, w.P, w.plan, w.sel_f, sel_idx[g], rows[row0[g]:row0[g] + (1 << depth)],
                                          None if coef is None else coef[g], w.ksk) for g in range(len(row0))])
        want.setflags(write=False)
        w.oracle_memo[key] = want
    return w.oracle_memo[key]


def _cuda(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()


def _tree_dev(w, kind, depth, count, sel_idx, row0, coef=None, extract=False, on=None):
    """the _dev form on the world's engine, selectors and tables, or on=(engine, selectors, table)"""
    import torch
    eng, sel, lut = on or (w.eng, w.sel, w.lut[kind])
    st = torch.cuda.current_stream().cuda_stream
    if extract:
        d_out = torch.zeros((count, w.rp.n + 1), dtype=torch.int32, device="cuda")
        eng.cmux_tree_extract_batch_dev(sel, lut, depth, d_out, count, _cuda(sel_idx), _cuda(row0), _cuda(coef), st)
    else:
        d_out = torch.zeros((count, 2, w.N), dtype=torch.int32, device="cuda")
        eng.cmux_tree_batch_dev(sel, lut, depth, d_out, count, _cuda(sel_idx), _cuda(row0), st)
    eng.sync(st)
    return d_out.cpu().numpy().view(np.uint32)


def _lookups(depth, count):
    """(sel_idx, row0, and what they mean to the oracle) twice: six selectors shared between the lookups with row0 non-zero and differing per
    lookup; then sel_idx = NULL and row0 = NULL"""
    rng = np.random.default_rng(100 * depth + count)
    shared = rng.integers(0, 6, (count, depth)).astype(np.int32)             # six selectors serve every lookup
    rows0 = rng.integers(1, N_ROWS - (1 << depth) + 1, count).astype(np.int32)
    if count > 1:
        rows0[0], rows0[1] = 1, N_ROWS - (1 << depth)                        # they differ, and one lookup ends on the table's last row
    default_idx = np.arange(count * depth, dtype=np.int32).reshape(count, depth)
    return (shared, rows0, shared, rows0), (None, None, default_idx, np.zeros(count, np.int32))


@pytest.mark.parametrize("count", [1, 5, 37])
@pytest.mark.parametrize("depth", [1, 2, 3, 4])
def test_every_word_equals_the_oracle_tree(orc, world, depth, count):
    """Plain and really encrypted tables; selectors shared between lookups with row0 non-zero and differing per lookup, then sel_idx = NULL and
    row0 = NULL; the host form against the oracle and the _dev form against the host form.  Depths 1 .. 4 cover the single-level case and odd
    and even numbers of buffer swaps; 37 lookups of depth 4 are 296 level-0 nodes, more than one workgroup, and 74 and 37 nodes at the last
    two levels: no multiple of a wave count."""
    w = world
    for kind in ("plain", "encrypted"):
        for sel_idx, row0, exp_idx, exp_row0 in _lookups(depth, count):
            want = _oracle(orc, w, kind, depth, exp_idx, exp_row0)
            got = w.eng.cmux_tree_batch(w.sel, w.lut[kind], depth, count, sel_idx, row0)
            assert got.shape == (count, 2, w.N)
            assert np.array_equal(got, want), (kind, sel_idx is None, np.flatnonzero((got != want).any(axis=(1, 2)))[:8])
            assert np.array_equal(_tree_dev(w, kind, depth, count, sel_idx, row0), got), (kind, sel_idx is None)


def test_extract_form_equals_the_oracle(orc, world):
    """identity_key_switch(sample_extract_index(result, coef)) at coef 0, 1 and N - 1, and coef = NULL; host and _dev forms."""
    w = world
    depth, count = 3, 7
    rng = np.random.default_rng(w.N + 31)
    sel_idx = rng.integers(0, N_SEL, (count, depth)).astype(np.int32)
    row0 = rng.integers(0, N_ROWS - 8 + 1, count).astype(np.int32)
    coef = np.array([0, 1, w.N - 1, w.N - 1, 1, 0, w.N // 2 + 3], np.int32)
    for kind in ("plain", "encrypted"):
        for cf, exp in ((coef, coef), (None, np.zeros(count, np.int32))):
            want = _oracle(orc, w, kind, depth, sel_idx, row0, exp)
            got = w.eng.cmux_tree_extract_batch(w.sel, w.lut[kind], depth, count, sel_idx, row0, cf)
            assert got.shape == (count, w.rp.n + 1) and np.array_equal(got, want), (kind, cf is None)
            assert np.array_equal(_tree_dev(w, kind, depth, count, sel_idx, row0, cf, extract=True), got), (kind, cf is None)


def test_extract_form_of_a_single_level(orc, world):
    """Depth 1 has no ping-pong buffers: level 0 reads the table and, in the extract form, writes the lvl1 samples itself (no node is stored
    anywhere).  Plain and encrypted tables, coef given and NULL, host and _dev forms -- first thing on a fresh engine, whose streams own no
    tree buffers yet."""
    w = world
    depth, count = 1, 5
    sel_idx = np.array([[0], [1], [1], [7], [0]], np.int32)
    row0 = np.array([0, N_ROWS - 2, 3, 3, 8], np.int32)
    coef = np.array([0, 1, w.N - 1, w.N // 2 + 3, 0], np.int32)
    e = _engine(w.R, w.rp, w.bk, w.ksk)
    try:
        with e.selectors(w.sel_t[:8]) as sel:
            for kind in ("plain", "encrypted"):
                with (e.lut(w.rows[kind]) if kind == "plain" else e.lut_encrypted(w.rows[kind])) as lut:
                    for cf, exp in ((coef, coef), (None, np.zeros(count, np.int32))):
                        want = _oracle(orc, w, kind, depth, sel_idx, row0, exp)
                        got = e.cmux_tree_extract_batch(sel, lut, depth, count, sel_idx, row0, cf)
                        assert got.shape == (count, w.rp.n + 1) and np.array_equal(got, want), (kind, cf is None)
                        assert np.array_equal(_tree_dev(w, kind, depth, count, sel_idx, row0, cf, extract=True, on=(e, sel, lut)), got), (kind, cf is None)
    finally:
        e.close()


def test_extract_form_with_the_wave_per_sample_key_switch(orc, world, monkeypatch):
    """RTFHE_KS_MM_MIN=0: a context without the matrix form of the key-switching key runs k_key_switch_ext after the tree; the same words."""
    w = world
    e = _engine(w.R, w.rp, w.bk, w.ksk, monkeypatch, {"RTFHE_KS_MM_MIN": "0"})
    try:
        depth, count = 2, 5
        sel_idx = np.array([[0, 1], [1, 0], [2, 3], [5, 5], [1, 1]], np.int32)
        row0 = np.array([0, 3, 7, 19, 1], np.int32)
        coef = np.array([0, 1, w.N - 1, 17, 0], np.int32)
        with e.selectors(w.sel_t[:6]) as sel, e.lut_encrypted(w.rows["encrypted"]) as lut:
            got = e.cmux_tree_extract_batch(sel, lut, depth, count, sel_idx, row0, coef)
        assert np.array_equal(got, _oracle(orc, w, "encrypted", depth, sel_idx, row0, coef))
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
    row0 = rng.integers(0, N_ROWS - 8 + 1, count).astype(np.int32)
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
    bad_sel[3, 1] = N_SEL
    bad_row[3] = N_ROWS - 3
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
    for kw in ({"d_sel_idx": _cuda(bad_sel), "d_row0": _cuda(row0)}, {"d_sel_idx": _cuda(sel_idx), "d_row0": _cuda(bad_row)}):
        d_out = torch.zeros((count, 2, w.N), dtype=torch.int32, device="cuda")
        w.eng.cmux_tree_batch_dev(w.sel, lut, depth, d_out, count, stream=st, **kw)
        with pytest.raises(R.RtfheError) as ei:
            w.eng.sync(st)
        assert ei.value.code == R._ffi.ERR_INVALID
        got = d_out.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[keep], ref[keep]) and not got[3].any()
    d_out = torch.zeros((count, w.rp.n + 1), dtype=torch.int32, device="cuda")
    w.eng.cmux_tree_extract_batch_dev(w.sel, lut, depth, d_out, count, _cuda(sel_idx), _cuda(row0), _cuda(bad_coef), st)
    with pytest.raises(R.RtfheError):
        w.eng.sync(st)
    assert np.array_equal(d_out.cpu().numpy().view(np.uint32)[keep], ref_x[keep])
    w.eng.sync(st)                                           # reported once
    assert np.array_equal(_tree_dev(w, "encrypted", depth, count, sel_idx, row0), ref)


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
    sel_idx = _cuda(rng.integers(0, N_SEL, (count, depth)))
    row0 = _cuda(rng.integers(0, N_ROWS - 8 + 1, count))
    coef = _cuda(rng.integers(0, w.N, count))
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
    idx2, row2, _, _ = _lookups(2, 5)[0]
    idx3, row3, _, _ = _lookups(3, 37)[0]
    d_idx2, d_row2, d_idx3, d_row3 = _cuda(idx2), _cuda(row2), _cuda(idx3), _cuda(row3)
    s = torch.cuda.Stream()
    out = torch.zeros((5, 2, w.N), dtype=torch.int32, device="cuda")
    big = torch.zeros((37, 2, w.N), dtype=torch.int32, device="cuda")
    with torch.cuda.stream(s):
        w.eng.cmux_tree_batch_dev(w.sel, lut, 2, out, 5, d_idx2, d_row2, s.cuda_stream)
        w.eng.sync(s.cuda_stream)
        eager = out.clone()
        assert np.array_equal(eager.cpu().numpy().view(np.uint32), _oracle(orc, w, "encrypted", 2, idx2, row2))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            w.eng.cmux_tree_batch_dev(w.sel, lut, 2, out, 5, d_idx2, d_row2, s.cuda_stream)
        w.eng.cmux_tree_batch_dev(w.sel, lut, 3, big, 37, d_idx3, d_row3, s.cuda_stream)
        w.eng.sync(s.cuda_stream)
        assert np.array_equal(big.cpu().numpy().view(np.uint32), _oracle(orc, w, "encrypted", 3, idx3, row3))
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
