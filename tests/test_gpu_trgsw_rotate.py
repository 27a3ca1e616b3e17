"""GPU: TRGSW blind rotation (rtfhe_trgsw_rotate_batch[_dev], rtfhe_trgsw_rotate_extract_batch[_dev]; the k_trgsw_rotate kernels).  Every word
against the oracle's rotation (tests/leveled_oracle.py: oracle_trgsw_rotate) at both N, depths 1, 2, 5 and log2 N + 1 and counts 1, 5
and 37; the extract form; in place; a second opinion from the bootstrap's own blind rotation; the composition with the CMUX tree into a fully
encrypted table lookup; skipped lookups; refusals and the capture rule.  Small TLWE dimensions as the other stage tests use: n = 40 at
N = 1024, n = 24 at N = 2048."""
import numpy as np
import pytest

import gpu_kit as gk
from kit import random_words
from leveled_kit import rotate_dev, selector_world
from leveled_oracle import oracle_trgsw_rotate

pytestmark = pytest.mark.gpu

N_SEL = 37 * 5          # sel_idx = NULL at depth 5 and 37 lookups reads selectors 0 .. 184
N_ROWS = 37


@pytest.fixture(scope="module", params=[1024, 2048], ids=lambda N: "N%d" % N)
def world(request, orc):
    """Per N: keys from the product's keygen on an engine, N_SEL selectors of known random bits (device handle, torus words and the oracle's
    spectra of them) and N_ROWS input rows with random words in both halves."""
    N = request.param
    w, rng = selector_world(orc, N, 0x207 + N, N + 12, N_SEL, 0x207A7E + N)
    w.rows = random_words(rng, (N_ROWS, 2, N))
    base = [2 * N - 1, 0, N, 1] + [int(r) for r in rng.integers(0, 2 * N, 12)]
    w.rot = lambda depth: np.array(base[:depth], np.int32)      # noqa: E731
    w.eng = gk.engine(w.R, w.rp, w.bk, w.ksk)
    w.sel = w.eng.selectors(w.sel_t)
    w.oracle_memo = {}
    yield w
    w.sel.close()
    w.eng.close()


def _oracle(orc, w, sel_idx, rot, rows, extract=False):
    """the oracle's rotation of every lookup: sel_idx [count][depth], rot [depth] or None, rows [count][2][N]; computed once per world and
    arguments, shared by the tests that ask for the same lookups, and read-only"""
    return gk.memo(w.oracle_memo, (sel_idx, None if rot is None else np.asarray(rot, np.int32), rows, extract), lambda: np.stack(
        [oracle_trgsw_rotate(orc, w.P, w.plan, w.sel_f, sel_idx[g], None if rot is None else [int(r) for r in rot], rows[g], extract, w.ksk) for g in range(len(rows))]))


def _depth(w, d):
    return w.logn + 1 if d == "logN+1" else d


@pytest.mark.parametrize("count", [1, 5, 37])
@pytest.mark.parametrize("d", [1, 2, 5, "logN+1"])
def test_every_word_equals_the_oracle_rotation(orc, world, d, count):
    """Six selectors shared between the lookups with an explicit rot -- 2N - 1, 0 (a step that changes nothing but the noise term), N (negation),
    1, then random exponents --, then rot = NULL with sel_idx = NULL (where the set has count * depth selectors, else the shared ones again);
    the host form against the oracle and the _dev form against the host form.  37 lookups are ten workgroups of four waves, the last with
    three idle ones."""
    w = world
    depth = _depth(w, d)
    rng = np.random.default_rng(100 * depth + count)
    rows = w.rows[:count]
    shared = rng.integers(0, 6, (count, depth)).astype(np.int32)
    default_idx = np.arange(count * depth, dtype=np.int32).reshape(count, depth)
    cases = [(shared, w.rot(depth), shared)]
    cases.append((None, None, default_idx) if count * depth <= N_SEL else (shared, None, shared))
    for sel_idx, rot, exp_idx in cases:
        want = _oracle(orc, w, exp_idx, rot, rows)
        got = w.eng.trgsw_rotate_batch(w.sel, rows, depth, sel_idx, rot)
        assert got.shape == (count, 2, w.N)
        assert np.array_equal(got, want), (sel_idx is None, rot is None, np.flatnonzero((got != want).any(axis=(1, 2)))[:8])
        assert np.array_equal(rotate_dev(w, rows, depth, sel_idx, rot), got), (sel_idx is None, rot is None)


def _extract_case(w):
    depth, count = 3, 7
    rng = np.random.default_rng(w.N + 32)
    return depth, count, rng.integers(0, N_SEL, (count, depth)).astype(np.int32), w.rows[5:5 + count]


def test_extract_form_equals_the_oracle(orc, world):
    """identity_key_switch(sample_extract_index(result, 0)) with an explicit rot and with rot = NULL; host and _dev forms."""
    w = world
    depth, count, sel_idx, rows = _extract_case(w)
    for rot in (w.rot(depth), None):
        want = _oracle(orc, w, sel_idx, rot, rows, extract=True)
        got = w.eng.trgsw_rotate_extract_batch(w.sel, rows, depth, sel_idx, rot)
        assert got.shape == (count, w.rp.n + 1) and np.array_equal(got, want), rot is None
        assert np.array_equal(rotate_dev(w, rows, depth, sel_idx, rot, extract=True), got), rot is None


def test_extract_form_with_the_wave_per_sample_key_switch(orc, world, monkeypatch):
    """RTFHE_KS_MM_MIN=0: a context without the matrix form of the key-switching key runs k_key_switch_ext after the rotation; the same words."""
    w = world
    depth, count, sel_idx, rows = _extract_case(w)
    e = gk.engine(w.R, w.rp, w.bk, w.ksk, monkeypatch, {"RTFHE_KS_MM_MIN": "0"})
    try:
        with e.selectors(w.sel_t) as sel:
            got = e.trgsw_rotate_extract_batch(sel, rows, depth, sel_idx, w.rot(depth))
            assert np.array_equal(got, _oracle(orc, w, sel_idx, w.rot(depth), rows, extract=True))
            assert np.array_equal(rotate_dev(w, rows, depth, sel_idx, w.rot(depth), extract=True, on=(e, sel)), got)
    finally:
        e.close()


def test_in_place_gives_the_words_of_the_out_of_place_call(world):
    w = world
    depth, count = 5, 37
    sel_idx = np.random.default_rng(w.N + 33).integers(0, N_SEL, (count, depth)).astype(np.int32)
    ref = rotate_dev(w, w.rows, depth, sel_idx, w.rot(depth))
    assert np.array_equal(rotate_dev(w, w.rows, depth, sel_idx, w.rot(depth), in_place=True), ref)
    assert np.array_equal(ref, w.eng.trgsw_rotate_batch(w.sel, w.rows, depth, sel_idx, w.rot(depth)))


def test_second_opinion_from_the_bootstraps_blind_rotation(world):
    """No oracle: the first 16 bootstrapping-key entries as a selector set, three lvl0 inputs with one common mask and different b, the start
    X^{-bbar} * (tv, 0) of the gate test vector built here, rot[k] = the mod-switched abar_k (tfhe.rs:97, 107-108) and depth 16.  Every word
    equals blind_rotate_batch(tlwe, steps=16): the new kernel's rotation convention is the bootstrap kernels'."""
    w = world
    N, n = w.N, w.rp.n
    rng = np.random.default_rng(N + 34)
    tlwe = np.tile(random_words(rng, (1, n + 1)), (3, 1))
    tlwe[:, n] = random_words(rng, 3)
    sh = 32 - w.logn - 1
    bbar = (tlwe[:, n] >> np.uint32(sh)).astype(np.int64)
    rot = (((tlwe[0, :16].astype(np.uint64) + (1 << (sh - 1))) & 0xFFFFFFFF) >> sh).astype(np.int32)
    assert (rot >= 0).all() and (rot < 2 * N).all()
    start = np.zeros((3, 2, N), np.uint32)
    c = np.arange(N)
    for g in range(3):
        e = (c + bbar[g]) % (2 * N)                                   # X^{-bbar} * tv at coefficient c is tv[c + bbar], negated past N
        start[g, 0] = np.where(e >= N, np.uint32(0xE0000000), np.uint32(0x20000000))
    want = w.eng.blind_rotate_batch(tlwe, steps=16)
    with w.eng.selectors(np.ascontiguousarray(w.bk, np.uint32).reshape(n, 2, 2 * w.rp.l, N)[:16]) as sel:
        got = w.eng.trgsw_rotate_batch(sel, start, 16, np.tile(np.arange(16, dtype=np.int32), (3, 1)), rot)
    assert np.array_equal(got, want)


def _addressed(w, bits_of, depth, addrs, salt=0):
    """sel_idx [len(addrs)][depth] over the world's selectors: entry k encrypts bit bits_of(addr, k)"""
    by_bit = [np.flatnonzero(w.bits == 0), np.flatnonzero(w.bits == 1)]
    return np.array([[by_bit[bits_of(a, k)][(3 * a + k + salt) % len(by_bit[bits_of(a, k)])] for k in range(depth)] for a in addrs], np.int32)


def test_tree_then_rotation_is_a_fully_encrypted_lookup(world):
    """A depth-2 tree over four encrypted rows of N 2-bit messages into a device buffer, then the rotate-extract _dev form at depth log2 N on
    the same stream: for several full addresses (row bits then coefficient bits) the result decrypts under key0 to the clear table's entry.
    Messages, not words: every CMUX adds its product's noise."""
    import torch
    w, R = world, world.R
    rng = np.random.default_rng(w.N + 35)
    msgs = rng.integers(0, 4, (4, w.N))
    addrs = [0, w.N - 1, w.N, 4 * w.N - 1, 2 * w.N + 1] + [int(a) for a in rng.integers(0, 4 * w.N, 5)]
    hi = _addressed(w, lambda a, k: (a >> (w.logn + k)) & 1, 2, addrs)
    lo = _addressed(w, lambda a, k: (a >> k) & 1, w.logn, addrs, salt=7)
    count = len(addrs)
    st = torch.cuda.current_stream().cuda_stream
    d_row = torch.zeros((count, 2, w.N), dtype=torch.int32, device="cuda")
    d_out = torch.zeros((count, w.rp.n + 1), dtype=torch.int32, device="cuda")
    with w.eng.lut_encrypted(R.encrypt_lut(w.rp, w.key1, R.encode_msgs(msgs, 2), seed=0xF00 + w.N)) as table:
        w.eng.cmux_tree_batch_dev(w.sel, table, 2, d_row, count, gk.to_device(hi), None, st)
        w.eng.trgsw_rotate_extract_batch_dev(w.sel, d_row, w.logn, d_out, count, gk.to_device(lo), None, st)
        w.eng.sync(st)
    got = R.decode_msgs(R.phases(w.rp, w.key0, d_out.cpu().numpy().view(np.uint32)), 2)
    assert np.array_equal(got, msgs.reshape(-1)[addrs])


def _bad_patterns(count, depth):
    """(name, sel_idx) with bad entries -1 and N_SEL, in step 0 and in the last step"""
    good = np.tile(np.arange(depth, dtype=np.int32) % 6, (count, 1))
    out = []

    def bad(name, lookups):
        idx = good.copy()
        for i, g in enumerate(lookups):
            idx[g, 0 if i % 2 == 0 else depth - 1] = -1 if (i // 2) % 2 == 0 else N_SEL
        out.append((name, idx, sorted(lookups)))

    bad("lookup 0, step 0, -1", [0])
    bad("the last lookup", [count - 1, count - 1])          # the last step (and step 0)
    if count >= 8:
        bad("a whole workgroup", [4, 5, 6, 7])
    bad("every lookup", list(range(count)))
    return good, out


def _five_lookups_behind_both_key_switches(orc, w, monkeypatch):
    """The extract form's restore kernel (k_rows_restore) on five lookups of depth 2 -- one more than a workgroup's four waves -- with lookups 0
    and 4 out of range in their LAST step only, behind the batch key switch and behind the wave-per-sample one (RTFHE_KS_MM_MIN=0): rows 0 and 4
    keep the bytes written before the call, rows 1 to 3 equal the oracle, the next sync reports the fault once."""
    import torch
    R = w.R
    depth, count, width = 2, 5, w.rp.n + 1
    st = torch.cuda.current_stream().cuda_stream
    rows = w.rows[:count]
    idx = np.tile(np.arange(depth, dtype=np.int32), (count, 1))
    idx[0, depth - 1], idx[4, depth - 1] = -1, N_SEL
    want = (0xC3000000 + 0x1001 * np.arange(count, dtype=np.uint32)[:, None] + np.arange(width, dtype=np.uint32)[None, :]).astype(np.uint32)
    before = want.copy()
    want[1:4] = _oracle(orc, w, idx[1:4], w.rot(depth), rows[1:4], extract=True)
    ext = gk.engine(R, w.rp, w.bk, w.ksk, monkeypatch, {"RTFHE_KS_MM_MIN": "0"})
    try:
        with ext.selectors(w.sel_t) as ext_sel:
            for name, e, sel in (("batch key switch", w.eng, w.sel), ("wave-per-sample key switch", ext, ext_sel)):
                d_out = gk.to_device(before, np.uint32)
                e.trgsw_rotate_extract_batch_dev(sel, gk.to_device(rows, np.uint32), depth, d_out, count, gk.to_device(idx), w.rot(depth), st)
                with pytest.raises(R.RtfheError) as ei:
                    e.sync(st)
                assert ei.value.code == R._ffi.ERR_INVALID, name
                e.sync(st)                                       # reported once
                got = d_out.cpu().numpy().view(np.uint32)
                assert np.array_equal(got[[0, 4]], before[[0, 4]]), (name, "a skipped lookup's row changed")
                assert np.array_equal(got[1:4], want[1:4]), (name, np.flatnonzero((got != want).any(axis=1)))
    finally:
        ext.close()


@pytest.mark.parametrize("form", ["rows", "extract", "extract-five"])
def test_skipped_lookups_leave_their_rows_untouched(orc, world, monkeypatch, form):
    """Device-side sel_idx with entries outside [0, n_sel): the lookup is skipped whole, its output row and the guard rows around the output keep
    every byte of a row-dependent sentinel, the valid rows equal the clean call's, sync raises exactly once and a clean call follows.
    extract-five: _five_lookups_behind_both_key_switches."""
    if form == "extract-five":
        return _five_lookups_behind_both_key_switches(orc, world, monkeypatch)
    extract = form == "extract"
    import torch
    w, R = world, world.R
    depth = 3
    st = torch.cuda.current_stream().cuda_stream
    width = (w.rp.n + 1) if extract else 2 * w.N
    for count in (1, 4, 10):
        rows = w.rows[:count]
        good, patterns = _bad_patterns(count, depth)
        clean = rotate_dev(w, rows, depth, good, w.rot(depth), extract=extract)
        sentinel = (0xA5000000 + 0x1001 * np.arange(count + 8, dtype=np.uint32)[:, None] + np.arange(width, dtype=np.uint32)[None, :]).astype(np.uint32)
        d_in = gk.to_device(rows, np.uint32)
        for name, idx, skipped in patterns:
            buf = gk.to_device(sentinel, np.uint32)
            d_out = buf[4:4 + count]                        # four guard rows on each side (the output stays 16-byte aligned)
            call = w.eng.trgsw_rotate_extract_batch_dev if extract else w.eng.trgsw_rotate_batch_dev
            call(w.sel, d_in, depth, d_out, count, gk.to_device(idx), w.rot(depth), st)
            with pytest.raises(R.RtfheError) as ei:
                w.eng.sync(st)
            assert ei.value.code == R._ffi.ERR_INVALID, name
            w.eng.sync(st)                                       # reported once
            got = buf.cpu().numpy().view(np.uint32)
            want = sentinel.copy()
            keep = np.setdiff1d(np.arange(count), skipped)
            want[4 + keep] = clean.reshape(count, width)[keep]
            assert np.array_equal(got, want), (count, name, np.flatnonzero((got != want).any(axis=1)))
        assert np.array_equal(rotate_dev(w, rows, depth, good, w.rot(depth), extract=extract), clean)


def test_refusals_leave_the_engine_usable(world):
    w, R = world, world.R
    rows = w.rows[:5]
    ref = w.eng.trgsw_rotate_batch(w.sel, rows, 2)
    N = w.N
    bad_sel = np.zeros((5, 2), np.int32)
    bad_sel[3, 1] = N_SEL
    w.eng.timer_begin()
    for call, names in ((lambda: w.eng.trgsw_rotate_batch(w.sel, rows, 0), "depth"),
                        (lambda: w.eng.trgsw_rotate_batch(w.sel, rows, 17, None, np.zeros(17, np.int32)), "depth"),
                        (lambda: w.eng.trgsw_rotate_batch(w.sel, rows, 2, None, [0, 2 * N]), "step 1"),
                        (lambda: w.eng.trgsw_rotate_batch(w.sel, rows, 2, None, [-1, 0]), "step 0"),
                        (lambda: w.eng.trgsw_rotate_extract_batch(w.sel, rows, 2, None, [0, 2 * N]), "step 1"),
                        (lambda: w.eng.trgsw_rotate_batch(w.sel, rows[:1], w.logn + 2), "rot NULL"),
                        (lambda: w.eng.trgsw_rotate_batch(w.sel, rows, 2, bad_sel), "lookup 3: sel_idx[1]"),
                        (lambda: w.eng.trgsw_rotate_extract_batch(w.sel, rows, 2, bad_sel), "lookup 3: sel_idx[1]"),
                        (lambda: w.eng.trgsw_rotate_batch(w.sel, w.rows, 6, None, np.zeros(6, np.int32)), "lookup 36")):     # sel_idx NULL: 222 selectors of 185
        with pytest.raises(R.RtfheError) as ei:
            call()
        assert ei.value.code == R._ffi.ERR_INVALID and names in str(ei.value), str(ei.value)
    assert w.eng.timer_end()[1] == 0, "the checks come before any launch"
    try:
        for b in (R._ffi.BACKEND_NTT_EXACT, R._ffi.BACKEND_FFT_SPLIT_EXACT):
            w.eng.set_backend(b)
            for call in (lambda: w.eng.trgsw_rotate_batch(w.sel, rows, 2), lambda: w.eng.trgsw_rotate_extract_batch(w.sel, rows, 2)):
                with pytest.raises(R.RtfheError) as ei:
                    call()
                assert ei.value.code == R._ffi.ERR_INVALID and "mirror" in str(ei.value)
    finally:
        w.eng.set_backend(R._ffi.BACKEND_FFT64_MIRROR)
    assert np.array_equal(w.eng.trgsw_rotate_batch(w.sel, rows, 2), ref)
    # no key-switching key: the plain form runs (a selector set does not depend on the context's keys), the extract form is refused
    bare = R.Engine(R.Params(n=w.rp.n, N=N), 0)
    try:
        sel = bare.selectors(w.sel_t[:10])
        assert np.array_equal(bare.trgsw_rotate_batch(sel, rows, 2), ref)
        with pytest.raises(R.RtfheError) as ei:
            bare.trgsw_rotate_extract_batch(sel, rows, 2)
        assert ei.value.code == R._ffi.ERR_STATE and "key-switching key" in str(ei.value)
    finally:
        bare.close()
    # ... whose context is gone now: the handle only remains to be freed
    with pytest.raises(R.RtfheError) as ei:
        w.eng.trgsw_rotate_batch(sel, rows, 2)
    assert ei.value.code == R._ffi.ERR_STATE and "destroyed" in str(ei.value)
    sel.close()
    assert np.array_equal(w.eng.trgsw_rotate_batch(w.sel, rows, 2), ref)


def test_graph_capture_without_a_prior_eager_call(world):
    """The plain _dev form allocates nothing: captured in torch.cuda.graph as the first rotation of a fresh engine on a fresh stream it replays
    to the eager words, and again after the input buffer is rewritten (rot is baked in, the buffers are read at replay).  The extract form
    inside a capture without a prior eager call on the stream is refused."""
    import torch
    w, R = world, world.R
    depth, count = 5, 37
    rng = np.random.default_rng(w.N + 36)
    sel_idx = rng.integers(0, N_SEL, (count, depth)).astype(np.int32)
    rows2 = random_words(rng, (count, 2, w.N))
    want = [w.eng.trgsw_rotate_batch(w.sel, r, depth, sel_idx, w.rot(depth)) for r in (w.rows, rows2)]
    e = gk.engine(R, w.rp, w.bk, w.ksk)
    try:
        with e.selectors(w.sel_t) as sel:
            s = torch.cuda.Stream()
            d_idx = gk.to_device(sel_idx)
            d_in = gk.to_device(w.rows, np.uint32)
            out = torch.zeros((count, 2, w.N), dtype=torch.int32, device="cuda")
            out_x = torch.zeros((count, w.rp.n + 1), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            refused = []
            with torch.cuda.stream(s):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=s):
                    e.trgsw_rotate_batch_dev(sel, d_in, depth, out, count, d_idx, w.rot(depth), s.cuda_stream)
                    try:
                        e.trgsw_rotate_extract_batch_dev(sel, d_in, depth, out_x, count, d_idx, w.rot(depth), s.cuda_stream)
                    except R.RtfheError as err:
                        refused.append(err)
                assert len(refused) == 1 and refused[0].code == R._ffi.ERR_STATE and "capture" in str(refused[0])
                for rows, exp in zip((w.rows, rows2), want):
                    d_in.copy_(gk.to_device(rows, np.uint32))
                    out.zero_()
                    g.replay()
                    torch.cuda.synchronize()
                    assert np.array_equal(out.cpu().numpy().view(np.uint32), exp)
                e.sync(s.cuda_stream)
    finally:
        e.close()


def test_leveled_lut_example(params, keys):
    """examples/leveled_lut.py at the full parameter set on an engine that holds the key-switching key only: 24 twelve-bit lookups, two address
    bits by CMUX tree and ten by rotation, each also through the fused extract form."""
    import importlib.util
    import os
    import rustfhe_amd as R
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("leveled_lut", os.path.join(root, "examples", "leveled_lut.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    e = R.Engine(R.Params(n=params.n, N=params.N), 0)
    try:
        e.load_ksk(keys.ksk)
        addr, got, want = ex.run(e, keys.key0, keys.key1, 24, seed=0x1E7E1)
        assert len(addr) == 24 and np.array_equal(got, want)
        # the fused form on the same queries: the rotation and the extraction in one call, from the tree's rows
        rng = np.random.default_rng(0x1E7E1)
        table = rng.integers(0, 4, params.N << ex.ROW_BITS)
        addr2 = rng.integers(0, table.size, 24)
        assert np.array_equal(addr2, addr)
        rows = ex.encrypted_rows(e.p, keys.key1, table, seed=0x1E7E1)
        per = e.p.nbit + ex.ROW_BITS
        idx = np.arange(24 * per, dtype=np.int32).reshape(24, per)
        with e.selectors(ex.client_query(e.p, keys.key1, addr, seed=0x1E7E1)) as sel, e.lut_encrypted(rows) as tab:
            picked = e.cmux_tree_batch(sel, tab, ex.ROW_BITS, 24, idx[:, e.p.nbit:])
            out = e.trgsw_rotate_extract_batch(sel, picked, e.p.nbit, idx[:, :e.p.nbit])
        assert np.array_equal(R.decode_msgs(R.phases(e.p, keys.key0, out), 2), want)
    finally:
        e.close()
