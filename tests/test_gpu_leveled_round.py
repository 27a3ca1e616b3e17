"""GPU: the rounded gadget decomposition of the leveled entry points (rtfhe_set_leveled_decomposition; the ROUNDED = true twins of
k_cmux_tree, k_trgsw_rotate, k_cmux_net and k_external_product).  Every word against the restatement of the tree, the rotation and the
netlist with the rounded constants (tests/leveled_round_oracle.py, which tests/test_leveled_round_host.py holds to the oracle's own three in
reference mode) at both N; second opinions between the entry points; switching the mode forth and back, and what never reads it; captures;
refusals; and what the mode buys: 6-bit rows through a depth-8 tree and a 10-step rotation.  The world is that of tests/test_gpu_cmux_tree.py:
n = 40 at N = 1024, n = 24 at N = 2048."""
import contextlib

import numpy as np
import pytest

import gpu_kit as gk
import leveled_round_oracle as lo
from kit import random_words
from leveled_kit import TREE_N_ROWS, TREE_N_SEL, net_run, rotate_dev, selector_world, tree_dev, tree_lookups
from leveled_oracle import as_trlwe, oracle_cmux_tree, oracle_trgsw_rotate, rotate_clear, three_of_five

pytestmark = pytest.mark.gpu

N_ROT = 37          # input rows of the rotation tests


@contextlib.contextmanager
def _leveled(eng, rounded=True):
    """the engine's leveled decomposition mode set for the block and restored after it"""
    R = _R()
    before = eng.leveled_decomposition()
    eng.set_leveled_decomposition(R._ffi.DECOMP_ROUNDED if rounded else R._ffi.DECOMP_REFERENCE)
    try:
        yield eng
    finally:
        eng.set_leveled_decomposition(before)


def _R():
    import rustfhe_amd as R
    return R


@pytest.fixture(scope="module", params=[1024, 2048], ids=lambda N: "N%d" % N)
def world(request, orc):
    """Per N: keys from the product's keygen on an engine (in reference mode: every test sets the mode it wants around its calls), TREE_N_SEL
    selectors of known random bits (device handle, torus words and spectra), one plain and one really encrypted table of TREE_N_ROWS random rows,
    N_ROT random input rows of the rotation."""
    N = request.param
    w, rng = selector_world(orc, N, 0x17E + N, N + 17, TREE_N_SEL, 0x5E1EC9 + N)
    R = w.R
    w.rows = {"plain": random_words(rng, (TREE_N_ROWS, N)), "encrypted": R.encrypt_lut(w.rp, w.key1, random_words(rng, (TREE_N_ROWS, N)), seed=0x7AD + N)}
    w.rot_rows = random_words(rng, (N_ROT, 2, N))
    base = [2 * N - 1, 0, N, 1] + [int(r) for r in rng.integers(0, 2 * N, 12)]
    w.rot = lambda depth: np.array(base[:depth], np.int32)      # noqa: E731
    w.eng = gk.engine(R, w.rp, w.bk, w.ksk)
    assert w.eng.leveled_decomposition() == R._ffi.DECOMP_REFERENCE, "the mode is the reference's until set"
    w.sel = w.eng.selectors(w.sel_t)
    w.lut = {"plain": w.eng.lut(w.rows["plain"]), "encrypted": w.eng.lut_encrypted(w.rows["encrypted"])}
    w.memo = {}
    yield w
    for h in (w.sel, w.lut["plain"], w.lut["encrypted"]):
        h.close()
    w.eng.close()


def _want_tree(w, kind, depth, sel_idx, row0, coef=None):
    """the restated tree of every lookup in rounded mode; computed once per world and arguments, shared and read-only"""
    def compute():
        rows = as_trlwe(w.rows[kind], w.N)
        return np.stack([lo.cmux_tree(w.P, w.plan, w.sel_f, sel_idx[g], rows[row0[g]:row0[g] + (1 << depth)], None if coef is None else coef[g], w.ksk)
                         for g in range(len(row0))])
    return gk.memo(w.memo, ("tree", kind, depth, sel_idx, row0, coef), compute)


def _want_rotate(w, sel_idx, rot, rows, extract=False):
    """the restated rotation of every lookup in rounded mode; computed once per world and arguments, shared and read-only"""
    return gk.memo(w.memo, ("rot", sel_idx, None if rot is None else np.asarray(rot, np.int32), rows, extract), lambda: np.stack(
        [lo.trgsw_rotate(w.P, w.plan, w.sel_f, sel_idx[g], None if rot is None else [int(r) for r in rot], rows[g], extract, w.ksk) for g in range(len(rows))]))


# ---- tree ----
@pytest.mark.parametrize("count", [1, 37])
@pytest.mark.parametrize("depth", [1, 2, 4])
def test_tree_equals_the_restatement(world, depth, count):
    """Rounded mode, plain and really encrypted tables; six selectors shared between the lookups with row0 non-zero and differing, then
    sel_idx = NULL and row0 = NULL; the host form against the restatement and the _dev form against the host form.  37 lookups of depth 4
    are 296 / 74 / 37 nodes at the last three levels: more than one workgroup, and no multiple of the wave count."""
    w = world
    with _leveled(w.eng):
        for kind in ("plain", "encrypted"):
            for sel_idx, row0, exp_idx, exp_row0 in tree_lookups(depth, count):
                want = _want_tree(w, kind, depth, exp_idx, exp_row0)
                got = w.eng.cmux_tree_batch(w.sel, w.lut[kind], depth, count, sel_idx, row0)
                assert got.shape == (count, 2, w.N)
                assert np.array_equal(got, want), (kind, sel_idx is None, np.flatnonzero((got != want).any(axis=(1, 2)))[:8])
                assert np.array_equal(tree_dev(w, kind, depth, count, sel_idx, row0), got), (kind, sel_idx is None)


def test_tree_extract_form_equals_the_restatement(world):
    """identity_key_switch(sample_extract_index(result, coef)) of the rounded tree at coef 0, 1 and N - 1, and coef = NULL; host and _dev."""
    w = world
    depth, count = 3, 7
    rng = np.random.default_rng(w.N + 31)
    sel_idx = rng.integers(0, TREE_N_SEL, (count, depth)).astype(np.int32)
    row0 = rng.integers(0, TREE_N_ROWS - 8 + 1, count).astype(np.int32)
    coef = np.array([0, 1, w.N - 1, w.N - 1, 1, 0, w.N // 2 + 3], np.int32)
    with _leveled(w.eng):
        for kind in ("plain", "encrypted"):
            for cf, exp in ((coef, coef), (None, np.zeros(count, np.int32))):
                want = _want_tree(w, kind, depth, sel_idx, row0, exp)
                got = w.eng.cmux_tree_extract_batch(w.sel, w.lut[kind], depth, count, sel_idx, row0, cf)
                assert got.shape == (count, w.rp.n + 1) and np.array_equal(got, want), (kind, cf is None)
                assert np.array_equal(tree_dev(w, kind, depth, count, sel_idx, row0, cf, extract=True), got), (kind, cf is None)


# ---- rotation ----
@pytest.mark.parametrize("count", [1, 37])
@pytest.mark.parametrize("d", [1, 2, 5, "logN+1"])
def test_rotation_equals_the_restatement(world, d, count):
    """Rounded mode: six shared selectors with an explicit rot (2N - 1, 0, N, 1, then random exponents), then the default rot with
    sel_idx = NULL where the set has count * depth selectors (else the shared ones again); host form against the restatement, _dev form and
    the in-place _dev form against the host form."""
    w = world
    depth = w.logn + 1 if d == "logN+1" else d
    rng = np.random.default_rng(100 * depth + count)
    rows = w.rot_rows[:count]
    shared = rng.integers(0, 6, (count, depth)).astype(np.int32)
    default_idx = np.arange(count * depth, dtype=np.int32).reshape(count, depth)
    cases = [(shared, w.rot(depth), shared), (None, None, default_idx) if count * depth <= TREE_N_SEL else (shared, None, shared)]
    with _leveled(w.eng):
        for sel_idx, rot, exp_idx in cases:
            want = _want_rotate(w, exp_idx, rot, rows)
            got = w.eng.trgsw_rotate_batch(w.sel, rows, depth, sel_idx, rot)
            assert np.array_equal(got, want), (sel_idx is None, rot is None, np.flatnonzero((got != want).any(axis=(1, 2)))[:8])
            assert np.array_equal(rotate_dev(w, rows, depth, sel_idx, rot), got), (sel_idx is None, rot is None)
            assert np.array_equal(rotate_dev(w, rows, depth, sel_idx, rot, in_place=True), got), (sel_idx is None, rot is None, "in place")


def test_rotation_extract_form_equals_the_restatement(world):
    w = world
    depth, count = 3, 7
    sel_idx = np.random.default_rng(w.N + 32).integers(0, TREE_N_SEL, (count, depth)).astype(np.int32)
    rows = w.rot_rows[5:5 + count]
    with _leveled(w.eng):
        for rot in (w.rot(depth), None):
            want = _want_rotate(w, sel_idx, rot, rows, extract=True)
            got = w.eng.trgsw_rotate_extract_batch(w.sel, rows, depth, sel_idx, rot)
            assert got.shape == (count, w.rp.n + 1) and np.array_equal(got, want), rot is None
            assert np.array_equal(rotate_dev(w, rows, depth, sel_idx, rot, extract=True), got), rot is None


@pytest.mark.parametrize("extract", [False, True], ids=["rows", "extract"])
def test_rotation_skips_lookups_with_a_bad_index(world, extract):
    """Rounded mode, device-side sel_idx with entries -1 and TREE_N_SEL in lookups 1 and 4 of 6: those output rows and the guard rows keep every
    byte of a sentinel, the other rows are the clean call's, sync raises once."""
    import torch
    w, R = world, world.R
    depth, count = 3, 6
    st = torch.cuda.current_stream().cuda_stream
    width = (w.rp.n + 1) if extract else 2 * w.N
    rows = w.rot_rows[:count]
    good = np.tile(np.arange(depth, dtype=np.int32), (count, 1))
    bad = good.copy()
    bad[1, 0], bad[4, depth - 1] = -1, TREE_N_SEL
    with _leveled(w.eng):
        clean = rotate_dev(w, rows, depth, good, w.rot(depth), extract=extract)
        assert np.array_equal(clean[0], _want_rotate(w, good[:1], w.rot(depth), rows[:1], extract)[0])
        sentinel = (0xA5000000 + 0x1001 * np.arange(count + 8, dtype=np.uint32)[:, None] + np.arange(width, dtype=np.uint32)[None, :]).astype(np.uint32)
        buf = gk.to_device(sentinel, np.uint32)
        call = w.eng.trgsw_rotate_extract_batch_dev if extract else w.eng.trgsw_rotate_batch_dev
        call(w.sel, gk.to_device(rows, np.uint32), depth, buf[4:4 + count], count, gk.to_device(bad), w.rot(depth), st)
        with pytest.raises(R.RtfheError) as ei:
            w.eng.sync(st)
        assert ei.value.code == R._ffi.ERR_INVALID
        w.eng.sync(st)                                       # reported once
    got = buf.cpu().numpy().view(np.uint32)
    want = sentinel.copy()
    keep = np.array([0, 2, 3, 5])
    want[4 + keep] = clean.reshape(count, width)[keep]
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))


# ---- netlists ----
def test_reduced_diagram_equals_the_restated_net(world):
    """bdd_netlist(5, three_of_five) recorded with rounded=True on an engine in reference mode: 5 replicas over the first two table rows from
    row0 on, plain and encrypted, word for word with the restated net; the engine's mode is restored."""
    w, R = world, world.R
    net = R.bdd_netlist(5, three_of_five)
    count = 5
    rng = np.random.default_rng(w.N + 41)
    sel_idx = rng.integers(0, TREE_N_SEL, (count, 5)).astype(np.int32)
    row0 = rng.integers(0, TREE_N_ROWS - 2 + 1, count).astype(np.int32)
    import torch
    st = torch.cuda.current_stream().cuda_stream
    for kind in ("plain", "encrypted"):
        rows = as_trlwe(w.rows[kind], w.N)
        want = np.stack([lo.cmux_net(w.P, w.plan, w.sel_f, sel_idx[g], rows[row0[g]:], net) for g in range(count)])
        d_out = torch.zeros((count, 3, 2, w.N), dtype=torch.int32, device="cuda")
        with w.eng.cmux_circuit(net, w.sel, w.lut[kind], d_out, count, gk.to_device(sel_idx), gk.to_device(row0), rounded=True) as c:
            assert c.rounded and w.eng.leveled_decomposition() == R._ffi.DECOMP_REFERENCE
            c.launch(st)
            w.eng.sync(st)
        assert np.array_equal(d_out.cpu().numpy().view(np.uint32), want), kind


def test_tree_and_rotation_netlists_equal_their_entry_points_in_rounded_mode(world):
    """No restatement: cmux_tree_netlist(3) and trgsw_rotate_netlist(5) recorded in rounded mode, word for word with cmux_tree_batch and
    trgsw_rotate_batch in rounded mode -- and not with their reference-mode words."""
    w = world
    count = 6
    rng = np.random.default_rng(w.N + 43)
    sel3 = rng.integers(0, TREE_N_SEL, (count, 3)).astype(np.int32)
    sel5 = rng.integers(0, TREE_N_SEL, (count, 5)).astype(np.int32)
    row0 = rng.integers(0, TREE_N_ROWS - 8 + 1, count).astype(np.int32)
    rot = [2 * w.N - 1, 0, w.N, 1, int(rng.integers(0, 2 * w.N))]
    rows = as_trlwe(w.rows["encrypted"], w.N)[:count]
    ref_tree = w.eng.cmux_tree_batch(w.sel, w.lut["encrypted"], 3, count, sel3, row0)
    ref_rot = w.eng.trgsw_rotate_batch(w.sel, rows, 5, sel5, rot)
    with _leveled(w.eng):
        for kind in ("plain", "encrypted"):
            want = w.eng.cmux_tree_batch(w.sel, w.lut[kind], 3, count, sel3, row0)
            assert np.array_equal(net_run(w, w.R.cmux_tree_netlist(3), w.lut[kind], count, sel3, row0)[:, 0], want), kind
        assert not np.array_equal(want, ref_tree)
        want = w.eng.trgsw_rotate_batch(w.sel, rows, 5, sel5, rot)
        got = net_run(w, w.R.trgsw_rotate_netlist(5, rot), w.lut["encrypted"], count, sel5, np.arange(count, dtype=np.int32))
        assert np.array_equal(got[:, 0], want) and not np.array_equal(want, ref_rot)


def test_a_cmux_circuit_keeps_the_mode_it_was_recorded_in(world):
    """cmux_tree_netlist(2) recorded once per mode (rounded=None: the mode in force); each circuit replays its own mode's words whatever the
    context is set to at replay, in both directions."""
    import torch
    w = world
    count = 5
    sel_idx = np.random.default_rng(w.N + 45).integers(0, TREE_N_SEL, (count, 2)).astype(np.int32)
    lut = w.lut["encrypted"]
    net = w.R.cmux_tree_netlist(2)
    st = torch.cuda.current_stream().cuda_stream
    want, circ, outs = {}, {}, {}
    try:
        for rounded in (False, True):
            with _leveled(w.eng, rounded):
                want[rounded] = w.eng.cmux_tree_batch(w.sel, lut, 2, count, sel_idx)
                outs[rounded] = torch.zeros((count, 1, 2, w.N), dtype=torch.int32, device="cuda")
                circ[rounded] = w.eng.cmux_circuit(net, w.sel, lut, outs[rounded], count, gk.to_device(sel_idx))
                assert circ[rounded].rounded == rounded
        assert not np.array_equal(want[False], want[True])
        for at_replay in (False, True, False):
            with _leveled(w.eng, at_replay):
                for rounded in (False, True):
                    outs[rounded].zero_()
                    circ[rounded].launch(st)
                    w.eng.sync(st)
                    assert np.array_equal(outs[rounded].cpu().numpy().view(np.uint32)[:, 0], want[rounded]), (at_replay, rounded)
    finally:
        for c in circ.values():
            c.close()


# ---- second opinion ----
def test_second_opinion_from_external_products_alone(world):
    """No restatement: a context with Params(n = depth) takes the selector set as its bootstrapping key, and the depth-3 tree is run level by
    level as external_product_batch(idx, r1 - r0) + r0 in numpy, both in rounded leveled mode.  Every word equals the rounded tree call's, and
    differs from the reference-mode product's."""
    w, R = world, world.R
    depth, count = 3, 5
    rng = np.random.default_rng(w.N + 47)
    sel_idx = rng.integers(0, depth, (count, depth)).astype(np.int32)
    row0 = rng.integers(0, TREE_N_ROWS - 8 + 1, count).astype(np.int32)
    e = R.Engine(R.Params(n=depth, N=w.N), 0)
    try:
        e.load_bk_torus(w.sel_t[:depth].reshape(-1))
        for kind in ("plain", "encrypted"):
            table = as_trlwe(w.rows[kind], w.N)
            first = np.stack([table[r:r + 8] for r in row0])                                # [count][8][2][N]
            nodes = first
            with _leveled(e):
                for k in range(depth):
                    r0, r1 = nodes[:, 0::2], nodes[:, 1::2]
                    idx = np.repeat(sel_idx[:, k], r0.shape[1])
                    nodes = e.external_product_batch(idx, (r1 - r0).reshape(-1, 2, w.N)).reshape(r0.shape) + r0
                with e.selectors(w.sel_t[:depth]) as sel, (e.lut(w.rows[kind]) if kind == "plain" else e.lut_encrypted(w.rows[kind])) as lut:
                    assert np.array_equal(e.cmux_tree_batch(sel, lut, depth, count, sel_idx, row0), nodes[:, 0]), kind
            r0, r1 = first[:, 0::2], first[:, 1::2]
            d = (r1 - r0).reshape(-1, 2, w.N)
            idx = np.repeat(sel_idx[:, 0], r0.shape[1])
            ref = e.external_product_batch(idx, d)
            with _leveled(e):
                assert not np.array_equal(e.external_product_batch(idx, d), ref), kind
            assert np.array_equal(e.external_product_batch(idx, d), ref), kind
    finally:
        e.close()


# ---- mode switching ----
def _leveled_calls(w):
    rng = np.random.default_rng(w.N + 51)
    count = 5
    sel3 = rng.integers(0, TREE_N_SEL, (count, 3)).astype(np.int32)
    row0 = rng.integers(0, TREE_N_ROWS - 8 + 1, count).astype(np.int32)
    rows = w.rot_rows[:count]
    idx = rng.integers(0, w.rp.n, count).astype(np.int32)
    net = w.R.cmux_tree_netlist(3)

    def run():
        return [w.eng.cmux_tree_batch(w.sel, w.lut["encrypted"], 3, count, sel3, row0), w.eng.cmux_tree_extract_batch(w.sel, w.lut["plain"], 3, count, sel3, row0),
                w.eng.trgsw_rotate_batch(w.sel, rows, 3, sel3, w.rot(3)), w.eng.trgsw_rotate_extract_batch(w.sel, rows, 3, sel3),
                net_run(w, net, w.lut["encrypted"], count, sel3, row0), w.eng.external_product_batch(idx, rows)]
    return run, (sel3, row0, rows)


def test_switching_back_gives_the_oracles_words_again(orc, world):
    w, R = world, world.R
    run, (sel3, row0, rows) = _leveled_calls(w)
    before = run()
    table = as_trlwe(w.rows["encrypted"], w.N)
    assert np.array_equal(before[0][0], oracle_cmux_tree(orc, w.P, w.plan, w.sel_f, sel3[0], table[row0[0]:row0[0] + 8]))
    assert np.array_equal(before[2][0], oracle_trgsw_rotate(orc, w.P, w.plan, w.sel_f, sel3[0], [int(r) for r in w.rot(3)], rows[0]))
    with _leveled(w.eng):
        assert w.eng.leveled_decomposition() == R._ffi.DECOMP_ROUNDED
        rounded = run()
    assert w.eng.leveled_decomposition() == R._ffi.DECOMP_REFERENCE
    after = run()
    for a, b, r in zip(before, after, rounded):
        assert np.array_equal(a, b) and not np.array_equal(a, r)


def test_the_pbs_mode_alone_leaves_every_leveled_word_the_references(world):
    w, R = world, world.R
    run, _ = _leveled_calls(w)
    ref = run()
    w.eng.set_decomposition(R._ffi.DECOMP_ROUNDED)
    try:
        assert w.eng.leveled_decomposition() == R._ffi.DECOMP_REFERENCE, "neither setter touches the other's state"
        got = run()
    finally:
        w.eng.set_decomposition(R._ffi.DECOMP_REFERENCE)
    for a, b in zip(ref, got):
        assert np.array_equal(a, b)


def test_the_leveled_mode_alone_leaves_pbs_gates_mux_bootstrap_blind_rotation_and_pack(world):
    """... in both states of the PBS family's own mode, which the leveled setter does not touch."""
    w, R = world, world.R
    rng = np.random.default_rng(w.N + 53)
    n1 = w.rp.n + 1
    a, b, c = (random_words(rng, (37, n1)) for _ in range(3))
    tv, trl = random_words(rng, (2, w.N)), random_words(rng, (2, 2, w.N))
    idx = rng.integers(0, 2, 37).astype(np.int32)
    pk = R.packing_keygen(w.rp, w.key0, w.key1, 0xBACC + w.N)
    with w.eng.lut(tv) as plain, w.eng.lut_encrypted(trl) as enc, w.eng.packing_key(pk) as key:
        def run():
            return [w.eng.gate_batch(R.NAND, a, b), w.eng.gate_batch(R.XOR, a, b), w.eng.mux_batch(c, a, b), w.eng.bootstrap_batch(a), w.eng.blind_rotate_batch(a),
                    w.eng.pbs_batch(plain, a, idx), w.eng.pbs_many_batch(plain, a, 4, idx), w.eng.pbs_batch(enc, a, idx), w.eng.pack_batch(key, a[:36].reshape(9, 4, n1), 4)]
        for pbs_mode in (R._ffi.DECOMP_REFERENCE, R._ffi.DECOMP_ROUNDED):
            w.eng.set_decomposition(pbs_mode)
            try:
                ref = run()
                with _leveled(w.eng):
                    assert w.eng.decomposition() == pbs_mode
                    got = run()
            finally:
                w.eng.set_decomposition(R._ffi.DECOMP_REFERENCE)
            for x, y in zip(ref, got):
                assert np.array_equal(x, y), pbs_mode


# ---- captures ----
def test_captured_tree_replays_the_eager_words_in_rounded_mode(world):
    """The eager calls the header asks for run in REFERENCE mode (they size the stream's buffers; every launch grants both twins their LDS);
    the capture is then made in rounded mode and replays the rounded host words, also after the context has been switched back."""
    import torch
    w = world
    depth, count = 3, 37
    rng = np.random.default_rng(w.N + 61)
    sel_idx, row0, coef = (rng.integers(0, hi, shape).astype(np.int32) for hi, shape in ((TREE_N_SEL, (count, depth)), (TREE_N_ROWS - 8 + 1, count), (w.N, count)))
    lut = w.lut["encrypted"]
    with _leveled(w.eng):
        want = w.eng.cmux_tree_batch(w.sel, lut, depth, count, sel_idx, row0)
        want_x = w.eng.cmux_tree_extract_batch(w.sel, lut, depth, count, sel_idx, row0, coef)
    e = gk.engine(w.R, w.rp, w.bk, w.ksk)
    try:
        with e.selectors(w.sel_t) as sel, e.lut_encrypted(w.rows["encrypted"]) as elut:
            s = torch.cuda.Stream()
            d_idx, d_row0, d_coef = gk.to_device(sel_idx), gk.to_device(row0), gk.to_device(coef)
            out = torch.zeros((count, 2, w.N), dtype=torch.int32, device="cuda")
            out_x = torch.zeros((count, w.rp.n + 1), dtype=torch.int32, device="cuda")

            def both():
                e.cmux_tree_batch_dev(sel, elut, depth, out, count, d_idx, d_row0, s.cuda_stream)
                e.cmux_tree_extract_batch_dev(sel, elut, depth, out_x, count, d_idx, d_row0, d_coef, s.cuda_stream)

            with torch.cuda.stream(s):
                both()                                               # eager, reference mode
                e.sync(s.cuda_stream)
                assert not np.array_equal(out.cpu().numpy().view(np.uint32), want)
                g = torch.cuda.CUDAGraph()
                with _leveled(e):
                    with torch.cuda.graph(g, stream=s):
                        both()
                for _ in range(2):                                   # the context is back in reference mode: the twins are baked in
                    out.zero_()
                    out_x.zero_()
                    g.replay()
                    torch.cuda.synchronize()
                    assert np.array_equal(out.cpu().numpy().view(np.uint32), want) and np.array_equal(out_x.cpu().numpy().view(np.uint32), want_x)
                e.sync(s.cuda_stream)
    finally:
        e.close()


def test_captured_rotation_without_a_prior_eager_call_in_rounded_mode(world):
    """A fresh engine whose selector set was created in reference mode, switched to rounded mode, captures the plain _dev form as its first
    rotation on a fresh stream: the set's creation granted both twins their LDS.  The replay gives the rounded host words."""
    import torch
    w = world
    depth, count = 5, 37
    sel_idx = np.random.default_rng(w.N + 63).integers(0, TREE_N_SEL, (count, depth)).astype(np.int32)
    with _leveled(w.eng):
        want = w.eng.trgsw_rotate_batch(w.sel, w.rot_rows, depth, sel_idx, w.rot(depth))
    e = gk.engine(w.R, w.rp, w.bk, w.ksk)
    try:
        with e.selectors(w.sel_t) as sel:
            s = torch.cuda.Stream()
            d_idx, d_in = gk.to_device(sel_idx), gk.to_device(w.rot_rows, np.uint32)
            out = torch.zeros((count, 2, w.N), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                g = torch.cuda.CUDAGraph()
                with _leveled(e):
                    with torch.cuda.graph(g, stream=s):
                        e.trgsw_rotate_batch_dev(sel, d_in, depth, out, count, d_idx, w.rot(depth), s.cuda_stream)
                for _ in range(2):
                    out.zero_()
                    g.replay()
                    torch.cuda.synchronize()
                    assert np.array_equal(out.cpu().numpy().view(np.uint32), want)
                e.sync(s.cuda_stream)
    finally:
        e.close()


# ---- refusals and contexts ----
def test_exact_backends_refuse_the_rounded_external_product_and_accept_the_setter(world):
    w, R = world, world.R
    rows = w.rot_rows[:5]
    idx = np.arange(5, dtype=np.int32)
    ref = w.eng.external_product_batch(idx, rows)
    try:
        for b in (R._ffi.BACKEND_NTT_EXACT, R._ffi.BACKEND_FFT_SPLIT_EXACT):
            w.eng.set_backend(b)
            exact = w.eng.external_product_batch(idx, rows)          # reference mode: as before
            for mode in (R._ffi.DECOMP_ROUNDED, R._ffi.DECOMP_REFERENCE, R._ffi.DECOMP_ROUNDED):
                w.eng.set_leveled_decomposition(mode)
                assert w.eng.leveled_decomposition() == mode
            with pytest.raises(R.RtfheError) as ei:
                w.eng.external_product_batch(idx, rows)
            assert ei.value.code == R._ffi.ERR_INVALID and "mirror" in str(ei.value)
            w.eng.set_leveled_decomposition(R._ffi.DECOMP_REFERENCE)
            assert np.array_equal(w.eng.external_product_batch(idx, rows), exact)
    finally:
        w.eng.set_leveled_decomposition(R._ffi.DECOMP_REFERENCE)
        w.eng.set_backend(R._ffi.BACKEND_FFT64_MIRROR)
    assert np.array_equal(w.eng.external_product_batch(idx, rows), ref)


def test_bad_modes_are_refused_and_leave_the_context_clean(world):
    w, R = world, world.R
    try:
        for start in (R._ffi.DECOMP_ROUNDED, R._ffi.DECOMP_REFERENCE):
            w.eng.set_leveled_decomposition(start)
            for bad in (2, -1, 255, 1 << 30):
                with pytest.raises(R.RtfheError) as ei:
                    w.eng.set_leveled_decomposition(bad)
                assert ei.value.code == R._ffi.ERR_INVALID and "decomposition" in str(ei.value)
                assert w.eng.leveled_decomposition() == start and w.eng.decomposition() == R._ffi.DECOMP_REFERENCE
            w.eng.sync()
    finally:
        w.eng.set_leveled_decomposition(R._ffi.DECOMP_REFERENCE)


def test_two_entry_context_takes_the_mode(world):
    """The setter sets every entry; the leveled calls run on the primary, so what shows is: the getter, the rounded words of the tree and the
    rotation equal to the single-device engine's, and gates sharded over both entries unchanged."""
    w, R = world, world.R
    rng = np.random.default_rng(w.N + 71)
    count = 5
    sel3 = rng.integers(0, TREE_N_SEL, (count, 3)).astype(np.int32)
    a, b = random_words(rng, (7, w.rp.n + 1)), random_words(rng, (7, w.rp.n + 1))
    gates = w.eng.gate_batch(R.NAND, a, b)
    with _leveled(w.eng):
        want = w.eng.cmux_tree_batch(w.sel, w.lut["plain"], 3, count, sel3), w.eng.trgsw_rotate_batch(w.sel, w.rot_rows[:count], 3, sel3)
    multi = gk.engine(R, w.rp, w.bk, w.ksk, devices=[0, 0])
    try:
        assert multi.device_count() == 2 and multi.leveled_decomposition() == R._ffi.DECOMP_REFERENCE
        multi.set_leveled_decomposition(R._ffi.DECOMP_ROUNDED)
        assert multi.leveled_decomposition() == R._ffi.DECOMP_ROUNDED and multi.decomposition() == R._ffi.DECOMP_REFERENCE
        with multi.selectors(w.sel_t) as sel, multi.lut(w.rows["plain"]) as lut:
            assert np.array_equal(multi.cmux_tree_batch(sel, lut, 3, count, sel3), want[0])
            assert np.array_equal(multi.trgsw_rotate_batch(sel, w.rot_rows[:count], 3, sel3), want[1])
        assert np.array_equal(multi.gate_batch(R.NAND, a, b), gates)
    finally:
        multi.close()


# ---- meaning ----
@pytest.fixture(scope="module")
def meaning():
    """leveled_round_oracle.gpu_meaning_world on a bare engine (the leveled path needs no key of the context); the CPU suite runs the same
    inputs through the restatement first (tests/test_leveled_round_host.py: test_seeds_of_the_gpu_meaning_tests)."""
    R = _R()
    m = lo.gpu_meaning_world(R)
    m.eng = R.Engine(m.rp, 0)
    m.lut = {"plain": m.eng.lut(m.plain), "encrypted": m.eng.lut_encrypted(m.rows["encrypted"])}
    yield m
    for h in m.lut.values():
        h.close()
    m.eng.close()


def _decoded(m, out):
    R = _R()
    return R.decode_msgs(R.trlwe_phase(m.rp, m.key1, out), lo.MSG_BITS)


def test_6bit_rows_through_the_depth8_tree(meaning):
    """N = 1024, 256 rows of N random 6-bit messages, plain and encrypted, addresses 0, 255 and 0xA5 in one batch: rounded mode decodes every
    coefficient of every lookup; reference mode on the same ciphertexts decodes wrong at address 255 (on the CPU: 500-odd of 1,024)."""
    m = meaning
    addrs = m.TREE_ADDRS
    with m.eng.selectors(np.concatenate([m.tree_sel[a] for a in addrs])) as sel:
        for kind in ("plain", "encrypted"):
            with _leveled(m.eng):
                got = _decoded(m, m.eng.cmux_tree_batch(sel, m.lut[kind], 8, len(addrs)))
            assert np.array_equal(got, m.msgs[list(addrs)]), kind
            ref = _decoded(m, m.eng.cmux_tree_batch(sel, m.lut[kind], 8, len(addrs)))
            assert not np.array_equal(ref[addrs.index(255)], m.msgs[255]), kind


def test_6bit_rows_through_the_10_step_rotation(meaning):
    """The same for the rotation with the default rot at addresses 0, 1023 and 0x2B5 of row ROT_ROW: X^-addr * row at every coefficient in
    rounded mode; reference mode decodes wrong at address 1023."""
    m = meaning
    addrs = m.ROT_ADDRS
    with m.eng.selectors(np.concatenate([m.rot_sel[a] for a in addrs])) as sel:
        for kind in ("plain", "encrypted"):
            rows = np.repeat(m.rows[kind][m.ROT_ROW][None], len(addrs), axis=0)
            want = np.stack([_R().decode_msgs(rotate_clear(m.plain[m.ROT_ROW], a), lo.MSG_BITS) for a in addrs])
            with _leveled(m.eng):
                got = _decoded(m, m.eng.trgsw_rotate_batch(sel, rows, 10))
            assert np.array_equal(got, want), kind
            ref = _decoded(m, m.eng.trgsw_rotate_batch(sel, rows, 10))
            assert not np.array_equal(ref[addrs.index(1023)], want[addrs.index(1023)]), kind


def test_leveled_lut_6bit_example(params, keys):
    """examples/leveled_lut_6bit.py at the full parameter set on an engine without keys, at a small size: 4 eighteen-bit lookups (the all-ones
    address and address 0 among them) into 2^8 N six-bit entries; all right in rounded mode, and the engine's mode is restored."""
    import importlib.util
    import os
    R = _R()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("leveled_lut_6bit", os.path.join(root, "examples", "leveled_lut_6bit.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    e = R.Engine(R.Params(n=params.n, N=params.N), 0)
    try:
        addr, want, got, ref = ex.run(e, keys.key1, 4, seed=0x6B17)
        assert len(addr) == 4 and addr[0] == (params.N << ex.ROW_BITS) - 1 and addr[1] == 0
        assert np.array_equal(got, want) and len(ref) == 4
        assert e.leveled_decomposition() == R._ffi.DECOMP_REFERENCE
    finally:
        e.close()
