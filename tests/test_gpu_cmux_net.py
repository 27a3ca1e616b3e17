"""GPU: CMUX netlists (rtfhe_cmux_circuit_create, rtfhe_trgsw_update; the k_cmux_net kernels).  Every word against the oracle's netlist
(tests/leveled_oracle.py: oracle_cmux_net) at both N on a mixed netlist of 11 nodes, plain and encrypted tables, counts 1, 5 and 37, both
output forms and both key-switch routes; second opinions from the tree and the rotation entry points; replay, selector update and a destroyed
set; skipped replicas; what a comparator means; refusals.  Small TLWE dimensions as the tree tests use: n = 40 at N = 1024, n = 24 at N = 2048."""
import numpy as np
import pytest

import gpu_kit as gk
from kit import random_words
from leveled_kit import net_run, selector_world
from leveled_oracle import as_trlwe, comparator_netlist, oracle_cmux_net
from pbs_oracle import bk_fft

pytestmark = pytest.mark.gpu

N_VARS = 5
N_SEL = 37 * N_VARS      # sel_idx = NULL at 37 replicas reads selectors 0 .. 184
N_ROWS = 8 + 7           # the mixed netlist names rows 0 .. 7, row0 up to 7
SENTINEL = 0x5A5A5A5A


def mixed_netlist(R, N, coefs=None):
    """11 nodes on 5 variables over 4 levels of 4, 3, 3 and 1 nodes (no level is a multiple of the four waves of a workgroup): node 5 has two
    parents (7 and 9); nodes 3 (over a row) and 9 (over a node) have hi == lo and rot != 0; rots 0, 1, N and 2N - 1; rows at level 0 and, as
    node 8's hi, at level 2; a node as hi over a row as lo (5) and the reverse (6, 8); outputs at the last level, at level 1 and at level 2."""
    net = R.CmuxNetlist(N_VARS)
    row = net.row
    n0 = net.node(0, row(1), row(0))
    n1 = net.node(1, row(3), row(2), rot=1)
    n2 = net.node(2, row(5), row(4), rot=N)
    net.node(3, row(0), row(0), rot=2 * N - 1)
    n4 = net.node(4, n0, n1)
    n5 = net.node(0, n1, row(4), rot=3)
    n6 = net.node(1, row(6), n2)
    n7 = net.node(2, n4, n5)
    n8 = net.node(3, row(7), n6, rot=17)
    n9 = net.node(4, n5, n5, rot=5)
    n10 = net.node(0, n7, n8)
    for k, ref in enumerate((n10, n4, n9)):
        net.output(ref, None if coefs is None else coefs[k])
    assert [len(l) for l in net.levels()] == [4, 3, 3, 1]
    return net


@pytest.fixture(scope="module", params=[1024, 2048], ids=lambda N: "N%d" % N)
def world(request, orc):
    """Per N: keys from the product's keygen on an engine, N_SEL selectors of known random bits (device handle, torus words and the oracle's
    spectra of them), one plain and one really encrypted table of N_ROWS random rows."""
    N = request.param
    w, rng = selector_world(orc, N, 0x9E7 + N, N + 17, N_SEL, 0x5E1EC8 + N, known=())
    w.rows = {"plain": random_words(rng, (N_ROWS, N)), "encrypted": w.R.encrypt_lut(w.rp, w.key1, random_words(rng, (N_ROWS, N)), seed=0x7AC + N)}
    w.eng = gk.engine(w.R, w.rp, w.bk, w.ksk)
    w.sel = w.eng.selectors(w.sel_t)
    w.lut = {"plain": w.eng.lut(w.rows["plain"]), "encrypted": w.eng.lut_encrypted(w.rows["encrypted"])}
    w.oracle_memo = {}
    yield w
    for h in (w.sel, w.lut["plain"], w.lut["encrypted"]):
        h.close()
    w.eng.close()


def _oracle(orc, w, kind, sel_idx, row0, coefs=None, sel_f=None, tag=None):
    """the oracle's mixed netlist of every replica: sel_idx [count][5], row0 [count]; computed once per world and arguments, shared by the tests
    that ask for the same replicas, and read-only"""
    def compute():
        net = mixed_netlist(w.R, w.N, coefs)
        rows = as_trlwe(w.rows[kind], w.N)
        return np.stack([oracle_cmux_net(orc, w.P, w.plan, w.sel_f if sel_f is None else sel_f, sel_idx[g], rows[row0[g]:], net, w.ksk)
                         for g in range(len(row0))])
    return gk.memo(w.oracle_memo, (kind, sel_idx, row0, coefs, tag), compute)


def _replicas(count):
    """(sel_idx, row0, and what they mean to the oracle) twice: seven selectors shared between the replicas with row0 non-zero and differing per
    replica; then d_sel_idx = NULL and d_row0 = NULL"""
    rng = np.random.default_rng(1000 + count)
    shared = rng.integers(0, 7, (count, N_VARS)).astype(np.int32)
    rows0 = rng.integers(1, N_ROWS - 8 + 1, count).astype(np.int32)
    if count > 1:
        rows0[0], rows0[1] = 1, N_ROWS - 8                                     # they differ, and one replica ends on the table's last row
    default_idx = np.arange(count * N_VARS, dtype=np.int32).reshape(count, N_VARS)
    return (shared, rows0, shared, rows0), (None, None, default_idx, np.zeros(count, np.int32))


@pytest.mark.parametrize("count", [1, 5, 37])
def test_every_word_equals_the_oracle_net(orc, world, count):
    """TRLWE form, plain and really encrypted tables; selectors shared between replicas with row0 non-zero and differing, then d_sel_idx and
    d_row0 NULL.  37 replicas are 148, 111, 111 and 37 waves at the four levels: several workgroups, the last one never full."""
    w = world
    net = mixed_netlist(w.R, w.N)
    for kind in ("plain", "encrypted"):
        for sel_idx, row0, exp_idx, exp_row0 in _replicas(count):
            want = _oracle(orc, w, kind, exp_idx, exp_row0)
            got = net_run(w, net, w.lut[kind], count, sel_idx, row0)
            assert got.shape == (count, 3, 2, w.N)
            assert np.array_equal(got, want), (kind, sel_idx is None, np.argwhere((got != want).any(axis=(2, 3)))[:8])


def test_extract_form_equals_the_oracle(orc, world, monkeypatch):
    """identity_key_switch(sample_extract_index(node, coef)) at coef 0, 1 and N - 1 of the three outputs, on the batch key switch and, under
    RTFHE_KS_MM_MIN=0, on the wave-per-sample one."""
    w = world
    coefs = (0, 1, w.N - 1)
    net = mixed_netlist(w.R, w.N, coefs)
    count = 5
    (sel_idx, row0, _, _), _ = _replicas(count)
    plain_route = gk.engine(w.R, w.rp, w.bk, w.ksk, monkeypatch, {"RTFHE_KS_MM_MIN": "0"})
    try:
        for kind in ("plain", "encrypted"):
            want = _oracle(orc, w, kind, sel_idx, row0, coefs)
            got = net_run(w, net, w.lut[kind], count, sel_idx, row0)
            assert got.shape == (count, 3, w.rp.n + 1) and np.array_equal(got, want), kind
            with plain_route.selectors(w.sel_t[:7]) as sel, (plain_route.lut(w.rows[kind]) if kind == "plain" else plain_route.lut_encrypted(w.rows[kind])) as lut:
                assert np.array_equal(net_run(w, net, lut, count, sel_idx, row0, on=plain_route, sel=sel), want), kind
    finally:
        plain_route.close()


def test_tree_netlist_equals_the_tree_entry(world):
    """No oracle: cmux_tree_netlist(3) word for word with cmux_tree_batch on the same selectors, rows and row0."""
    w = world
    count = 6
    rng = np.random.default_rng(w.N + 3)
    sel_idx = rng.integers(0, N_SEL, (count, 3)).astype(np.int32)
    row0 = rng.integers(0, N_ROWS - 8 + 1, count).astype(np.int32)
    net = w.R.cmux_tree_netlist(3)
    for kind in ("plain", "encrypted"):
        want = w.eng.cmux_tree_batch(w.sel, w.lut[kind], 3, count, sel_idx, row0)
        assert np.array_equal(net_run(w, net, w.lut[kind], count, sel_idx, row0)[:, 0], want), kind


def test_rotation_netlist_equals_the_rotation_entry(world):
    """No oracle: trgsw_rotate_netlist(5) with explicit exponents word for word with trgsw_rotate_batch; the rows to rotate are the rows of an
    encrypted table, replica g starts from row g."""
    w = world
    count = 6
    rng = np.random.default_rng(w.N + 5)
    sel_idx = rng.integers(0, N_SEL, (count, 5)).astype(np.int32)
    rot = [2 * w.N - 1, 0, w.N, 1, int(rng.integers(0, 2 * w.N))]
    rows = as_trlwe(w.rows["encrypted"], w.N)[:count]
    want = w.eng.trgsw_rotate_batch(w.sel, rows, 5, sel_idx, rot)
    got = net_run(w, w.R.trgsw_rotate_netlist(5, rot), w.lut["encrypted"], count, sel_idx, np.arange(count, dtype=np.int32))
    assert np.array_equal(got[:, 0], want)
    # rot None is X^-2^k, the entry's default
    want = w.eng.trgsw_rotate_batch(w.sel, rows, 5, sel_idx)
    got = net_run(w, w.R.trgsw_rotate_netlist(5), w.lut["encrypted"], count, sel_idx, np.arange(count, dtype=np.int32))
    assert np.array_equal(got[:, 0], want)


def test_replay_update_and_a_destroyed_set(orc, world):
    """Two replays give equal outputs, also on a second stream; after Selectors.update with new bits a replay equals the oracle on the new
    selectors, and the updated set computes what a fresh set of the same words computes; destroying the set makes launch fail."""
    import torch
    w, R = world, world.R
    count = 5
    net = mixed_netlist(R, w.N)
    (sel_idx, row0, _, _), _ = _replicas(count)
    want = _oracle(orc, w, "encrypted", sel_idx, row0)
    d_out = torch.zeros((count, 3, 2, w.N), dtype=torch.int32, device="cuda")
    words = lambda: d_out.cpu().numpy().view(np.uint32)  # noqa: E731
    st = torch.cuda.current_stream().cuda_stream
    sel = w.eng.selectors(w.sel_t[:7])
    c = w.eng.cmux_circuit(net, sel, w.lut["encrypted"], d_out, count, gk.to_device(sel_idx), gk.to_device(row0))
    try:
        c.launch(st)
        w.eng.sync(st)
        assert np.array_equal(words(), want)
        d_out.zero_()
        c.launch(st)
        w.eng.sync(st)
        assert np.array_equal(words(), want)
        torch.cuda.synchronize()
        s2 = torch.cuda.Stream()
        d_out.zero_()
        torch.cuda.synchronize()
        c.launch(s2.cuda_stream)
        w.eng.sync(s2.cuda_stream)
        assert np.array_equal(words(), want)
        # new ciphertexts of new bits in selectors 2 .. 6: the recorded circuit runs on them
        new_t = np.array(w.sel_t[:7])
        new_t[2:7] = R.encrypt_selectors(w.rp, w.key1, 1 - w.bits[2:7], seed=0xF5E5 + w.N)
        sel.update(new_t[2:7], first=2)
        d_out.zero_()
        c.launch(st)
        w.eng.sync(st)
        want2 = _oracle(orc, w, "encrypted", sel_idx, row0, sel_f=bk_fft(orc, w.P, w.plan, new_t.reshape(-1)), tag="updated")
        assert not np.array_equal(want2, want) and np.array_equal(words(), want2)
        tree_idx = np.array([[0, 2, 6], [5, 3, 1], [4, 4, 2]], np.int32)
        with w.eng.selectors(new_t) as fresh:
            assert np.array_equal(w.eng.cmux_tree_batch(sel, w.lut["plain"], 3, 3, tree_idx), w.eng.cmux_tree_batch(fresh, w.lut["plain"], 3, 3, tree_idx))
        for bad in (lambda: sel.update(new_t[:2], first=6), lambda: sel.update(new_t[:1], first=-1)):
            with pytest.raises(R.RtfheError) as ei:
                bad()
            assert ei.value.code == R._ffi.ERR_INVALID and "outside the set" in str(ei.value)
        before = words()
        sel.close()
        with pytest.raises(R.RtfheError) as ei:
            c.launch(st)
        assert ei.value.code == R._ffi.ERR_STATE and "destroyed" in str(ei.value)
        w.eng.sync(st)
        assert np.array_equal(words(), before)
    finally:
        c.close()
        sel.close()


def test_skipped_replicas(orc, world):
    """One bad selector index and one bad row0 among 7 replicas: rtfhe_sync fails once, the good replicas equal the oracle, the bad replicas'
    TRLWE rows and guard rows around d_out keep a sentinel; in the extract form the bad replicas' rows are all zero."""
    import torch
    w, R = world, world.R
    count = 7
    (sel_idx, row0, _, _), _ = _replicas(count)
    bad_sel, bad_row = sel_idx.copy(), row0.copy()
    bad_sel[2, 4] = 7                                    # the set below has selectors 0 .. 6
    bad_row[5] = N_ROWS - 7                              # its row 7 is one past the table
    keep = np.ones(count, bool)
    keep[[2, 5]] = False
    st = torch.cuda.current_stream().cuda_stream
    sentinel = np.int32(SENTINEL)
    with w.eng.selectors(w.sel_t[:7]) as sel:
        for coefs in (None, (0, 1, w.N - 1)):
            net = mixed_netlist(R, w.N, coefs)
            want = _oracle(orc, w, "encrypted", sel_idx, row0, coefs)
            guarded = torch.full((count + 2,) + want.shape[1:], int(sentinel), dtype=torch.int32, device="cuda")
            with w.eng.cmux_circuit(net, sel, w.lut["encrypted"], guarded[1:], count, gk.to_device(bad_sel), gk.to_device(bad_row)) as c:
                c.launch(st)
                with pytest.raises(R.RtfheError) as ei:
                    w.eng.sync(st)
                assert ei.value.code == R._ffi.ERR_INVALID
                w.eng.sync(st)                           # reported once
            got = guarded.cpu().numpy()
            assert (got[0] == sentinel).all() and (got[-1] == sentinel).all(), "guard rows"
            got = got[1:-1]
            assert np.array_equal(got.view(np.uint32)[keep], want[keep])
            if coefs is None:
                assert (got[~keep] == sentinel).all()
            else:
                assert not got[~keep].any()


def test_comparator_means_less_than(world):
    """A 4-bit a < b over all 256 pairs as replicas: 128 selectors (every value of a and of b, bit by bit), the diagram under the interleaved
    order, terminals +-1/8 at coefficient 0, extract form.  decrypt_bits equals a < b, and gate_batch(NAND, y, y) decrypts to its negation."""
    w, R = world, world.R
    vals = np.arange(16)
    bits = np.array([[(v >> i) & 1 for i in range(4)] for v in vals], np.uint8)                  # [value][bit]
    sel_t = R.encrypt_selectors(w.rp, w.key1, np.concatenate([bits.reshape(-1), bits.reshape(-1)]), seed=0xC0FFEE + w.N)
    a, b = np.repeat(vals, 16), np.tile(vals, 16)
    sel_idx = np.concatenate([a[:, None] * 4 + np.arange(4), 64 + b[:, None] * 4 + np.arange(4)], axis=1).astype(np.int32)
    net = comparator_netlist(4)
    assert net.n_nodes <= 12
    out = R.CmuxNetlist(8)
    for var, hi, lo, rot in net.nodes:
        out.node(var, hi, lo, rot)
    out.output(net.outputs[0][0], coef=0)
    rows = np.zeros((2, w.N), np.uint32)
    rows[0, 0], rows[1, 0] = 0x20000000, 0xE0000000
    with w.eng.selectors(sel_t) as sel, w.eng.lut(rows) as lut:
        y = net_run(w, out, lut, 256, sel_idx, sel=sel)[:, 0]
    assert np.array_equal(R.decrypt_bits(w.rp, w.key0, y).astype(bool), a < b)
    assert np.array_equal(R.decrypt_bits(w.rp, w.key0, w.eng.gate_batch(R.NAND, y, y)).astype(bool), ~(a < b))


def test_refusals(world):
    """The description is checked before anything is allocated or launched, and the message names the node or output; the exact backends refuse."""
    import torch
    w, R = world, world.R
    N = w.N
    d_out = torch.zeros((38, 3, 2, N), dtype=torch.int32, device="cuda")
    lut = w.lut["plain"]

    def net(edit=None, coefs=None):
        n = mixed_netlist(R, N, coefs)
        if edit:
            edit(n)
        return n

    def set_node(i, **kw):
        def edit(n):
            var, hi, lo, rot = n.nodes[i]
            n.nodes[i] = (kw.get("var", var), kw.get("hi", hi), kw.get("lo", lo), kw.get("rot", rot))
        return edit

    def set_out(o, ref=None, coef=None):
        def edit(n):
            r, c = n.outputs[o]
            n.outputs[o] = (r if ref is None else ref, c if coef is None else coef)
        return edit

    w.eng.timer_begin()
    for n, count, names in ((net(set_node(4, hi=7)), 5, "node 4: hi = 7"),                          # a forward reference
                            (net(set_node(4, lo=4)), 5, "node 4: lo = 4"),
                            (net(set_node(8, hi=-1 - N_ROWS)), 5, "node 8: hi = %d is table row %d" % (-1 - N_ROWS, N_ROWS)),
                            (net(set_node(10, lo=11)), 5, "node 10: lo = 11"),                      # past the nodes
                            (net(set_node(2, rot=2 * N)), 5, "node 2: rot = %d" % (2 * N)),
                            (net(set_node(6, var=5)), 5, "node 6: var = 5"),
                            (net(set_out(1, ref=-3)), 5, "output 1: out_ref = -3 names a table row"),
                            (net(set_out(1, ref=11)), 5, "output 1: out_ref = 11"),
                            (net(set_out(2, coef=N), coefs=(0, 1, 2)), 5, "output 2: out_coef = %d" % N),
                            (net(), 38, "sel_idx NULL: replica 37")):                               # 190 selectors of 185
        with pytest.raises(R.RtfheError) as ei:
            w.eng.cmux_circuit(n, w.sel, lut, d_out, count)
        assert ei.value.code == R._ffi.ERR_INVALID and names in str(ei.value), str(ei.value)
    with pytest.raises(R.RtfheError) as ei:
        w.eng.cmux_circuit(net(), w.sel, lut, d_out, 0)
    assert ei.value.code == R._ffi.ERR_INVALID and "at least 1" in str(ei.value)
    assert w.eng.timer_end()[1] == 0, "the checks come before any launch"
    ref = net_run(w, net(), lut, 5)
    try:
        for b in (R._ffi.BACKEND_NTT_EXACT, R._ffi.BACKEND_FFT_SPLIT_EXACT):
            w.eng.set_backend(b)
            with pytest.raises(R.RtfheError) as ei:
                w.eng.cmux_circuit(net(), w.sel, lut, d_out, 5)
            assert ei.value.code == R._ffi.ERR_INVALID and "mirror" in str(ei.value)
    finally:
        w.eng.set_backend(R._ffi.BACKEND_FFT64_MIRROR)
    assert np.array_equal(net_run(w, net(), lut, 5), ref)
    # no key-switching key: the TRLWE form runs (a netlist needs no key of the context), the extract form is refused
    bare = R.Engine(R.Params(n=w.rp.n, N=N), 0)
    try:
        with bare.selectors(w.sel_t[:25]) as sel, bare.lut(w.rows["plain"]) as blut:
            assert np.array_equal(net_run(w, net(), blut, 5, on=bare, sel=sel), ref)
            with pytest.raises(R.RtfheError) as ei:
                bare.cmux_circuit(net(coefs=(0, 1, 2)), sel, blut, d_out, 5)
            assert ei.value.code == R._ffi.ERR_STATE and "key-switching key" in str(ei.value)
    finally:
        bare.close()
