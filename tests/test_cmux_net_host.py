"""CPU: CMUX netlists (include/rtfhe.h, rtfhe_cmux_circuit_create; rustfhe_amd/cmux_net.py) without a GPU -- the netlist restated with the
oracle's own building blocks (tests/leveled_oracle.py: oracle_cmux_net, which tests/test_gpu_cmux_net.py compares the device's words with), what it means with keys
and selectors the product generated, the builders' structure, and the entry points' argument checks."""
import ctypes as C

import numpy as np
import pytest

import orc as _orc_mod  # noqa: F401  (conftest puts tests/ on the path)
from kit import torus_dist
from leveled_oracle import as_trlwe, comparator_netlist, oracle_cmux_net, three_of_five
from pbs_oracle import bk_fft

@pytest.mark.parametrize("N", [1024, 2048])
def test_oracle_net_means_its_function(orc, N, capsys):
    """Keys from the product's keygen (n = 8), selectors from encrypt_selectors, the reduced diagram of a 3-output function of 5 variables over
    two rows of N random 2-bit messages -- plain rows and TRLWE encryptions of them: for all 32 inputs the oracle net's phase decodes to
    evaluate_plain at every coefficient of every output, and stays within levels * 2e-3 * N / 1024 of it, the bound the tree's host test
    asserts per level (one CMUX per level lies on any path to an output)."""
    import rustfhe_amd as R
    rp = R.Params(n=8, N=N)
    _, key1, _, _ = R.keygen(rp, 0xBDD + N, want_bk=False, want_ksk=False)
    p = orc.Params(n=8, N=N)
    plan = orc.Plan(N)
    rng = np.random.default_rng(N + 13)
    net = R.bdd_netlist(5, three_of_five)
    levels = len(net.levels())
    msgs = rng.integers(0, 4, (2, N))
    plain = R.encode_msgs(msgs, 2)
    worst = {}
    for kind, rows in (("plain", as_trlwe(plain, N)), ("encrypted", R.encrypt_lut(rp, key1, plain, seed=0xE5))):
        for x in range(32):
            bits = [(x >> v) & 1 for v in range(5)]
            sel = R.encrypt_selectors(rp, key1, bits, seed=0x5E1 + x)
            got = oracle_cmux_net(orc, p, plan, bk_fft(orc, p, plan, sel.reshape(-1)), range(5), rows, net)
            want = net.evaluate_plain(bits, plain)
            for o, f in enumerate(three_of_five(bits)):
                assert np.array_equal(want[o], plain[0 if f else 1]), (x, o)
            ph = R.trlwe_phase(rp, key1, got)
            assert np.array_equal(R.decode_msgs(ph, 2), R.decode_msgs(want, 2)), (kind, x)
            worst[kind] = max(worst.get(kind, 0.0), float(torus_dist(ph, want).max()))
    with capsys.disabled():
        print("\noracle CMUX net, N = %d, %d nodes on %d levels: largest torus distance from evaluate_plain %s"
              % (N, net.n_nodes, levels, {k: round(v, 5) for k, v in worst.items()}))
    for kind, w in worst.items():
        assert w < levels * 2e-3 * N / 1024, (kind, w)


def test_levels_of_a_shared_node_and_outputs_at_different_levels():
    import rustfhe_amd as R
    net = R.CmuxNetlist(3)
    a = net.node(0, net.row(1), net.row(0))            # level 0, used by b and c
    b = net.node(1, a, net.row(2))                     # level 1
    c = net.node(2, a, a, rot=5)                       # level 1
    d = net.node(0, net.row(3), net.row(2), rot=1)     # level 0, added late
    e = net.node(1, b, d)                              # level 2
    f = net.node(2, e, c)                              # level 3
    net.output(a)
    net.output(c)
    net.output(f)
    assert net.levels() == [[a, d], [b, c], [e], [f]]
    arr = net.arrays()
    assert arr["n_nodes"] == 6 and arr["n_out"] == 3 and arr["out_coef"] is None
    assert arr["hi"].tolist() == [-2, 0, 0, -4, 1, 4] and arr["lo"].tolist() == [-1, -3, 0, -3, 3, 2] and arr["rot"].tolist() == [0, 0, 5, 1, 0, 0]
    # the clear meaning: rows of 4 coefficients, row k = (k + 1, 0, 0, 0)
    rows = np.zeros((4, 4), np.uint32)
    rows[:, 0] = np.arange(1, 5)
    out = net.evaluate_plain([1, 0, 1], rows)
    assert out[0].tolist() == [2, 0, 0, 0]                                    # a = row 1
    assert out[1].tolist() == [0, (-2) & 0xFFFFFFFF, 0, 0]                    # c = X^5 * a = -X * a in Z[X]/(X^4 + 1)
    assert out[2].tolist() == [0, 4, 0, 0]                                    # f = e = d = X * row 3


def test_bdd_equals_its_function_on_every_input():
    """6 variables, 3 outputs, under the natural and under a shuffled order, from a callable and from its truth tables."""
    import rustfhe_amd as R
    f = lambda b: (b[0] ^ b[3] ^ b[5], int(sum(b) in (2, 3)), (b[1] & b[2]) | (b[4] & ~b[0] & 1))  # noqa: E731
    rows = np.zeros((2, 4), np.uint32)
    rows[0, 0] = 1                                                            # true_row 0 = 1, false_row 1 = 0
    tables = np.array([f(tuple((x >> v) & 1 for v in range(6))) for x in range(64)]).T
    for fn, order in ((f, None), (f, [4, 0, 5, 2, 1, 3]), (tables, [5, 4, 3, 2, 1, 0])):
        net = R.bdd_netlist(6, fn, order)
        assert len(net.outputs) == 3 and net.n_nodes <= 3 * 63
        seen = set()
        for i, (_, hi, lo, _) in enumerate(net.nodes):
            assert hi != lo and hi < i and lo < i, "reduced, and in topological order"
            seen.add(net.nodes[i])
        assert len(seen) == net.n_nodes, "no duplicate nodes"
        for x in range(64):
            bits = tuple((x >> v) & 1 for v in range(6))
            assert net.evaluate_plain(bits, rows)[:, 0].tolist() == list(f(bits)), (order, x)


def test_comparator_under_the_interleaved_order_is_small():
    net = comparator_netlist(8)
    assert net.n_nodes <= 24 and len(net.levels()) == 16, (net.n_nodes, len(net.levels()))
    rows = np.zeros((2, 4), np.uint32)
    rows[0, 0] = 1
    rng = np.random.default_rng(8)
    for a_, b_ in [(0, 0), (255, 255), (0, 255), (255, 0), (127, 128), (128, 127)] + [tuple(rng.integers(0, 256, 2)) for _ in range(50)]:
        bits = [(int(a_) >> i) & 1 for i in range(8)] + [(int(b_) >> i) & 1 for i in range(8)]
        assert net.evaluate_plain(bits, rows)[0, 0] == int(a_ < b_), (a_, b_)


def test_tree_and_rotation_builders_follow_their_headers():
    import rustfhe_amd as R
    tree = R.cmux_tree_netlist(3)
    assert tree.n_nodes == 7 and tree.levels() == [[0, 1, 2, 3], [4, 5], [6]] and tree.outputs == [(6, None)]
    # level k, node j: cmux(S_k, r_{2j+1}, r_{2j}); level 0 reads table rows 2j + 1 and 2j
    assert tree.nodes == [(0, -2, -1, 0), (0, -4, -3, 0), (0, -6, -5, 0), (0, -8, -7, 0), (1, 1, 0, 0), (1, 3, 2, 0), (2, 5, 4, 0)]
    rot = R.trgsw_rotate_netlist(5)
    assert rot.n_nodes == 5 and rot.levels() == [[0], [1], [2], [3], [4]] and rot.outputs == [(4, None)]
    for N in (1024, 2048):
        a = rot.arrays(N)
        # step k: cmux(S_k, X^rot[k] * acc, acc) with rot NULL = 2N - 2^k; step 0 on table row 0
        assert a["var"].tolist() == [0, 1, 2, 3, 4] and a["hi"].tolist() == [-1, 0, 1, 2, 3] and a["lo"].tolist() == a["hi"].tolist()
        assert a["rot"].tolist() == [2 * N - (1 << k) for k in range(5)]
    assert R.trgsw_rotate_netlist(3, [7, 0, 2047]).arrays()["rot"].tolist() == [7, 0, 2047]
    # its clear meaning: the address bits rotate row 0 by X^-addr
    row = np.arange(1, 9, dtype=np.uint32)[None]
    out = R.trgsw_rotate_netlist(3).evaluate_plain([1, 0, 1], row)[0]
    assert out.tolist() == [6, 7, 8] + [(-v) & 0xFFFFFFFF for v in (1, 2, 3, 4, 5)]


def test_construction_refusals():
    import rustfhe_amd as R
    net = R.CmuxNetlist(2)
    for bad in (lambda: R.CmuxNetlist(0), lambda: net.node(2, net.row(0), net.row(1)), lambda: net.node(-1, net.row(0), net.row(1)),
                lambda: net.node(0, 0, net.row(0)), lambda: net.row(-1), lambda: net.output(net.row(0)), lambda: net.output(0), lambda: net.arrays(),
                lambda: R.cmux_tree_netlist(0), lambda: R.trgsw_rotate_netlist(3, [1, 2]), lambda: R.bdd_netlist(17, lambda b: b[0]),
                lambda: R.bdd_netlist(2, lambda b: 1), lambda: R.bdd_netlist(2, lambda b: (b[0], 0)), lambda: R.bdd_netlist(2, lambda b: b[0], [0, 0]),
                lambda: R.bdd_netlist(2, [[0, 1, 1]])):
        with pytest.raises(ValueError):
            bad()
    n0 = net.node(0, net.row(0), net.row(1), rot=-1)
    with pytest.raises(ValueError):
        net.node(1, n0 + 1, n0)                                   # a forward reference
    net.output(n0, coef=3)
    with pytest.raises(ValueError):
        net.output(n0)                                            # one form per netlist
    with pytest.raises(ValueError):
        net.arrays()                                              # a negative exponent needs N
    assert net.arrays(1024)["rot"].tolist() == [2047] and net.arrays(1024)["out_coef"].tolist() == [3]


def test_entries_reject_null_handles():
    """The device entry points: a null context or handle (there is none without a GPU) is refused before anything else is looked at."""
    import rustfhe_amd as R
    L = R.load()
    INV = R._ffi.ERR_INVALID
    one = np.zeros(1, np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    h = C.c_void_p()
    assert L.rtfhe_cmux_circuit_create(None, None, None, ptr(one), ptr(one), ptr(one), None, 1, 1, ptr(one), None, 1, None, None, None, 1, C.byref(h)) == INV
    assert not h.value and b"null context" in L.rtfhe_last_error(None)
    assert L.rtfhe_trgsw_update(None, ptr(one), 0, 1) == INV
    assert b"null selector set" in L.rtfhe_last_error(None)
