"""CPU: LUT circuits (rustfhe_amd.lut_circuit) without a GPU -- the plain evaluator, the split of levels into waves of one n_out, and the arrays
handed to rtfhe_lut_circuit_create."""
import numpy as np
import pytest

from rustfhe_amd.lut_circuit import LutNetlist, lut_ripple_adder


def test_adder_plain_every_pair():
    net = lut_ripple_adder(8)
    assert net.num_inputs == 16 and len(net.nodes) == 8 and len(net.outputs) == 9
    for a in range(256):
        for b in range(256):
            bits = [(a >> i) & 1 for i in range(8)] + [(b >> i) & 1 for i in range(8)]
            out = net.evaluate_plain(bits)
            assert sum(v << i for i, v in enumerate(out)) == a + b, (a, b)


def _mixed_net():
    """Three tables of 1, 2 and 4 functions; two levels, each with nodes of every n_out in creation order 4, 1, 2, 1."""
    net = LutNetlist(2)
    x = net.inputs(3)
    t1 = net.table([lambda s: s])
    t2 = net.table([lambda s: s & 1, lambda s: s >> 1])
    t4 = net.table([lambda s: s, lambda s: 3 - s, lambda s: (s + 1) % 4, lambda s: s >> 1])
    l1 = [net.node([(x[0], 1)], 0, t4), net.node([(x[1], 1)], 0, t1), net.node([(x[0], 1), (x[2], 1)], 0, t2), net.node([(x[2], 1)], 1, t1)]
    l2 = [net.node([(l1[0][1], 1)], 0, t4), net.node([(l1[1][0], 1), (l1[2][0], 1)], 0, t1), net.node([(l1[3][0], -1)], 3, t2),
          net.node([(l1[2][1], 2), (l1[0][3], 1)], 0, t1)]
    for w in l2:
        for o in w:
            net.output(o)
    return net


def test_waves_split_levels_by_n_out_and_respect_dependencies():
    net = _mixed_net()
    assert net.levels() == [[0, 1, 2, 3], [4, 5, 6, 7]]
    assert net.waves() == [(1, [1, 3]), (2, [2]), (4, [0]), (1, [5, 7]), (2, [6]), (4, [4])]
    done = set(range(net.num_inputs))
    for th, nodes in net.waves():
        made = set()
        for g in nodes:
            terms, _, table, first = net.nodes[g]
            assert net.n_out(g) == th
            assert all(w in done for w, _ in terms), "a node reads a wire that no earlier wave wrote"
            made |= set(range(first, first + th))
        done |= made
    assert done == set(range(net.num_wires))
    d = net.arrays(1)
    assert list(d["wave_n_out"]) == [1, 2, 4, 1, 2, 4] and list(d["wave_offsets"]) == [0, 2, 3, 4, 6, 7, 8]
    assert d["out_idx"].size == sum(net.n_out(g) for g in range(len(net.nodes)))
    assert net.evaluate_plain([1, 2, 0]) == [2, 1, 3, 1, 3, 0, 1, 0]


def test_arrays_offset_every_replica_by_its_wire_block():
    net = _mixed_net()
    W = net.num_wires
    one, R = net.arrays(1), 3
    many = net.arrays(R)
    assert many["num_wires"] == R * W and many["fan_in"] == one["fan_in"] == 2
    assert list(many["wave_offsets"]) == [R * o for o in one["wave_offsets"]]
    assert list(many["wave_n_out"]) == list(one["wave_n_out"])
    obase = np.concatenate([[0], np.cumsum(np.diff(one["wave_offsets"]) * one["wave_n_out"])])
    for w in range(len(one["wave_n_out"])):
        lo, hi, th = one["wave_offsets"][w], one["wave_offsets"][w + 1], one["wave_n_out"][w]
        for r in range(R):
            sl = slice(R * lo + r * (hi - lo), R * lo + (r + 1) * (hi - lo))
            base = one["in_idx"][lo:hi]
            assert np.array_equal(many["in_idx"][sl], np.where(base >= 0, base + r * W, -1))
            assert np.array_equal(many["weights"][sl], one["weights"][lo:hi])
            assert np.array_equal(many["cst"][sl], one["cst"][lo:hi])
            assert np.array_equal(many["lut_idx"][sl], one["lut_idx"][lo:hi])
            n = (hi - lo) * th
            got = many["out_idx"][R * obase[w] + r * n: R * obase[w] + (r + 1) * n]
            assert np.array_equal(got, one["out_idx"][obase[w]:obase[w] + n] + r * W)
    assert set(many["out_idx"].tolist()) == set(range(R * W)) - {r * W + i for r in range(R) for i in range(net.num_inputs)}


def test_constants_are_torus_words_on_b():
    net = LutNetlist(2)
    x = net.input()
    t = net.table([lambda s: s])
    net.node([(x, 1)], 1, t)
    net.node([(x, -1)], 3, t)
    assert list(net.arrays(1)["cst"]) == [1 << 29, 3 << 29]
    net3 = LutNetlist(3)
    y = net3.input()
    net3.node([(y, 1)], -1, net3.table([lambda s: s]))
    assert list(net3.arrays(1)["cst"]) == [(-(1 << 28)) & 0xFFFFFFFF]


def test_evaluate_plain_rejects_a_sum_outside_the_message_space():
    net = LutNetlist(1)
    a, b = net.inputs(2)
    t = net.table([lambda s: s])
    (o,) = net.node([(a, 1), (b, 1)], 0, t)
    net.output(o)
    assert net.evaluate_plain([1, 0]) == [1]
    with pytest.raises(ValueError, match="node 0: sum 2"):
        net.evaluate_plain([1, 1])
    neg = LutNetlist(2)
    a = neg.input()
    neg.node([(a, -1)], 0, neg.table([lambda s: s]))
    assert neg.evaluate_plain([0]) == []
    with pytest.raises(ValueError, match="sum -1"):
        neg.evaluate_plain([1])
    with pytest.raises(ValueError, match="node 0: sum 4"):
        lut_ripple_adder(2).evaluate_plain([3, 0, 1, 0])


def test_construction_checks():
    net = LutNetlist(2)
    a = net.input()
    with pytest.raises(ValueError):
        net.table([lambda s: s] * 3)
    t = net.table([lambda s: s])
    with pytest.raises(ValueError):
        net.node([(a, 1)], 0, 1)
    with pytest.raises(ValueError):
        net.node([(5, 1)], 0, t)
    with pytest.raises(ValueError):
        net.node([(a, 1)] * 9, 0, t)
