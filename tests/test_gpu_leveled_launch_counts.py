"""GPU: how many kernels the leveled and the pack entry points and the replay of a recorded circuit enqueue, counted with the counter
rtfhe_timer_end returns (a circuit of any kind: the launches its recording counted, which every replay adds to that counter; the recording itself
and a refused one add nothing).  The expected counts restate the host code of rtfhe_cmux_tree.hip, rtfhe_cmux_net.hip, rtfhe_pack.hip,
rtfhe_circuit.hip, rtfhe_batch.hip and rtfhe_stages.hip:

  tree, depth d                  d           one k_cmux_tree per level
  tree with extraction           d + 1       ... and the batch key switch: 1 with the matrix key (k_key_switch_mm) and without (RTFHE_KS_MM_MIN=0,
                                             k_key_switch_ext)
  demultiplexer, depth d         d           one k_demux_tree per level
  rotation                       1           all steps of all lookups in one k_trgsw_rotate
  rotation with extraction       3           the rotation, the key switch, k_rows_restore
  Lut.accumulate_dev             1           k_trlwe_accumulate
  netlist of L levels            L + 2       k_cmux_net_check, one k_cmux_net per level, k_cmux_net_out; + 1 key switch in the extract form
  pack of P positions            1 + ceil(P / 512)      k_pack_ks_mm, then k_pack_combine per PACK_POS_MAX = 512 positions
  external_product_batch         0           a stage-level call: launched, not counted
  gate circuit of W waves        2 W         per wave (at most one gate per CU: one rung of the ladder) the bootstrap launch and the batch key
                                             switch of the split path (k_key_switch_mm); W without the matrix key: one fused launch per wave
  LUT circuit of W waves         4 W         per wave k_lut_gather, the many-LUT launch, the key switch of its count * n_out rows (k_key_switch_mm,
                                             or k_key_switch_ext without the matrix key) and k_lut_scatter

Both rings at the small mask lengths of the other leveled tests (n = 40 at N = 1024, n = 24 at N = 2048); 5 and 9 lookups, so that the last
workgroup of four waves holds one wave; depths 1, 2, 3; the tree and the rotation in both leveled modes.  The extract forms' words are compared
between the two key-switch routes on the way: both are exact.  The two circuits have three waves of 1, 2 and 5 nodes, one replica, the LUT circuit's
second wave with two outputs per node."""
import types

import numpy as np
import pytest

import gpu_kit as gk
from kit import SMALL_N, random_words

pytestmark = pytest.mark.gpu

COUNTS = (5, 9)
DEPTHS = (1, 2, 3)
N_SEL = 9 * 3            # sel_idx = NULL at depth 3 and 9 lookups reads selectors 0 .. 26
N_ROWS = 8               # a depth-3 tree
PACK_POS_MAX = 512       # rtfhe_kernels_pack.hpp


@pytest.fixture(scope="module", params=[1024, 2048], ids=lambda N: "N%d" % N)
def world(request):
    """Per N: an engine with the matrix form of the key-switching key and one without, each with the same selectors and encrypted table, a
    packing key of random words and 9 input rows.  Nothing is decrypted here: tables, rows and the packing key are random words."""
    import rustfhe_amd as R
    N = request.param
    rp = R.Params(n=SMALL_N[N], N=N)
    key0, key1, bk, ksk = R.keygen(rp, 0x1C0 + N)
    rng = np.random.default_rng(N + 19)
    w = types.SimpleNamespace(R=R, N=N, rp=rp)
    sel_t = R.encrypt_selectors(rp, key1, rng.integers(0, 2, N_SEL).astype(np.uint8), seed=0x1C1 + N)
    table = random_words(rng, (N_ROWS, 2, N))
    w.rows = random_words(rng, (max(COUNTS), 2, N))
    w.pk = random_words(rng, (rp.n, 8, 3, 2, N))
    mp = pytest.MonkeyPatch()
    w.mm = gk.engine(R, rp, bk, ksk)
    w.ext = gk.engine(R, rp, bk, ksk, mp, {"RTFHE_KS_MM_MIN": "0"})
    w.on = {}
    for e in (w.mm, w.ext):
        w.on[e] = (e.selectors(sel_t), e.lut_encrypted(table))
    w.key = w.mm.packing_key(w.pk)
    yield w
    w.key.close()
    for e in (w.mm, w.ext):
        for h in w.on[e]:
            h.close()
        e.close()
    mp.undo()


def _counted(e, fn, stream=None):
    e.timer_begin(stream)
    out = fn()
    return e.timer_end(stream)[1], out


def _mode(w, rounded):
    return w.R._ffi.DECOMP_ROUNDED if rounded else w.R._ffi.DECOMP_REFERENCE


@pytest.mark.parametrize("rounded", [False, True], ids=["reference", "rounded"])
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("depth", DEPTHS)
def test_tree_and_rotation(world, depth, count, rounded):
    w = world
    tag = "N = %d %s depth %d count %d" % (w.N, "rounded" if rounded else "reference", depth, count)
    words = {}
    for name, e in (("mm", w.mm), ("ext", w.ext)):
        sel, lut = w.on[e]
        e.set_leveled_decomposition(_mode(w, rounded))
        try:
            k_tree, _ = _counted(e, lambda: e.cmux_tree_batch(sel, lut, depth, count))
            k_tree_x, tree_x = _counted(e, lambda: e.cmux_tree_extract_batch(sel, lut, depth, count))
            k_rot, _ = _counted(e, lambda: e.trgsw_rotate_batch(sel, w.rows[:count], depth))
            k_rot_x, rot_x = _counted(e, lambda: e.trgsw_rotate_extract_batch(sel, w.rows[:count], depth))
        finally:
            e.set_leveled_decomposition(_mode(w, False))
        print("%s, key switch %s: tree %d, tree with extraction %d, rotation %d, rotation with extraction %d launches" % (tag, name, k_tree, k_tree_x, k_rot, k_rot_x))
        assert (k_tree, k_tree_x, k_rot, k_rot_x) == (depth, depth + 1, 1, 3), (tag, name)
        words[name] = (tree_x, rot_x)
    assert np.array_equal(words["mm"][0], words["ext"][0]) and np.array_equal(words["mm"][1], words["ext"][1]), tag


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("depth", DEPTHS)
def test_demultiplexer_and_accumulate(world, depth, count):
    import torch
    w, e = world, world.mm
    sel, _ = w.on[e]
    k, leaves = _counted(e, lambda: e.demux_tree_batch(sel, w.rows[:count], depth))
    print("N = %d depth %d count %d: demultiplexer %d launches" % (w.N, depth, count, k))
    assert k == depth and leaves.shape == (count, 1 << depth, 2, w.N)
    st = torch.cuda.current_stream().cuda_stream
    d_leaves = torch.from_numpy(leaves.view(np.int32)).cuda()
    with e.lut_encrypted(np.zeros((1 << depth, 2, w.N), np.uint32)) as acc:      # (a table of its own: the world's is shared and read-only)
        k, _ = _counted(e, lambda: acc.accumulate_dev(d_leaves, 0, 1 << depth, count, st), st)
        e.sync(st)
    print("N = %d depth %d count %d: accumulate %d launches" % (w.N, depth, count, k))
    assert k == 1


@pytest.mark.parametrize("extract", [False, True], ids=["trlwe", "extract"])
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("depth", DEPTHS)
def test_netlist(world, depth, count, extract):
    """cmux_tree_netlist(depth) has `depth` levels; the extract form names its output's coefficient 1"""
    import torch
    w = world
    net = w.R.cmux_tree_netlist(depth)
    if extract:
        (ref, _), = net.outputs
        net.outputs = []
        net.output(ref, 1)
    assert len(net.levels()) == depth
    st = torch.cuda.current_stream().cuda_stream
    words = {}
    for name, e in (("mm", w.mm), ("ext", w.ext)):
        sel, lut = w.on[e]
        d_out = torch.zeros((count, 1, w.rp.n + 1) if extract else (count, 1, 2, w.N), dtype=torch.int32, device="cuda")
        k_create, c = _counted(e, lambda: e.cmux_circuit(net, sel, lut, d_out, count), st)
        with c:
            k, _ = _counted(e, lambda: c.launch(st), st)
            e.sync(st)
        print("N = %d depth %d count %d %s, key switch %s: netlist %d launches" % (w.N, depth, count, "extract" if extract else "trlwe", name, k))
        assert k_create == 0, "recording counts nothing: a replay does"
        assert k == depth + 2 + (1 if extract else 0), (w.N, depth, count, extract, name)
        words[name] = d_out.cpu().numpy()
    assert np.array_equal(words["mm"], words["ext"])


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("P", [1, 4, PACK_POS_MAX, PACK_POS_MAX + 1, 600])
def test_pack(world, P, count):
    w, e = world, world.mm
    tlwe = random_words(np.random.default_rng(P + count), (count, P, w.rp.n + 1))
    k, out = _counted(e, lambda: e.pack_batch(w.key, tlwe, P))
    print("N = %d P %d count %d: pack %d launches" % (w.N, P, count, k))
    assert k == 1 + (P + PACK_POS_MAX - 1) // PACK_POS_MAX and out.shape == (count, 2, w.N)


@pytest.mark.parametrize("rounded", [False, True], ids=["reference", "rounded"])
@pytest.mark.parametrize("count", COUNTS)
def test_external_product_is_not_counted(world, count, rounded):
    w, e = world, world.mm
    e.set_leveled_decomposition(_mode(w, rounded))
    try:
        k, out = _counted(e, lambda: e.external_product_batch(np.arange(count) % w.rp.n, w.rows[:count]))
    finally:
        e.set_leveled_decomposition(_mode(w, False))
    print("N = %d %s count %d: external product %d launches" % (w.N, "rounded" if rounded else "reference", count, k))
    assert k == 0 and out.any()


# ---- recorded circuits: what a replay adds, twice over, and that neither a recording nor a refused one adds anything ----
WAVES = (1, 2, 5)        # nodes per wave
INPUTS = 8               # wires 0 .. 7 are inputs, every node writes the next free wire(s)


def _refused(R, create, msg):
    with pytest.raises(R.RtfheError) as ei:
        create()
    assert ei.value.code == R._ffi.ERR_INVALID and msg in str(ei.value), str(ei.value)


def _replays(e, handle, st):
    """what one replay adds to the counter, and what two add"""
    one, _ = _counted(e, lambda: e.circuit_launch(handle, st), st)
    two, _ = _counted(e, lambda: (e.circuit_launch(handle, st), e.circuit_launch(handle, st)), st)
    e.sync(st)
    return one, two


def _sources(rng, written):
    """for every node, wave by wave, a wire it may read: an input or one of the wires the earlier waves wrote (written: wires per wave)"""
    before = np.concatenate([[0], np.cumsum(written)])
    return np.concatenate([rng.integers(0, INPUTS + before[v], k) for v, k in enumerate(WAVES)])


def test_gate_circuit(world):
    import torch
    w = world
    rng = np.random.default_rng(w.N + 23)
    nodes, offs = sum(WAVES), np.concatenate([[0], np.cumsum(WAVES)]).astype(np.int32)
    ops = rng.choice([w.R.NAND, w.R.AND, w.R.OR, w.R.XOR], nodes)
    idx0, idx1 = _sources(rng, WAVES), rng.integers(0, INPUTS, nodes)
    idx_out = INPUTS + np.arange(nodes)
    wires0 = random_words(rng, (INPUTS + nodes, w.rp.n + 1))
    st = torch.cuda.current_stream().cuda_stream
    words = {}
    for name, e, per_wave in (("mm", w.mm, 2), ("ext", w.ext, 1)):
        d = [gk.to_device(a) for a in (ops, idx0, idx1, idx_out)]
        d_wires = gk.to_device(wires0, np.uint32)
        k_refused, _ = _counted(e, lambda: (_refused(w.R, lambda: e.circuit_create(*d, np.array([0, 1, 1, 8], np.int32), d_wires, INPUTS + nodes), "wave_offsets"),
                                            _refused(w.R, lambda: e.circuit_create(*d, offs, d_wires, 0), "num_wires")), st)
        k_create, c = _counted(e, lambda: e.circuit_create(*d, offs, d_wires, INPUTS + nodes), st)
        try:
            one, two = _replays(e, c, st)
        finally:
            e.circuit_destroy(c)
        print("N = %d, key switch %s: gate circuit of %d waves: refused %d, recording %d, one replay %d, two replays %d launches" %
              (w.N, name, len(WAVES), k_refused, k_create, one, two))
        assert (k_refused, k_create) == (0, 0), "recording counts nothing: a replay does"
        assert (one, two) == (per_wave * len(WAVES), 2 * per_wave * len(WAVES)), (w.N, name)
        words[name] = gk.words_of(d_wires)
    assert np.array_equal(words["mm"], words["ext"]) and not np.array_equal(words["mm"], wires0)


def test_lut_circuit(world):
    import torch
    from lut_circuit_kit import create
    w = world
    rng = np.random.default_rng(w.N + 29)
    n_out = np.array([1, 2, 1], np.int32)
    nodes, rows = sum(WAVES), int(np.dot(WAVES, n_out))
    in_idx = np.stack([_sources(rng, WAVES * n_out), rng.integers(-1, INPUTS, nodes)], axis=1)      # (-1: an unused slot)
    d = {"fan_in": 2, "in_idx": in_idx.astype(np.int32), "weights": rng.integers(-(1 << 31), 1 << 31, (nodes, 2)).astype(np.int32),
         "cst": random_words(rng, (nodes,)), "lut_idx": rng.integers(0, 2, nodes).astype(np.int32),
         "wave_offsets": np.concatenate([[0], np.cumsum(WAVES)]).astype(np.int32), "wave_n_out": n_out,
         "out_idx": (INPUTS + np.arange(rows)).astype(np.int32), "num_wires": INPUTS + rows}
    wires0 = random_words(rng, (INPUTS + rows, w.rp.n + 1))
    tv = random_words(rng, (2, w.N))
    st = torch.cuda.current_stream().cuda_stream
    words = {}
    for name, e in (("mm", w.mm), ("ext", w.ext)):
        d_wires = gk.to_device(wires0, np.uint32)
        with e.lut(tv) as lut:
            k_refused, _ = _counted(e, lambda: _refused(w.R, lambda: create(e, lut, dict(d, wave_n_out=np.array([1, 3, 1], np.int32)), d_wires), "n_out = 3"), st)
            k_create, c = _counted(e, lambda: create(e, lut, d, d_wires), st)
        try:
            one, two = _replays(e, c, st)
        finally:
            e.circuit_destroy(c)
        print("N = %d, key switch %s: LUT circuit of %d waves: refused %d, recording %d, one replay %d, two replays %d launches" %
              (w.N, name, len(WAVES), k_refused, k_create, one, two))
        assert (k_refused, k_create) == (0, 0), "recording counts nothing: a replay does"
        assert (one, two) == (4 * len(WAVES), 8 * len(WAVES)), (w.N, name)
        words[name] = gk.words_of(d_wires)
    assert np.array_equal(words["mm"], words["ext"]) and not np.array_equal(words["mm"], wires0)
