"""GPU: LUT circuits (rtfhe_lut_circuit_create: k_lut_gather, the many-LUT PBS, k_lut_scatter per wave, one recorded graph).
Gate netlists translated into LUT nodes give CircuitRunner's wire table word for word; random circuits give the host composition (numpy sums +
Engine.pbs_many_batch, wave by wave) word for word; the adder decrypts to a + b; replays, rejects and lifetimes."""
import importlib.util
import os

import numpy as np
import pytest

import gpu_kit as gk
from kit import keys_2048, random_words
from lut_circuit_kit import adder_inputs, create, decode, host_compose, random_circuit, replay

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E8 = 0x20000000
U32 = 0xFFFFFFFF


# ---- gate netlists as LUT circuits -------------------------------------------------------------------------------------------------------
def _gate_arrays(net, replicas):
    """Every gate of a levelised netlist as one n_out = 1 node of the constant 1/8 table, with CircuitRunner's wire numbering and wave order."""
    import rustfhe_amd as R
    lin = {R.NAND: ((-1, -1), E8), R.AND: ((1, 1), -E8), R.OR: ((1, 1), E8), R.XOR: ((2, 2), 2 * E8), R.NOT: ((-1,), 0),
           R.ANDNY: ((-1, 1), -E8), R.COPY: ((1,), 0)}
    W, base = net.num_wires, 2 + net.num_inputs
    in_idx, wts, cst, out_idx, offs = [], [], [], [], [0]
    for wave in net.levels():
        for r in range(replicas):
            for g in wave:
                op, a, b = net.gates[g]
                w, c = lin[op]
                ins = [a, b][:len(w)]
                in_idx.append([r * W + x for x in ins] + [-1] * (2 - len(w)))
                wts.append(list(w) + [0] * (2 - len(w)))
                cst.append(c & U32)
                out_idx.append(r * W + base + g)
        offs.append(offs[-1] + replicas * len(wave))
    return {"fan_in": 2, "in_idx": np.array(in_idx), "weights": np.array(wts), "cst": np.array(cst, np.uint32), "lut_idx": None,
            "wave_offsets": np.array(offs), "wave_n_out": np.ones(len(offs) - 1, np.int32), "out_idx": np.array(out_idx), "num_wires": replicas * W}


@pytest.mark.parametrize("which", ["ripple_nand", "prefix"])
def test_gate_netlists_as_lut_circuits_word_for_word(engine, keys, params, which):
    from rustfhe_amd.circuit import CircuitRunner, prefix_adder, ripple_carry_adder
    net = ripple_carry_adder(8, nand_only=True) if which == "ripple_nand" else prefix_adder(8)
    reps = 1024
    rng = np.random.default_rng(0x6A7E)
    A, B = rng.integers(0, 256, reps), rng.integers(0, 256, reps)
    bits = np.array([[(a >> i) & 1 for i in range(8)] + [(b >> i) & 1 for i in range(8)] for a, b in zip(A, B)])
    cts = keys.encrypt_bits(bits.reshape(-1)).reshape(reps, 16, params.n + 1)
    ref = CircuitRunner(engine, net, reps)
    ref.set_inputs(cts)
    wires = ref.wires.clone()
    ref.run()
    with engine.lut(np.full(engine.p.N, E8, np.uint32)) as lut:
        c = create(engine, lut, _gate_arrays(net, reps), wires)
    try:
        got = replay(engine, c, wires)
    finally:
        engine.circuit_destroy(c)
    assert np.array_equal(got, ref.wires.cpu().numpy().view(np.uint32))
    dec = np.array(keys.decrypt_bits(ref.outputs().reshape(-1, params.n + 1))).reshape(reps, 9)
    assert np.array_equal((dec << np.arange(9)).sum(axis=1), A + B)
    ref.close()


# ---- random circuits against the host composition ----------------------------------------------------------------------------------------
def _check_random(e, seed, fan_ins, replica_counts):
    import torch
    rng = np.random.default_rng(seed)
    n1 = e.p.n + 1
    with e.lut(random_words(rng, (3, e.p.N))) as lut:
        for fan_in in fan_ins:
            for reps in replica_counts:
                d = random_circuit(rng, fan_in, reps)
                w0 = random_words(rng, (d["num_wires"], n1))
                wires = torch.from_numpy(w0.view(np.int32)).cuda()
                want = host_compose(e, lut, d, w0)
                c = create(e, lut, d, wires)
                try:
                    got = replay(e, c, wires)
                finally:
                    e.circuit_destroy(c)
                assert np.array_equal(got, want), (fan_in, reps)


REPLICAS = (1, 37, 1024, 1280)


def test_random_circuits_match_host_composition_n1024(engine):
    _check_random(engine, 101, (1, 3, 8), REPLICAS)


def test_random_circuits_match_host_composition_ks_ext(params, keys, monkeypatch):
    import rustfhe_amd as R
    e = gk.engine(R, R.Params(n=params.n, N=params.N), keys.bk_t, keys.ksk, monkeypatch, {"RTFHE_KS_MM_MIN": "0"})
    try:
        _check_random(e, 102, (2, 5), REPLICAS)
    finally:
        e.close()


@pytest.fixture(scope="module")
def keys2048(orc):
    return keys_2048(orc)


def test_random_circuits_match_host_composition_n2048(keys2048):
    import rustfhe_amd as R
    P, K = keys2048
    e = gk.engine(R, R.Params(N=2048), K.bk_t, K.ksk)
    try:
        _check_random(e, 103, (4, 7), REPLICAS)
    finally:
        e.close()


# ---- the adder -----------------------------------------------------------------------------------------------------------------------
def test_adder_on_encrypted_bytes(engine, keys):
    import rustfhe_amd as R
    p = engine.p
    reps = 1024
    net = R.lut_ripple_adder(8)
    a, b, cts = adder_inputs(R, p, keys.key0, reps, 0xB17E)
    run = R.LutCircuitRunner(engine, net, reps)
    try:
        run.set_inputs(cts)
        w0 = run.wires.cpu().numpy().view(np.uint32).copy()
        run.run()
        with engine.lut(net.polynomials(p.N)) as lut:
            want = host_compose(engine, lut, run.desc, w0)
        assert np.array_equal(run.wires.cpu().numpy().view(np.uint32), want)
        assert np.array_equal(decode(R, p, keys.key0, run.outputs()), a + b)
    finally:
        run.close()


def test_replays_new_inputs_and_a_key_change(params, keys):
    import rustfhe_amd as R
    p = R.Params(n=params.n, N=params.N)
    e = gk.engine(R, p, keys.bk_t, keys.ksk)
    reps = 300
    run = R.LutCircuitRunner(e, R.lut_ripple_adder(8), reps)
    try:
        a, b, cts = adder_inputs(R, p, keys.key0, reps, 1)
        run.set_inputs(cts)
        first = run.run().wires.cpu().numpy().copy()
        second = run.run().wires.cpu().numpy().copy()
        assert np.array_equal(first, second)
        assert np.array_equal(decode(R, p, keys.key0, run.outputs()), a + b)
        a, b, cts = adder_inputs(R, p, keys.key0, reps, 2)
        run.set_inputs(cts)
        assert np.array_equal(decode(R, p, keys.key0, run.run().outputs()), a + b)
        # a different key set loaded after recording: the replay computes with it
        k0b, k1b, bkb, kskb = R.keygen(p, 535353)
        e.load_bk_torus(bkb)
        e.load_ksk(kskb)
        a, b, cts = adder_inputs(R, p, k0b, reps, 3)
        run.set_inputs(cts)
        assert np.array_equal(decode(R, p, k0b, run.run().outputs()), a + b), "the replay computed with the old key"
    finally:
        run.close()
        e.close()


# ---- rejects ---------------------------------------------------------------------------------------------------------------------------
def test_rejects_leave_the_context_usable(engine):
    import torch
    import rustfhe_amd as R
    rng = np.random.default_rng(7)
    p = engine.p
    d = random_circuit(rng, 3, 4)
    wires = torch.zeros((d["num_wires"], p.n + 1), dtype=torch.int32, device="cuda")
    ct = random_words(rng, (37, p.n + 1))
    with engine.lut(random_words(rng, (3, p.N))) as lut:
        ref = engine.pbs_many_batch(lut, ct, 2)

        def bad(**kw):
            b = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in d.items()}
            for k, f in kw.items():
                f(b[k]) if callable(f) else b.__setitem__(k, f)
            return b

        def oob_wire(a): a[5, 1] = d["num_wires"]
        def oob_table(a): a[3] = 3
        def twice(a): a[1] = a[0]            # wave 0 has one node per replica: nodes 0 and 1 write the same wire
        cases = [("in_idx", bad(in_idx=oob_wire), "node 5"), ("lut_idx", bad(lut_idx=oob_table), "node 3"),
                 ("n_out", bad(wave_n_out=np.array([1, 4, 3, 8, 1], np.int32)), "n_out = 3"), ("twice", bad(out_idx=twice), "written twice"),
                 ("offsets", bad(wave_offsets=np.array([0, 4, 4, 12, 16, 24], np.int32)), "wave_offsets")]
        for name, b, msg in cases:
            engine.timer_begin()
            with pytest.raises(R.RtfheError) as ei:
                create(engine, lut, b, wires)
            assert engine.timer_end()[1] == 0, name
            assert ei.value.code == R._ffi.ERR_INVALID and msg in str(ei.value), (name, str(ei.value))
            if name in ("in_idx", "lut_idx", "twice"):
                assert "wave" in str(ei.value) and "node" in str(ei.value)
        try:
            for be in (R._ffi.BACKEND_NTT_EXACT, R._ffi.BACKEND_FFT_SPLIT_EXACT):
                engine.set_backend(be)
                engine.timer_begin()
                with pytest.raises(R.RtfheError) as ei:
                    create(engine, lut, d, wires)
                assert engine.timer_end()[1] == 0
                assert ei.value.code == R._ffi.ERR_INVALID and "mirror" in str(ei.value)
        finally:
            engine.set_backend(R._ffi.BACKEND_FFT64_MIRROR)
        assert np.array_equal(engine.pbs_many_batch(lut, ct, 2), ref)


# ---- lifetimes ---------------------------------------------------------------------------------------------------------------------------
def test_table_destroyed_first_and_context_destroyed_first(params, keys):
    import torch
    import rustfhe_amd as R
    p = R.Params(n=params.n, N=params.N)
    e = gk.engine(R, p, keys.bk_t, keys.ksk)
    rng = np.random.default_rng(9)
    d = random_circuit(rng, 4, 37)
    w0 = random_words(rng, (d["num_wires"], p.n + 1))
    tv = random_words(rng, (3, p.N))
    wires = torch.from_numpy(w0.view(np.int32)).cuda()
    lut = e.lut(tv)
    keep = create(e, lut, d, wires)
    alone = create(e, lut, d, wires)
    want = replay(e, keep, wires)
    lut.close()
    e.circuit_destroy(keep)
    with e.lut(np.zeros((3, p.N), np.uint32)) as other:     # (takes whatever memory the table had)
        for _ in range(2):
            wires.copy_(torch.from_numpy(w0.view(np.int32)))
            assert np.array_equal(replay(e, alone, wires), want)
        assert other.n_lut == 3
    e.close()
    with pytest.raises(R.RtfheError) as ei:
        e.circuit_launch(alone)
    assert ei.value.code == R._ffi.ERR_STATE
    e.circuit_destroy(alone)


# ---- the example ------------------------------------------------------------------------------------------------------------------------
def test_lut_circuit_adder_example(engine, keys):
    spec = importlib.util.spec_from_file_location("lut_circuit_adder", os.path.join(ROOT, "examples", "lut_circuit_adder.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    a, b, got, ms = ex.run(engine, keys.key0, 1024, seed=0xE8, timed=2)
    assert np.array_equal(got, a + b)
    assert ms > 0
