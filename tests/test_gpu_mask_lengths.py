"""GPU: every bootstrap kernel family at the edges of the TLWE dimension n (rtfhe_ctx_create accepts 1 <= n <= 767 at both rings).

n sizes every family's LDS carve (npad = n + 1 rounded up to 64), is the step count of the blind rotation (and so the depth the key prefetch
rings run to), lowers the time-sliced launch from six gates per CU to five (n >= 640) and the N = 2048 whole rounds from four gates per CU to
three (n >= 704), and chooses the 16-byte or the scalar path of k_lut_gather / k_lut_scatter (n + 1 a multiple of 4 or not).  Mask lengths:
1, 2 (fewer steps than any prefetch depth); 63 / 639 / 703 / 767 (n + 1 == npad: the body word is the last word of its LDS row); 64 / 640 / 704
(one word into a new 64-block, n + 1 odd); 639 -> 640 (six -> five gates per CU time-sliced); 703 -> 704 (four -> three gates per CU at
N = 2048); 767 (the maximum).  Batch sizes derive from the device's CU count C so that each reaches the same launch shape on any device.
Every comparison is np.array_equal on uint32 words: there is no tolerance in this file.

Wall time, measured on an MI355X (256 CUs, 16 host threads for the oracle; profiles/r10/README.md): 130.7 s for this file against 115.3 s for
the rest of the GPU suite -- 113 % where 50 % was budgeted.  103 s are the CPU oracle on the six long masks of the default-engine sweep; the
random picks are at their floor of 8 per batch and the forced shapes at the smallest allowed subset plus 640 / 704, and the mask lengths, the
boundary gates and the default-engine sweep are not cut."""
import numpy as np
import pytest

import gpu_kit as gk
from kit import random_words
from lut_circuit_kit import adder_inputs, create, decode, host_compose, random_circuit, replay
from mask_kit import FORCED, FORCED_MASKS, ORDER, Mask, _picks
from pbs_oracle import oracle_pbs, oracle_pbs_enc, oracle_pbs_many

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module", params=ORDER, ids=lambda m: "N%d-n%d" % m)
def mask(request, orc):
    """One key set from the oracle's keygen and one default engine per (N, n).  No try / skip around the creation: an (N, n) inside the
    documented range that cannot be created fails every test of that mask length."""
    m = Mask(orc, *request.param)
    yield m
    m.e.close()


# ---- the default engine (FP64 mirror backend) against the oracle ------------------------------------------------------------------------
def test_default_engine_every_batch_shape_against_the_oracle(mask):
    """gate_batch(NAND), bootstrap_batch, pbs_batch (3 random rows), pbs_many_batch (n_out 1, 2, 8) and an encrypted table (n_out 4, and
    pbs_batch) on uniformly random words at every batch size; the oracle on the gates of _picks (all gates of gate_batch up to 4C)."""
    import rustfhe_amd as R
    m, orc, P, K, e = mask, mask.orc, mask.P, mask.K, mask.e
    rng = np.random.default_rng(100 * m.N + m.n)
    tv = random_words(rng, (3, m.N))
    trl = R.encrypt_lut(m.p, K.key1, tv, seed=m.n)
    with e.lut(tv) as lut, e.lut_encrypted(trl) as enc:
        for G in gk.sizes(m.N, m.C):
            c0, c1 = random_words(rng, (G, m.n + 1)), random_words(rng, (G, m.n + 1))
            idx = rng.integers(0, 3, G).astype(np.int32)
            pick = _picks(G, m.N, m.C, rng)
            out = e.gate_batch(R.NAND, c0, c1)
            sel = list(range(G)) if G <= 4 * m.C else pick
            assert np.array_equal(out[sel], m.gates(orc.NAND, c0[sel], c1[sel])), ("gate_batch", G)
            assert np.array_equal(e.bootstrap_batch(c0)[pick], m.gates(orc.COPY, c0[pick], None)), ("bootstrap_batch", G)
            got = e.pbs_batch(lut, c0, idx)
            exp = gk.pmap(lambda g: oracle_pbs(orc, P, gk.oracle_plan(orc, m.N), K.bk_f, K.ksk, tv[idx[g]], c0[g]), pick)
            assert np.array_equal(got[pick], np.stack(exp)), ("pbs_batch", G)
            for n_out in (1, 2, 8):
                got = e.pbs_many_batch(lut, c1, n_out, idx)
                exp = gk.pmap(lambda g: oracle_pbs_many(orc, P, gk.oracle_plan(orc, m.N), K.bk_f, K.ksk, tv[idx[g]], c1[g], n_out), pick)
                assert np.array_equal(got[pick], np.stack(exp)), ("pbs_many_batch", n_out, G)
            got = e.pbs_many_batch(enc, c0, 4, idx)
            exp = gk.pmap(lambda g: oracle_pbs_enc(orc, P, gk.oracle_plan(orc, m.N), K.bk_f, K.ksk, trl[idx[g]], c0[g], 4), pick)
            assert np.array_equal(got[pick], np.stack(exp)), ("encrypted table, n_out 4", G)
            got = e.pbs_batch(enc, c1, idx)
            exp = gk.pmap(lambda g: oracle_pbs_enc(orc, P, gk.oracle_plan(orc, m.N), K.bk_f, K.ksk, trl[idx[g]], c1[g], 1)[0], pick)
            assert np.array_equal(got[pick], np.stack(exp)), ("encrypted table, pbs_batch", G)
            if m.n >= 63:
                b0, b1 = rng.integers(0, 2, G), rng.integers(0, 2, G)
                assert K.decrypt_bits(e.gate_batch(R.NAND, K.encrypt_bits(b0), K.encrypt_bits(b1))) == list(1 - (b0 & b1)), ("decrypt", G)


def test_blind_rotation_prefixes_at_the_edges_of_the_step_count(mask):
    """blind_rotate_batch(t, steps) for steps in {0, 1, n - 1, n} (the step count is n: its edges) on 5 and on C + C//6 samples."""
    m, orc, e = mask, mask.orc, mask.e
    rng = np.random.default_rng(200 * m.N + m.n)
    for G in (5, m.C + m.C // 6):
        t = random_words(rng, (G, m.n + 1))
        pick = _picks(G, m.N, m.C, rng)
        for steps in sorted({0, 1, m.n - 1, m.n}):
            got = e.blind_rotate_batch(t, steps).reshape(G, -1)
            exp = gk.pmap(lambda g: orc.blind_rotate(m.P, gk.oracle_plan(orc, m.N), m.K.bk_f, None, t[g], steps), pick)
            assert np.array_equal(got[pick], np.stack(exp)), (G, steps)


# ---- every other shape against the default engine, whole batches ------------------------------------------------------------------------
def test_forced_shapes_equal_the_default_engine(mask, monkeypatch):
    """One engine per forced shape, same keys: gate_batch, pbs_batch, pbs_many_batch(n_out = 4) and the encrypted table give the default
    engine's words on whole batches.  Mask lengths: 1, 63, 64 and the largest of the ring (the required subset) plus the first n past the
    change of the dispatch (640: five gates per CU time-sliced, where RTFHE_PAIR_RR=0 differs from the default in a new way; 704: three
    gates per CU in the N = 2048 whole rounds).  2, 639 and 703 run the same carve as their neighbours 1, 640 / 63 and 704 / 63 one word
    apart and are covered against the oracle above; leaving them out here keeps the file inside its time budget."""
    import rustfhe_amd as R
    m, e = mask, mask.e
    if m.n not in FORCED_MASKS[m.N]:
        return
    rng = np.random.default_rng(300 * m.N + m.n)
    tv = random_words(rng, (3, m.N))
    trl = R.encrypt_lut(m.p, m.K.key1, tv, seed=m.n + 1)
    cases = []
    with e.lut(tv) as lut, e.lut_encrypted(trl) as enc:
        for G in gk.forced_sizes(m.N, m.C):
            c0, c1 = random_words(rng, (G, m.n + 1)), random_words(rng, (G, m.n + 1))
            idx = rng.integers(0, 3, G).astype(np.int32)
            cases.append((c0, c1, idx, e.gate_batch(R.NAND, c0, c1), e.pbs_batch(lut, c0, idx), e.pbs_many_batch(lut, c1, 4, idx),
                          e.pbs_many_batch(enc, c0, 4, idx)))
    for env in FORCED[m.N]:
        f = m.engine(monkeypatch, env)
        try:
            with f.lut(tv) as lut, f.lut_encrypted(trl) as enc:
                for c0, c1, idx, gate, pbs, many, many_enc in cases:
                    G = len(idx)
                    assert np.array_equal(f.gate_batch(R.NAND, c0, c1), gate), (env, "gate_batch", G)
                    assert np.array_equal(f.pbs_batch(lut, c0, idx), pbs), (env, "pbs_batch", G)
                    assert np.array_equal(f.pbs_many_batch(lut, c1, 4, idx), many), (env, "pbs_many_batch", G)
                    assert np.array_equal(f.pbs_many_batch(enc, c0, 4, idx), many_enc), (env, "encrypted table", G)
        finally:
            f.close()


# ---- the exact backends -----------------------------------------------------------------------------------------------------------------
def test_exact_backends_agree_and_match_the_exact_oracle(mask):
    """gate_batch(XOR) at 1, C + C//6, 4C, 5C, 6C: the NTT and the split-FFT backend equal each other word for word on the whole batch and
    refuse a PBS.  Against the exact-integer oracle (schoolbook products): whole gates for n <= 64 on the boundary gates; for the long
    masks blind-rotation prefixes of 1 and 3 steps on 5 and on C + C//6 samples, and encrypted bits decrypt."""
    import rustfhe_amd as R
    m, orc, K, e = mask, mask.orc, mask.K, mask.e
    C = m.C
    rng = np.random.default_rng(400 * m.N + m.n)
    backends = (R._ffi.BACKEND_NTT_EXACT, R._ffi.BACKEND_FFT_SPLIT_EXACT)
    try:
        for G in (1, C + C // 6, 4 * C, 5 * C, 6 * C):
            c0, c1 = random_words(rng, (G, m.n + 1)), random_words(rng, (G, m.n + 1))
            outs = []
            for b in backends:
                e.set_backend(b)
                outs.append(e.gate_batch(R.XOR, c0, c1))
            assert np.array_equal(outs[0], outs[1]), G
            if m.n <= 64:
                s = {0, G - 1}
                for bnd in range(4 * C, G, 4 * C):
                    s |= {bnd - 1, bnd}
                s = sorted(s)
                assert np.array_equal(outs[0][s], m.gates(orc.XOR, c0[s], c1[s], backend=orc.BACKEND_EXACT)), G
            elif G <= 4 * C:
                b0, b1 = rng.integers(0, 2, G), rng.integers(0, 2, G)
                assert K.decrypt_bits(e.gate_batch(R.XOR, K.encrypt_bits(b0), K.encrypt_bits(b1))) == list(b0 ^ b1), G
        if m.n > 64:
            for G in (5, C + C // 6):
                t = random_words(rng, (G, m.n + 1))
                pick = sorted({0, G - 1} | set(rng.choice(G, min(G, 4), replace=False).tolist()))
                for steps in (1, 3):
                    exp = np.stack(gk.pmap(lambda g: orc.blind_rotate(m.P, gk.oracle_plan(orc, m.N, orc.BACKEND_EXACT), None, K.bk_t, t[g], steps), pick))
                    for b in backends:
                        e.set_backend(b)
                        assert np.array_equal(e.blind_rotate_batch(t, steps).reshape(G, -1)[pick], exp), (b, G, steps)
        ct = random_words(rng, (37, m.n + 1))
        e.set_backend(R._ffi.BACKEND_FFT64_MIRROR)
        with e.lut(random_words(rng, (1, m.N))) as lut:
            for b in backends:
                e.set_backend(b)
                with pytest.raises(R.RtfheError) as ei:
                    e.pbs_batch(lut, ct)
                assert ei.value.code == R._ffi.ERR_INVALID
    finally:
        e.set_backend(R._ffi.BACKEND_FFT64_MIRROR)


# ---- LUT circuits: the 16-byte and the scalar rows of k_lut_gather / k_lut_scatter ------------------------------------------------------
LUT_MASKS = {(1024, 63): (False, True), (1024, 64): (False,), (1024, 640): (False,), (1024, 767): (False,), (2048, 64): (False,)}


def test_lut_circuit_adder_vector_and_scalar_rows(mask):
    """lut_ripple_adder(8), 4C + 1 replicas: n = 63 and 767 have 16-byte rows (n + 1 a multiple of 4), n = 64 and 640 take the scalar
    k_lut_gather<F, false> / k_lut_scatter<false>; at n = 63 once more with a wire table whose base is 4 bytes past a 16-byte boundary (the
    alignment half of the condition).  The wire table equals host_compose word for word on two replays; the sums decrypt for n >= 640.
    The adder's nodes all have the constant 0, so a random circuit (fan-in 3, random weights, constants and tables, n_out 1 .. 8) runs at
    the same mask lengths and replica count as well: a gather that loses the constant in the body word passes the adder and fails here."""
    import torch
    import rustfhe_amd as R
    m, e = mask, mask.e
    for misaligned in LUT_MASKS.get((m.N, m.n), ()):
        reps = 4 * m.C + 1
        net = R.lut_ripple_adder(8)
        a, b, cts = adder_inputs(R, m.p, m.K.key0, reps, 0xA000 + m.n)
        run = R.LutCircuitRunner(e, net, reps)
        try:
            if misaligned:
                words = run.wires.numel()
                big = torch.zeros(words + 8, dtype=torch.int32, device="cuda")
                run.wires = big[1:1 + words].view(run.wires.shape)
                assert run.wires.data_ptr() % 16 == 4
            run.set_inputs(cts)
            w0 = run.wires.cpu().numpy().view(np.uint32).copy()
            with e.lut(net.polynomials(m.N)) as lut:
                want = host_compose(e, lut, run.desc, w0)
            for _ in range(2):                       # the scatter zeroes its source for the next replay
                run.run()
                assert np.array_equal(run.wires.cpu().numpy().view(np.uint32), want), (m.n, misaligned)
            if m.n >= 640:
                assert np.array_equal(decode(R, m.p, m.K.key0, run.outputs()), a + b)
        finally:
            run.close()
        rng = np.random.default_rng(500 * m.N + m.n + misaligned)
        d = random_circuit(rng, 3, reps)
        assert np.count_nonzero(d["cst"]) > 0
        w0 = random_words(rng, (d["num_wires"], m.n + 1))
        big = torch.zeros(w0.size + 8, dtype=torch.int32, device="cuda")
        wires = big[1:1 + w0.size].view(w0.shape) if misaligned else big[:w0.size].view(w0.shape)
        wires.copy_(torch.from_numpy(w0.view(np.int32)))
        with e.lut(random_words(rng, (3, m.N))) as lut:
            c = create(e, lut, d, wires)
            try:
                for _ in range(2):                   # the last wave swaps two wires in place: the second replay starts from the first's table
                    w0 = host_compose(e, lut, d, w0)
                    assert np.array_equal(replay(e, c, wires), w0), (m.n, misaligned, "random circuit")
            finally:
                e.circuit_destroy(c)


# ---- the time-sliced launch at five gates per CU ----------------------------------------------------------------------------------------
def test_time_sliced_launch_at_five_gates_per_cu(mask, monkeypatch):
    """n = 640 and 767 (npad 704 / 768: five gates per CU fit, six do not): 4C + 1 and 5C gates take fewer bootstrap launches than an engine
    created with RTFHE_PAIR_RR=0 (one time-sliced launch instead of a round and a tail), 6C takes the same number (round + tail either way)."""
    import rustfhe_amd as R
    m, e = mask, mask.e
    if (m.N, m.n) not in ((1024, 640), (1024, 767)):
        return
    C = m.C
    rng = np.random.default_rng(m.n)
    off = m.engine(monkeypatch, {"RTFHE_PAIR_RR": "0"})
    try:
        def launches(eng, c0, c1):
            eng.timer_begin()
            out = eng.gate_batch(R.NAND, c0, c1)
            return eng.timer_end()[1], out
        for G, fewer in ((4 * C + 1, True), (5 * C, True), (6 * C, False)):
            c0, c1 = random_words(rng, (G, m.n + 1)), random_words(rng, (G, m.n + 1))
            (ka, a), (kb, b) = launches(e, c0, c1), launches(off, c0, c1)
            assert np.array_equal(a, b), G
            assert (ka < kb) if fewer else (ka == kb), (G, ka, kb)
    finally:
        off.close()
