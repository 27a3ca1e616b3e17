"""TEST INFRASTRUCTURE: inputs whose blind rotation walks rotations the test chooses, and inputs that stand on the edges of the mod switch
(tests/test_rotation_kit.py holds both to what they claim on the CPU; tests/test_gpu_rotation_schedules.py,
tests/test_gpu_rotation_schedules_exact.py and tests/test_gpu_mod_switch_edges.py run them through every bootstrap kernel family).  CPU only:
numpy and tests/kit.py.

The schedule.  A mask word a_i = r << SH, SH = 32 - log2 N - 1, is switched to abar_i = r exactly, so the CMUX step i of gate g rotates by
rotation(N, g, i) and not by whatever a ciphertext happens to hold.  r = 64 coarse + fine: the coarse part is the whole-lane-row shift of
every gather, the fine part the lane shift; the fine parts are no wrap, one, two, half a row less one, half, half plus one, all but two, all
but one.

The mod switch (rtfhe_kernels.hpp: mod_switch; rtfhe_gate_frame.hpp: gate_mask) at the grid S = SH + k, k = log2 n_out: the body word is
floored, a mask word rounded, both scaled back by 2^k.  The rounding adds half a step mod 2^32: tfhe.rs:108 uses wrapping_add, so a mask word
in the top half-step rounds up to 2N, which is 0 -- the wrap is the reference's behaviour, and no switched value is ever 2N."""
import numpy as np

from kit import random_words

U32 = 0xFFFFFFFF
GATES, STEPS = 8, 64
FINE = (0, 1, 2, 31, 32, 33, 62, 63)
RINGS = (1024, 2048)


def sh_of(N):
    return 32 - (int(N).bit_length() - 1) - 1


def rotation(N, g, i):
    """gate g < 8, step i < 64: every gate alone sees every coarse part, the eight gates together every (coarse, fine) pair"""
    Q = 2 * N // 64
    return 64 * (i % Q) + FINE[(g + i + 4 * (i // Q)) % 8]


def b_edges(N):
    return (0, 1, N - 1, N, N + 1, 2 * N - 1, 2 * N - 2, N // 2)


def schedule_inputs(rng, N, n, steps=STEPS):
    """u32[8][n + 1]: mask word i < steps of gate g is rotation(N, g, i) << SH, the mask words behind the prefix are random, the body word is
    b_edges(N)[g] << SH, for odd g with every bit below SH set (the floor drops them)"""
    sh = sh_of(N)
    t = random_words(rng, (GATES, n + 1))
    for g in range(GATES):
        for i in range(min(steps, n)):
            t[g, i] = rotation(N, g, i) << sh
        t[g, n] = (b_edges(N)[g] << sh) + (((1 << sh) - 1) if g % 2 else 0)
    return t


def mod_switch(words, is_body, S, k):
    """rtfhe_kernels.hpp's mod_switch on u32 words: floor for the body word, round for a mask word (the sum mod 2^32), scaled back by 2^k"""
    w = np.asarray(words, np.uint64)
    return ((w if is_body else (w + (1 << (S - 1))) & U32) >> S << k).astype(np.int64)


def edge_targets(N, k):
    return (0, 1, (N >> k) - 1, N >> k, (2 * N >> k) - 1)


def edge_words(N, k):
    """The mask words around the rounding boundaries of the grid S = SH + k: for every q of edge_targets the last word that rounds to q - 1, the
    first and the last that round to q, the first that rounds to q + 1; then 0xFFFFFFFF and 0.  22 words, u32."""
    S = sh_of(N) + k
    half = 1 << (S - 1)
    out = []
    for q in edge_targets(N, k):
        out += [(q << S) - half - 1, (q << S) - half, (q << S) + half - 1, (q << S) + half]
    return np.array([w & U32 for w in out] + [U32, 0], np.uint32)


def edge_rounds_to(N, k):
    """what each of edge_words(N, k) is switched to as a mask word, from its construction: q - 1, q, q, q + 1 on the grid, mod 2N / 2^k,
    scaled back; 0xFFFFFFFF wraps to 0"""
    m = 2 * N >> k
    out = []
    for q in edge_targets(N, k):
        out += [(q - 1) % m, q, q, (q + 1) % m]
    return np.array(out + [0, 0], np.int64) << k


def body_edge_words(N, k):
    """The body words around the floor boundaries of the grid S = SH + k: for every q of edge_targets the last word of q - 1, the first and the
    last of q; then 0xFFFFFFFF.  16 words, u32."""
    S = sh_of(N) + k
    out = []
    for q in edge_targets(N, k):
        out += [(q << S) - 1, q << S, (q << S) + (1 << S) - 1]
    return np.array([w & U32 for w in out] + [U32], np.uint32)


def body_floors_to(N, k):
    m = 2 * N >> k
    out = []
    for q in edge_targets(N, k):
        out += [(q - 1) % m, q, q]
    return np.array(out + [m - 1], np.int64) << k


def edge_inputs(rng, N, n, k, part=0):
    """u32[8][n + 1]: mask word i of gate g is edge_words(N, k)[(i + 5 g) mod 22], so every edge word stands at several step indices and in
    every gate once n >= 44.  The body word of gate g is body_edge_words(N, k)[8 part + g]: the sixteen body words take two parts, 0 and 1.
    Every word is prescribed; rng is not drawn from and is there so that both makers are called alike."""
    ew, bw = edge_words(N, k), body_edge_words(N, k)
    t = np.empty((GATES, n + 1), np.uint32)
    for g in range(GATES):
        t[g, :n] = ew[(np.arange(n) + 5 * g) % len(ew)]
        t[g, n] = bw[(GATES * part + g) % len(bw)]
    return t


def edge_rows(rng, N, n, k):
    """both parts of edge_inputs: u32[16][n + 1], every body edge word once"""
    return np.concatenate([edge_inputs(rng, N, n, k, 0), edge_inputs(rng, N, n, k, 1)])


# ---- batches beyond the prescribed rows, and what a failing comparison says -------------------------------------------------------------
SIZES = {"1": (0, 1), "3": (0, 3), "8": (0, 8), "16": (0, 16), "C+8": (1, 8), "2C+8": (2, 8), "3C+8": (3, 8), "4C": (4, 0), "4C+8": (4, 8)}


def size(sym, C):
    """a batch size named by its place in the dispatch on a device of C CUs"""
    a, b = SIZES[sym]
    return a * C + b


def tiled(rows, count):
    """gate g of the batch is row g mod len(rows): the prescribed rows repeated, which costs the oracle nothing"""
    rows = np.asarray(rows)
    return np.tile(rows, (-(-count // len(rows)),) + (1,) * (rows.ndim - 1))[:count]


def first_difference(got, exp, t, N, k=0, steps=None):
    """None if the rows are equal, else (g, text): the first differing gate of the batch and a line that places it -- its row of the inputs
    `t` the batch tiles, its switched body word, and the steps of its mask prefix whose rotations are the schedule's landmarks"""
    got, exp = np.asarray(got), np.asarray(exp)
    G = got.shape[0]
    assert exp.shape[0] == G and got.size == exp.size, (got.shape, exp.shape)
    bad = np.flatnonzero((got.reshape(G, -1) != exp.reshape(G, -1)).any(axis=1))
    if bad.size == 0:
        return None
    g = int(bad[0])
    row = t[g % len(t)]
    S = sh_of(N) + k
    n = len(row) - 1
    ab = mod_switch(row[:n if steps is None else min(steps, n)], False, S, k)
    marks = {0, 1, N - 1, N, N + 1, 2 * N - 2, 2 * N - 1}
    at = ["step %d: r = %d (coarse %d, fine %d, plane %d)" % (i, r, r >> 6, r & 63, r & 1) for i, r in enumerate(ab.tolist()) if r in marks]
    return g, ("%d of %d gates differ, the first is gate %d (input row %d): body word 0x%08X, bbar = %d; mask words [0..3] = %s, abar[0..3] = %s; "
               "landmark rotations of its prefix: %s" % (bad.size, G, g, g % len(t), int(row[n]), int(mod_switch(row[n:], True, S, k)[0]),
                                                        " ".join("0x%08X" % int(x) for x in row[:4]), ab[:4].tolist(), "; ".join(at[:8]) or "none"))


def first_wrong_step(run, oracle, row, N, steps=STEPS):
    """For one differing gate with input row `row`: run(s) and oracle(s) give its accumulator after s steps (the caller keeps the batch and the
    engine that failed, so the same kernel runs).  Bisection finds a step s with equal accumulators before it and different ones behind it;
    the line names that step's word and rotation: the coarse / fine / plane class of the failure."""
    if not np.array_equal(run(0), oracle(0)):
        return "the starting accumulator differs: bbar = %d" % int(mod_switch(row[-1:], True, sh_of(N), 0)[0])
    lo, hi = 0, steps                    # equal after lo steps, different after hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if np.array_equal(run(mid), oracle(mid)):
            lo = mid
        else:
            hi = mid
    r = int(mod_switch(row[lo:lo + 1], False, sh_of(N), 0)[0])
    return "first wrong step %d: word 0x%08X, r = %d (coarse %d, fine %d, plane %d)" % (lo, int(row[lo]), r, r >> 6, r & 63, r & 1)


def accumulators_differ(run, oracle, t, exp, N, count, steps=STEPS):
    """run(rows, s): the device's accumulators u32[len(rows)][2N] after s steps; oracle(row, s): the oracle's for one row; t, exp: the
    prescribed rows and the oracle's accumulators after `steps`.  None if the batch of `count` gates (t tiled) equals exp tiled, else the
    first differing gate placed by first_difference and its first wrong step by first_wrong_step, on the same batch."""
    rows = tiled(t, count)
    diff = first_difference(run(rows, steps), tiled(exp, count), t, N, steps=steps)
    if diff is None:
        return None
    g, text = diff
    row = t[g % len(t)]
    return text + "; " + first_wrong_step(lambda s: run(rows, s)[g], lambda s: oracle(row, s), row, N, steps)
