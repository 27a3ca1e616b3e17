"""TEST INFRASTRUCTURE: what tests/test_gpu_large_buffers.py (and its later siblings, tests/test_gpu_*_large.py) is written with -- device buffers past 2 GiB, 4 GiB and 8 GiB (DESIGN.md 6.2,
"Address arithmetic").  torch is imported inside the functions, as in gpu_kit.py: the module imports without a GPU and its arithmetic half
(boundaries, ks_segment, probe_items) is checked on the CPU by tests/test_large_plans_host.py.  Nothing here ever creates a large array on the
host: the big buffers are made, filled, compared and probed on the device, and only the probe rows (a few hundred) come down."""
import numpy as np

import gpu_kit as gk

NAMES = ("B31", "B32", "W31", "W32")          # byte offsets 2^31 and 2^32, then word index 2^31 and 2^32 of a uint32_t array: bytes 2^33, 2^34
EDGE = 32                                     # items probed either side of a boundary, and at both ends of a call
RANDOM_PROBES = 128
PIECE = 1 << 30                               # elements one random fill covers
HEADROOM = 2 << 30                            # free memory need() leaves untouched


def boundaries(item_bytes):
    """{name: b}: item b of an array of items of `item_bytes` bytes is the one that holds, or starts at, byte offset 2^31 (B31), 2^32 (B32),
    2^33 (W31) and 2^34 (W32) -- items 0 .. b - 1 lie wholly below the offset"""
    return {name: (1 << k) // item_bytes for name, k in zip(NAMES, (31, 32, 33, 34))}


def crossed(count, item_bytes):
    """the boundaries an array of `count` such items reaches past, in order"""
    return [name for name, k in zip(NAMES, (31, 32, 33, 34)) if count * item_bytes > (1 << k)]


def ks_segment(N):
    """seg_max of launch_key_switch_mm (rtfhe_stages.hip), restated: the samples one k_key_switch_mm launch addresses with 32-bit byte offsets,
    2^31 bytes of N + 1 words each, rounded down to whole workgroups of 16 samples x 4 tiles x 8 waves"""
    per_block = 16 * 4 * 8
    return (1 << 31) // ((N + 1) * 4) // per_block * per_block


def probe_items(count, item_bytes, segment=None, seed=0):
    """The items the oracle checks, sorted: the first and the last EDGE of the call, the EDGE ending at and the EDGE starting at every boundary
    the array crosses and -- segment given -- at every multiple of it below count, and RANDOM_PROBES drawn from a fixed seed."""
    marks = [0, count] + [boundaries(item_bytes)[name] for name in crossed(count, item_bytes)]
    if segment:
        marks += list(range(segment, count, segment))
    s = set()
    for m in marks:
        s |= set(range(max(m - EDGE, 0), min(m + EDGE, count)))
    rng = np.random.default_rng([count, item_bytes, seed])
    s |= set(rng.integers(0, count, RANDOM_PROBES).tolist())
    return np.array(sorted(s), np.int64)


def device_words(n_words, seed):
    """an int32 device tensor of n_words independent random words, filled in place in pieces of at most 2^30 elements from ONE generator (its
    Philox offset runs on from piece to piece): no block of the buffer repeats, so a row read 2^31 or 2^32 bytes away from where it lies
    cannot go unseen"""
    import torch
    gen = torch.Generator(device="cuda")
    gen.manual_seed(int(seed))
    t = torch.empty(int(n_words), dtype=torch.int32, device="cuda")
    for i in range(0, int(n_words), PIECE):
        t[i:i + PIECE].random_(-(1 << 31), 1 << 31, generator=gen)
    return t


def need(nbytes):
    """pytest.skip unless the device has nbytes + 2 GiB free"""
    import pytest
    import torch
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < nbytes + HEADROOM:
        pytest.skip("needs %.2f GB of device memory plus 2 GiB of headroom, %.2f GB are free" % (nbytes / 1e9, free / 1e9))


def guarded_device(words):
    """gk.guarded_out made on the device: int32[words + CANARY], every word gk.FILL"""
    import torch
    return torch.full((int(words) + gk.CANARY,), int(np.uint32(gk.FILL).view(np.int32)), dtype=torch.int32, device="cuda")


def check_canary(t, words):
    """the CANARY words behind the payload still hold gk.FILL"""
    tail = gk.words_of(t[int(words):])
    assert tail.size == gk.CANARY and (tail == gk.FILL).all(), "words behind d_out were written"


def rows_of(t, width, items, offset=0):
    """rows `items` (a sorted index array) of the device array [..][width] that starts `offset` words into t, as u32 on the host"""
    import torch
    idx = torch.from_numpy(np.asarray(items, np.int64)).cuda()
    body = t.reshape(-1)[int(offset):]
    n = body.numel() // int(width)
    return body[:n * int(width)].view(n, int(width))[idx].cpu().numpy().view(np.uint32)


def same_as_chunks(call, inputs, out, count, chunk):
    """The big call's output, EVERY word of it, against the same call made on slices of the same device inputs, `chunk` items at a time.
    inputs: [(tensor, words per item) or None]; out: (tensor, words per item).  call(slices, d_chunk_out, cnt) runs the entry point on cnt
    items into d_chunk_out (one chunk-sized buffer behind gk.FILL canaries, reused) and synchronises; each chunk is then compared with its
    slice of the big output on the device.  A second opinion from the same code at offsets the rest of the suite pins to the oracle."""
    import torch
    d_out, ow = out[0].reshape(-1), out[1]
    d_chunk = guarded_device(chunk * ow)
    for off in range(0, count, chunk):
        cnt = min(chunk, count - off)
        slices = [None if i is None else i[0].reshape(-1)[off * i[1]:(off + cnt) * i[1]] for i in inputs]      # (views: the inputs are contiguous)
        call(slices, d_chunk, cnt)
        assert torch.equal(d_chunk[:cnt * ow], d_out[off * ow:(off + cnt) * ow]), "items %d .. %d differ from the same call on a slice" % (off, off + cnt - 1)
        check_canary(d_chunk, chunk * ow)
    del d_chunk


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _tile_bytes(N):
    return 16 * (N + 1) * 4           # 65,600 (N = 1024) or 131,136 (N = 2048) per tile of 16 samples


def _split_path_taken(e, detail, samples, N, label, keys_only):
    """The signs that the big call ran the batch key switch in more than one segment.  keys_only: what a context with the same keys holds
    before any batch (the slice calls' context, measured at the start).  The library does not report a segment count -- it counts the whole
    batch key switch as one launch --, so the figure printed here is DERIVED from the kit's restatement of seg_max; the evidence is the three
    assertions below and the mutant of profiles/r32/README.md."""
    ms, ks_ms, launches = detail
    held = report(label, e) - keys_only
    print("[large] %s: %.1f ms on the device, %.2f ms of it in the batch key switch, %d launches, ceil(samples / seg_max) = %d (derived), scratch %.2f GB" %
          (label, ms, ks_ms, launches, -(-samples // ks_segment(N)), held / 1e9))
    assert ks_ms > 0, "the batch key switch (launch_key_switch_mm) did not run: the batch stayed on the fused kernel"
    assert launches >= 2, "a blind-rotation launch and the batch key switch"
    assert samples > ks_segment(N), "more than one key-switch segment"
    assert held >= -(-samples // 16) * _tile_bytes(N) > 1 << 31, "the context's scratch beyond its keys holds the batch's samples, and they lie across 2^31 bytes"


def _chunk_samples(N):
    """samples of a slice call whose sample buffer stays below 2^30 bytes"""
    return (1 << 30) // ((N + 1) * 4) // 1024 * 1024


def report(name, eng=None):
    """one line per test for the log: torch's peak allocation and what the context holds (rtfhe_ctx_memory_bytes)"""
    import torch
    ctx = eng.memory_bytes() if eng is not None else 0
    print("\n[large] %s: torch peak %.2f GB, context %.2f GB" % (name, torch.cuda.max_memory_allocated() / 1e9, ctx / 1e9))
    return ctx


def release():
    """what every test ends with, after closing its contexts and dropping its tensors: the allocator's cache goes back to the device"""
    import gc
    import torch
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
