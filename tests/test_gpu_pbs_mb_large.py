"""GPU: rtfhe_pbs_mb_batch_dev past 2^31 bytes of samples ("Address arithmetic"; the row of k_pbs_mb / k_pbs_mb_wg / launch_mb),
written with tests/large_kit.py as tests 1-6 of tests/test_gpu_large_buffers.py are.  The call launches once for the whole count (launch_mb; it
does not go through the round / tail ladder): gate numbers blockIdx.x * 4 + wave or blockIdx.x up to 524,836, their a.ext stores into the
stream's sample buffer -- tiles of 16 samples across byte offset 2^31 -- and launch_key_switch_rows behind it in two segments.

n = 3, g = 2: one full and one ragged group, two steps per gate.  Three random tables, a random lut_idx of which five entries, all in the second
key-switch segment, are out of range: sync reports them once and their rows keep the fill.  Each test asserts that the batch took the split
path (large_kit._split_path_taken), EVERY output word against the same call on slices on a second context whose sample buffer stays below 2^30
bytes (large_kit.same_as_chunks), the rows of large_kit.probe_items -- both ends, 32 either side of 2^31 bytes of samples and of the key-switch
segment edge, 128 at random -- and the neighbours of the skipped gates against tests/mb_oracle.py, and the canary.  No tolerance."""
import numpy as np
import pytest

import gpu_kit as gk
import large_kit as lk
import mb_oracle as mo
from kit import random_words

pytestmark = pytest.mark.gpu

N_SMALL, G_BITS = 3, 2
BAD_IDX = (3, -1, 2 ** 31 - 1, -2 ** 31, 7)


def _pbs_mb(orc, monkeypatch, N, count, shape, label):
    import rustfhe_amd as R
    import torch
    n, g = N_SMALL, G_BITS
    w1 = n + 1
    seg = lk.ks_segment(N)
    assert count > seg and count - seg > 1060
    lk.need(-(-count // 16) * lk._tile_bytes(N) + (1 << 30) + 4 * (3 * w1 + 1) * count)
    if shape:
        monkeypatch.setenv("RTFHE_MB_SHAPE", shape)
    P, p = orc.Params(n=n, N=N), R.Params(n=n, N=N)
    plan = orc.Plan(N)
    K = orc.Keys(P, 0x4D4C00 + N, plan=plan)
    words = R.mbk_keygen(p, K.key0, K.key1, g, seed=0x4D4C01 + N)
    key_f, tab = mo.key_spectra(P, plan, words), mo.Tables(R, N)
    tv = random_words(np.random.default_rng(0x4D4C02 + N), (3, N))
    e, e_small = gk.engine(R, p, K.bk_t, K.ksk), gk.engine(R, p, K.bk_t, K.ksk)
    handles = [e.multibit_key(words, g), e_small.multibit_key(words, g), e.lut(tv), e_small.lut(tv)]
    key, key_small, lut, lut_small = handles
    try:
        st = lk._stream()
        keys_only = e_small.memory_bytes()
        d_ct = lk.device_words(count * w1, 0x4D4C03 + N)
        d_idx = torch.randint(0, 3, (count,), dtype=torch.int32, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0x4D4C04 + N))
        bad = seg + np.array([0, 7, 500, 1000, 1060])
        d_idx[torch.from_numpy(bad).cuda()] = gk.to_device(np.array(BAD_IDX))
        d_out = lk.guarded_device(count * w1)
        e.timer_begin(st)
        e.pbs_mb_batch_dev(key, lut, d_ct, d_out, count, d_idx, st)
        detail = e.timer_end_detail(st)
        with pytest.raises(R.RtfheError) as ei:
            e.sync(st)
        assert ei.value.code == R._ffi.ERR_INVALID
        e.sync(st)                                   # reported once
        lk._split_path_taken(e, detail, count, N, label, keys_only)

        fill = int(np.uint32(gk.FILL).view(np.int32))
        raised = []

        def call(s, d_chunk, cnt):
            d_chunk[:cnt * w1].fill_(fill)           # the buffer is reused: a skipped gate's row must find the fill, as in the big call
            e_small.pbs_mb_batch_dev(key_small, lut_small, s[0], d_chunk, cnt, s[1], st)
            try:
                e_small.sync(st)
            except R.RtfheError as err:
                assert err.code == R._ffi.ERR_INVALID
                raised.append(cnt)
        chunk = lk._chunk_samples(N)
        lk.same_as_chunks(call, [(d_ct, w1), (d_idx, 1)], (d_out, w1), count, chunk)
        assert len(raised) == len({int(b) // chunk for b in bad}), "exactly the slices with a skipped gate reported one"
        assert e_small.memory_bytes() - keys_only <= 1 << 30, "the slice calls' sample buffer stayed below 2^30 bytes"

        pick = np.unique(np.concatenate([lk.probe_items(count, (N + 1) * 4, seg), bad - 1, bad, bad + 1]))
        pick = pick[pick < count]                    # (the last skipped gate is the call's last)
        assert pick.min() >= 0 and pick.max() == count - 1
        good = ~np.isin(pick, bad)
        got = lk.rows_of(d_out, w1, pick)
        assert (got[~good] == gk.FILL).all(), "a skipped gate's row keeps the fill"
        gp = pick[good]
        ct, idx = lk.rows_of(d_ct, w1, gp), lk.rows_of(d_idx, 1, gp).view(np.int32).reshape(-1)
        exp = np.stack([mo.pbs_mb(P, plan, tab, key_f, K.ksk, tv[idx[k]], ct[k], g) for k in range(len(gp))])
        diff = np.flatnonzero((got[good] != exp).any(axis=1))
        assert diff.size == 0, ("gates that differ from the oracle", gp[diff][:16].tolist())
        lk.check_canary(d_out, count * w1)
        torch.cuda.synchronize()
    finally:
        for h in handles + [e, e_small]:
            h.close()
        d_ct = d_idx = d_out = None
        lk.release()


def test_pbs_mb_workgroup_shape_two_key_switch_segments_n1024(orc, monkeypatch):
    """523,776 + 1,061 gates at N = 1024 in the default shape, a workgroup per gate: a grid of 524,837 workgroups, 2.15 GB of samples"""
    _pbs_mb(orc, monkeypatch, 1024, 523776 + 1061, None, "pbs_mb_batch_dev wg N=1024")


def test_pbs_mb_wave_shape_two_key_switch_segments_n1024(orc, monkeypatch):
    """the same count under RTFHE_MB_SHAPE=wave: gate numbers blockIdx.x * 4 + wave, the last workgroup with one live wave"""
    _pbs_mb(orc, monkeypatch, 1024, 523776 + 1061, "wave", "pbs_mb_batch_dev wave N=1024")


def test_pbs_mb_wave_shape_two_key_switch_segments_n2048(orc, monkeypatch):
    """261,632 + 1,061 gates at N = 2048 (the wave shape): the same span in tiles of 131,136 bytes"""
    _pbs_mb(orc, monkeypatch, 2048, 261632 + 1061, "wave", "pbs_mb_batch_dev wave N=2048")
