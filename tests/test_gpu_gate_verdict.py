"""GPU tests of the carrier gate's verdict (k_gate_verdict behind the detectors' carrier stage) against
a float64 restatement of cardet (fastcard/cardet.c:7-41) written out here, with
oracle.OracleFastdet's float32 restatement as the second opinion.

The set of passed blocks must equal the oracle's for every block with |max - thr| > 1e-4 * thr: five
times the 2e-5 relative that DESIGN.md section 4 asserts for float32 energies (`max` and `noise` each
carry one).  The tests assert FROM THE ORACLE, BEFORE THE GPU IS ASKED, that no block of the input lies
inside that margin: with c = 0 and s = the geometric mean of the largest max/noise among the tone-free
blocks and the smallest among the tone blocks (asserted to be at least a factor 4 apart), and once
with `1000c2s`.  Window `0--1` is not a verdict case on this data -- the u8 quantiser leaves a DC line
above most tones -- and is its own exact case below.
"""
import math

import numpy as np
import pytest

from oracle import thrifty_np as onp
from thrifty_amd import _native as F
from thrifty_amd import block_data, fastcard, synth

pytestmark = pytest.mark.gpu

MARGIN = 1e-4
N_BLOCKS = 4096


def cardet64(blocks, window, chunk=128):
    """cardet_detect's quantities in float64 for u8 blocks [B, 2N]: (sum, max, argmax, noise, second
    largest window power)."""
    n = blocks.shape[1] // 2
    lo, hi = fastcard.normalize_window(window[0], window[1], n)
    total, mx, arg, second = (np.empty(len(blocks)) for _ in range(4))
    for a in range(0, len(blocks), chunk):
        v = (blocks[a:a + chunk].astype(np.float64) - 127.4) / 128.0
        power = np.abs(np.fft.fft(v[:, 0::2] + 1j * v[:, 1::2], axis=1)) ** 2
        total[a:a + chunk] = power.sum(axis=1)
        w = power[:, lo:hi + 1]
        k = np.argmax(w, axis=1)                                  # the first maximum
        arg[a:a + chunk] = k + lo
        mx[a:a + chunk] = w[np.arange(len(w)), k]
        if w.shape[1] > 1:
            second[a:a + chunk] = np.partition(w, -2, axis=1)[:, -2]
        else:
            second[a:a + chunk] = 0.0
    noise = np.where(total != 0, (total - 2 * mx) / (n - 1), 0.0)
    return total, mx, arg.astype(np.int64), noise, second


_DATA = {}


def _data(n, h, seed=1):
    key = (n, h, seed)
    if key not in _DATA:
        _DATA.clear()                                             # (one geometry's blocks in memory at a time)
        tpl = synth.gold_template(10, 2)                          # the 1023-chip Gold template
        assert len(tpl) == 1023
        rng = np.random.default_rng(seed)
        blocks, truth = synth.synth_blocks(rng, N_BLOCKS, n, tpl, onp.unique_window(n, h, len(tpl)), signal_frac=0.1)
        _DATA[key] = (tpl, blocks, truth["has_signal"])
    return _DATA[key]


def _check(n, h, window, thresholds):
    tpl, blocks, has = _data(n, h)
    total, mx, arg, noise, second = cardet64(blocks, window)
    ratio = mx / noise
    top_free, low_tone = ratio[~has].max(), ratio[has].min()
    print("block %d window %s: %d tone blocks; max/noise tone-free <= %.2f, tone >= %.2f (factor %.1f); "
          "noise power per bin %.2f" % (n, window, has.sum(), top_free, low_tone, low_tone / top_free,
                                        np.median(noise)))
    assert has.sum() >= 100 and low_tone >= 4 * top_free
    for thr_c, thr_s in thresholds:
        if thr_s is None:
            thr_s = math.sqrt(top_free * low_tone)
        c32, s32 = float(np.float32(thr_c)), float(np.float32(thr_s))
        thr = c32 + s32 * noise
        want = mx > thr
        # ---- conditions, from the oracle, before the GPU is asked
        gap = np.abs(mx - thr) / thr
        print("  threshold %gc%gs: %d pass; closest block at %.3g of its threshold" % (c32, s32, want.sum(), gap.min()))
        assert gap.min() > MARGIN, "a block lies inside the verdict margin"
        assert np.array_equal(want, has)
        # near-tie condition of the bin check: the carrier stage takes the first maximum of the float32
        # MAGNITUDE, cardet of the power, so the bins are compared where the oracle's two largest window
        # powers differ by more than 1e-5 relative.  The OOK burst's main lobe is 16 (block 16384) to 64
        # (block 65536) bins wide and nearly flat at its top, so among some 400 tone blocks a few such
        # near-ties are expected whatever the seed (block 16384, seed 1, 4096 blocks: at least one); those
        # blocks are set apart and must report a bin whose oracle power is within 1e-5 of the maximum.
        tie = want & ((mx - second) <= 1e-5 * mx)
        clear = want & ~tie
        print("  near-ties among the passed blocks: %d of %d" % (tie.sum(), want.sum()))
        assert tie.sum() <= 0.01 * want.sum()      # (a kernel that picks neighbour bins on flat lobes cannot hide here)
        # ---- second opinion: the float32 restatement
        orc = onp.OracleFastdet(n, h, tpl, (c32, s32, 0), window, (1e30, 0, 0))
        res = [orc.detect_u8(i, blocks[i]) for i in range(len(blocks))]
        assert np.array_equal(np.array([r.carrier for r in res]), want)
        assert np.array_equal(np.array([r.argmax for r in res])[clear], arg[clear])
        np.testing.assert_allclose(np.array([r.carrier_max for r in res], dtype=np.float64), mx, rtol=2e-5)
        # ---- the engine
        eng = F.Engine.gate(n, h, window, (c32, s32), max_batch=2048)
        assert eng.path_info()["carrier_kernel"] == KERNELS[(n, window)]
        rec, k, slots = eng.gate_blocks(blocks)
        eng.close()
        got = (rec["flags"] & F.FLAG_CARRIER) != 0
        assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
        assert k == want.sum() and np.all(rec["flags"] & ~np.uint32(F.FLAG_CARRIER) == 0)
        p = np.flatnonzero(want)
        assert np.array_equal(rec["carrier_bin"][clear], arg[clear])
        for i in np.flatnonzero(tie):
            v = (blocks[i].astype(np.float64) - 127.4) / 128.0
            power = np.abs(np.fft.fft(v[0::2] + 1j * v[1::2])) ** 2
            lo, hi = fastcard.normalize_window(window[0], window[1], n)
            assert lo <= rec["carrier_bin"][i] <= hi and power[rec["carrier_bin"][i]] >= mx[i] * (1 - 1e-5), i
        np.testing.assert_allclose(rec["carrier_energy"][p], np.sqrt(mx[p]), rtol=2e-5)
        np.testing.assert_allclose(rec["carrier_noise"][p], np.sqrt(noise[p]), rtol=2e-5)
        np.testing.assert_allclose(rec["reserved"][p].astype(np.uint32).view(np.float32), thr[p], rtol=2e-5)
        np.testing.assert_allclose(rec["carrier_energy"][p], [math.sqrt(res[i].carrier_max) for i in p], rtol=2e-5)
        np.testing.assert_allclose(rec["carrier_noise"][p], [math.sqrt(res[i].carrier_noise) for i in p], rtol=2e-5)
        # the slots are the passed blocks, in order
        stride, chars = F.gate_slot_stride(n), F.gate_payload_chars(n)
        for s in (0, len(p) // 2, len(p) - 1):
            assert slots[s * stride:s * stride + chars].tobytes() == block_data.card_line(0, 0, blocks[p[s]]).split(" ")[2][:-1].encode()


KERNELS = {(16384, (1, -1)): "k_carrier", (16384, (7, 110)): "k_carrier_pruned",
           (4096, (1, -1)): "k_carrier_small", (65536, (7, 110)): "k_carrier_dit+k_select_dit"}


@pytest.mark.parametrize("window", [(1, -1), (7, 110)])
def test_verdict_block_16384(window):
    _check(16384, 4920, window, [(0.0, None), (1000.0, 2.0)])


def test_verdict_block_4096():
    _check(4096, 1230, (1, -1), [(0.0, None)])


def test_verdict_block_65536():
    _check(65536, 4920, (7, 110), [(0.0, None)])


def test_window_0_to_minus_1_the_dc_line_passes_every_block():
    """With bin 0 in the window and s = 100 every block passes (the quantiser's DC line: max/noise about
    770), and the tone-free ones report carrier_bin == 0."""
    n, h = 16384, 4920
    tpl, blocks, has = _data(n, h)
    blocks, has = blocks[:512], has[:512]
    total, mx, arg, noise, _ = cardet64(blocks, (0, -1))
    assert np.all(mx > 100 * noise * (1 + MARGIN)) and np.all(arg[~has] == 0)
    eng = F.Engine.gate(n, h, (0, -1), (0.0, 100.0), max_batch=512)
    rec, k, _ = eng.gate_blocks(blocks)
    eng.close()
    assert k == 512 and np.all(rec["flags"] == F.FLAG_CARRIER)
    assert np.all(rec["carrier_bin"][~has] == 0)


def _tone(n, bin_, amp=0.4):
    return block_data.complex_to_raw(amp * np.exp(2j * np.pi * bin_ * np.arange(n) / n))


@pytest.mark.parametrize("n, window", [(16384, (7, 110)), (16384, (200, 5000)), (16384, (-300, -20)), (16384, (5000, 5100)), (4096, (110, 7)),
                                       (2048, (-2000, -100)), (32768, (7, 110)), (512, (7, 110))])
def test_window_ends(n, window):
    """A tone exactly at min, at max, and one bin outside either; windows given with negative ends."""
    lo, hi = fastcard.normalize_window(window[0], window[1], n)
    bins = [lo, hi, lo - 1, hi + 1, (lo + hi) // 2]
    blocks = np.stack([_tone(n, b) for b in bins])
    total, mx, arg, noise, second = cardet64(blocks, window)
    thr = 0.25 * (0.4 * n) ** 2                      # a quarter of the tone's power: in-window tones only
    gap = np.abs(mx - thr) / thr
    assert gap.min() > MARGIN and (mx > thr).tolist() == [True, True, False, False, True]
    eng = F.Engine.gate(n, 0, window, (thr, 0.0), max_batch=8)
    rec, k, _ = eng.gate_blocks(blocks)
    eng.close()
    assert ((rec["flags"] & F.FLAG_CARRIER) != 0).tolist() == [True, True, False, False, True] and k == 3
    assert rec["carrier_bin"][[0, 1, 4]].tolist() == [lo, hi, (lo + hi) // 2] == arg[[0, 1, 4]].tolist()
    np.testing.assert_allclose(rec["carrier_energy"][[0, 1, 4]], np.sqrt(mx[[0, 1, 4]]), rtol=2e-5)


def test_refused_window_raises():
    for win in ((-5, 10), (-1, 0), (0, 16384), (16384, 3)):
        with pytest.raises(F.NativeError, match="window"):
            F.Engine.gate(16384, 4920, win, (100.0, 2.0))
    with pytest.raises(F.NativeError, match="stddev"):
        lib = F.load_library()
        st = F.ThrSettings()
        st.block_len, st.history_len, st.max_batch = 16384, 4920, 8
        st.carrier_window[0], st.carrier_window[1] = 0, -1
        st.carrier_thresh[2] = 1.0
        import ctypes as C
        handle = C.c_void_p()
        F._check(lib, lib.thr_create_ex(C.byref(st), F.VARIANT_GATE, 0, 0, C.byref(handle)))
