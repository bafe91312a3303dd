"""A handle owns what it takes from the HIP runtime: thr_debug_live_resources -- the library's own count of
its live device buffers, pinned buffers, streams and events -- is back where it started once the handle is
closed, for every handle shape and after every entry point that allocates lazily has run.  (The count is the
library's, not the device's free memory: other processes share the device.)

One case per shape: create, drive every entry point the shape accepts over 16 blocks in batches of 8, see the
counts above the start, close, see them AT the start -- twice in the same process, so that the second handle
meets the kernels the first one prepared."""
import gc

import numpy as np
import pytest

import postdetect_scene as scene
from thrifty_amd import _native as F
from thrifty_amd import block_data, kitchen_sink, synth

pytestmark = pytest.mark.gpu

MAX_BATCH, BLOCKS = 8, 16

# name -> (block_len, history_len, gold-code bits, templates, Engine keywords)
SHAPES = {
    "16384 sectioned, one template": (16384, 4096, 10, 1, {}),
    "16384 sectioned, four templates": (16384, 4096, 10, 4, {}),
    "16384 unsectioned": (16384, 4096, 10, 1, dict(path="unsectioned")),
    "32768 sectioned": (32768, 4096, 11, 1, {}),
    "65536 unsectioned": (65536, 4096, 11, 1, dict(path="unsectioned")),
    "1024 small": (1024, 256, 7, 1, {}),
    "512 generic": (512, 128, 6, 1, {}),
    "2048 multipass": (2048, 512, 8, 1, dict(path="multipass")),
    "preshift 16384": (16384, 4096, 10, 1, dict(preshift_num=8)),
    "preshift 4096": (4096, 1024, 9, 1, dict(preshift_num=8)),
    "fastdet": (16384, 4096, 10, 1, dict(fastdet=True)),
}
EXPECTED_PATH = {      # (sections, section length) of thr_debug_sections: the shape is the one the case names
    "16384 sectioned, one template": (4, 4096), "16384 sectioned, four templates": (4, 4096),
    "16384 unsectioned": (0, 0), "32768 sectioned": (3, 16384), "65536 unsectioned": (0, 0),
}


def inputs(n, h, templates):
    """16 blocks with a burst in every other one, as dense blocks, as .card text + offsets and as a raw stream."""
    rng = np.random.default_rng(n)
    w = templates.shape[1]
    blocks, _ = synth.synth_blocks(rng, BLOCKS, n, templates[0], (h - w + 1, n - w), signal_frac=0.5,
                                   carrier_bins=(20.0, 60.0))
    text = "".join(block_data.card_line(100.0 + i, i, blocks[i]) for i in range(BLOCKS)).encode()
    _, _, off, _ = F.frame_card(text, 0, len(text), n, True, BLOCKS)
    assert len(off) == BLOCKS
    stream = np.ascontiguousarray(blocks[:, :2 * (n - h)]).reshape(-1)       # 15 whole overlapping blocks
    return blocks, text, off, stream


def drive_detector(eng, blocks, text, off, stream, dumps, offsets):
    import torch
    nt = eng.n_templates
    assert eng.detect(blocks).shape == (BLOCKS, nt)
    assert eng.detect_card(text, off).shape == (BLOCKS, nt)
    assert len(eng.detect_stream(stream)) == BLOCKS - 1
    tickets = [eng.submit(blocks[:MAX_BATCH]), eng.submit(blocks[MAX_BATCH:])]
    for t in tickets:
        assert eng.collect(t).shape == (MAX_BATCH, nt)
    if dumps:             # (the fused 16384 kernel of the preshift and fastdet variants has no stage dumps)
        assert eng.debug_fft(blocks[:MAX_BATCH]).shape == (MAX_BATCH, eng.block_len)
        eng.debug_stage(blocks[:MAX_BATCH], template_id=nt - 1)
    if offsets:           # (those variants interpolate the carrier themselves: the default detector only)
        eng.debug_stage(blocks[:MAX_BATCH], carrier_offset=np.full(MAX_BATCH, 0.25))
        assert eng.detect_offsets(blocks[:MAX_BATCH], np.full(MAX_BATCH, 0.25)).shape == (MAX_BATCH, nt)
    dev = torch.device("cuda:0")
    for n_rec in (300, 5000):         # (the tile array grows once)
        rec = np.zeros(n_rec, dtype=F.RECORD_DTYPE)
        d_in = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to(dev)
        d_out = torch.zeros_like(d_in)
        torch.cuda.synchronize()
        assert eng.compact_device(d_in.data_ptr(), n_rec, d_out.data_ptr()) == 0


def lifecycle(make, use):
    for _ in range(2):
        gc.collect()      # (an engine an earlier test dropped without close() goes now, not in the middle of the case)
        start = F.live_resources()
        eng = make()
        try:
            created = F.live_resources()
            assert created[0] > start[0] and created[2] == start[2] + 1, (start, created)
            use(eng)
            alive = F.live_resources()
            assert all(a >= c for a, c in zip(alive, created)) and sum(alive) > sum(created), (created, alive)
        finally:
            eng.close()
        assert F.live_resources() == start


@pytest.mark.parametrize("name", list(SHAPES))
def test_a_detector_handle_gives_back_all_it_took(name):
    n, h, bits, nt, kw = SHAPES[name]
    templates = np.stack([synth.gold_template(bits, k) for k in range(nt)])
    data = inputs(n, h, templates)
    variant = bool(kw.get("fastdet") or kw.get("preshift_num"))
    thresh = dict(carrier_thresh=(0.0, 8.0, 0.0), corr_thresh=(0.0, 10.0, 0.0), carrier_window=(5, 200))

    def make():
        eng = F.Engine(n, h, templates, max_batch=MAX_BATCH, **thresh, **kw)
        if name in EXPECTED_PATH:
            assert eng.sections() == EXPECTED_PATH[name], eng.path_info()
        return eng

    lifecycle(make, lambda eng: drive_detector(eng, *data, dumps=not (variant and n == 16384), offsets=not variant))


@pytest.mark.parametrize("n", [16384, 32768])
def test_a_gate_handle_gives_back_all_it_took(n):
    h = 4096
    blocks, text, off, stream = inputs(n, h, synth.gold_template(10, 0)[None, :])

    def use(eng):
        assert len(eng.gate_blocks(blocks)[0]) == BLOCKS
        assert len(eng.gate_stream(stream)[0]) == BLOCKS - 1
        assert len(eng.gate_card(text, off)[0]) == BLOCKS

    lifecycle(lambda: F.Engine.gate(n, h, window=(5, 200), max_batch=MAX_BATCH), use)


def test_an_extraction_gives_back_all_it_took_and_its_engine_the_rest():
    n, h = 16384, 4096
    template = synth.gold_template(10, 0)
    blocks, _, _, _ = inputs(n, h, template[None, :])

    def use(eng):
        before = F.live_resources()
        x = F.Extraction(eng, max_offset=0.5)
        took = np.subtract(F.live_resources(), before)
        assert took[0] > 0 and took[1] > 0 and took[2] == took[3] == 0, took
        x.feed(blocks, timestamps=np.arange(BLOCKS, dtype=np.float64))
        _, _, cut, qualifying = x.result(len(template))
        assert qualifying > 0 and cut.shape == template.shape
        alive = F.live_resources()
        x.close()         # (the feed grew the ENGINE's pipeline; the extraction gives back what it took itself)
        assert np.array_equal(np.subtract(alive, F.live_resources()), took)

    lifecycle(lambda: F.Engine(n, h, template, (0.0, 8.0, 0.0), (5, 200), (0.0, 10.0, 0.0), max_batch=MAX_BATCH), use)


def test_postdetect_gives_back_all_it_took():
    cols, st = scene.columns(60), scene.settings()
    for _ in range(2):
        gc.collect()
        start = F.live_resources()
        got = kitchen_sink.postdetect_columns(cols, st)          # (thr_postdetect, the fetches, thr_post_free)
        assert got["counts"]["kept"] > 0
        assert F.live_resources() == start
