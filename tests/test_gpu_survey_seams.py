"""The capture survey's kernels and chunk loop (survey.hip) at the seams tests/test_gpu_survey.py
does not reach, against tests/survey_ref.py: one call cut into several chunks with the open interval carried
from chunk to chunk (also across three chunks), K = 1 and K = the tile, the fold path at every kind of length
from 64 to 2^20 and on raw streams, strides that are multiples of 4 only, the spectrum of constant blocks, and
cap_intervals at the exact fit.

Row assignment is decided without a tolerance on survey_ref.signature_blocks: the K largest bins of a completed
row are the tone bins of that row's blocks, and hist / sums / the row count are those of np.bincount.  On top of
that every checked row meets test_gpu_survey.spectrum_bound against the float64 oracle, and every cut equals,
bit for bit, the same blocks fed one at a time.

max_batch = 8 gives chunk_max = 8 (7 at K = 1, where the 8 rows a chunk may touch include the open one), so 29
blocks are four chunks.  Open blocks at each chunk's start, from survey_create_body, for a call on an empty
survey (a call behind f open blocks shifts them by f):
    K = 3: 0 2 1 0    K = 4 and 8: 0 0 0 0    K = 5: 0 3 1 4    K = 20 (45 blocks): 0 8 16 4 12 0
    K = 1: 0 0 0 (20 blocks as 7 + 7 + 6; 1030 blocks on max_batch 8192 as 511 + 511 + 8: 512 rows in 64 MiB;
    16 blocks of 2^20 on max_batch 64 as 7 + 7 + 2: 8 rows in 64 MiB)

Measured (MI355X), largest rel-L2 of a row's mean spectrum against the float64 oracle per length (bounds 5.0e-6
... 6.4e-6), signature blocks: 64 1.04e-7, 512 8.4e-8, 1024 1.23e-7, 2048 1.47e-7, 8192 1.28e-7, 16384 2.47e-7 fused
and 1.49e-7 multipass, 32768 2.02e-7, 131072 3.09e-7, 2^20 8.63e-7; the stream at 65536 1.71e-7; constant blocks at
most 1.30e-7 (all-127).  No length needed a bound of its own.  Every case prints its figure before it asserts
(pytest -s).  The two longest cases: 2^20 1.4 s, 1030 blocks 0.8 s."""
import contextlib
import mmap

import numpy as np
import pytest

import survey_ref
from test_gpu_survey import byte_ref, make, mean_mag, rel_l2, spectrum_bound
from thrifty_amd import _native

pytestmark = pytest.mark.gpu

N = 16384
FOLD_LENGTHS = [64, 512, 1024, 2048, 8192, 32768, 131072]


@contextlib.contextmanager
def survey_on(n, k, h=0, max_batch=8, path="auto"):
    """a Survey on a gate engine of its own; the fused kernel exactly where DESIGN.md 3.11 says"""
    e = _native.Engine.gate(n, h, max_batch=max_batch, path=path)
    try:
        with _native.Survey(e, k) as s:
            assert s.geometry()[2] is (n == N and path == "auto") and s.shift == 30 - int(np.log2(n))
            yield e, s
    finally:
        e.close()


def joined(parts):
    return [np.concatenate([p[i] for p in parts]) for i in range(3)]


def one_at_a_time(s, blocks):
    s.reset()
    return joined([s.feed(blocks[i:i + 1]) for i in range(len(blocks))])


def same_bits(got, want):
    return all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(got, want))


def ref_row(blocks, j, k):
    """the float64 mean spectrum of interval j"""
    return survey_ref.survey(blocks[j * k:(j + 1) * k], k)[0][0]


def meets_the_statement(got, blocks, k, shift, rows=None, signature=True, refs=None):
    """hist, sums and the row count exactly; the K largest bins of every row are that row's tone bins; on `rows`
    (default: all) the mean spectrum is inside spectrum_bound.  -> (the largest rel-L2, the rows outside)"""
    spec, hist, sums = got
    n = blocks.shape[1] // 2
    want_hist, want_sums = byte_ref(blocks, k)
    assert spec.shape == (len(blocks) // k, n) and np.array_equal(hist, want_hist) and np.array_equal(sums, want_sums)
    worst, late = 0.0, []
    for j in range(len(spec) if signature else 0):
        assert survey_ref.top_bins(spec[j], k) == survey_ref.tone_bins(j, k, n), (n, k, j)
    for j in (range(len(spec)) if rows is None else rows):
        ref = ref_row(blocks, j, k) if refs is None else refs[j]
        err, bound = rel_l2(mean_mag(spec[j], shift, k), ref), spectrum_bound(shift, n, ref)
        worst = max(worst, err)
        if err > bound:
            late.append((j, err, bound))
    return worst, late


# ------------------------------------------------------------------ a. one call cut into chunks
def cut_call_case(n, k, nb, max_batch=8, path="auto", rows=None):
    scene = survey_ref.signature_blocks(nb + k - 1, n, seed=n + k)
    with survey_on(n, k, max_batch=max_batch, path=path) as (e, s):
        ones = one_at_a_time(s, scene)
        assert s.pending() == (len(scene), len(scene) % k)
        refs = {j: ref_row(scene, j, k) for j in (range(len(scene) // k) if rows is None else rows)}
        worst, late = meets_the_statement(ones, scene, k, s.shift, rows, refs=refs)
        for front in range(k):      # the big call's chunks start behind front, front + 8, ... blocks
            s.reset()
            parts = []
            if front:
                parts.append(s.feed(scene[:front]))
                assert s.pending() == (front, front) and len(parts[0][0]) == 0
            parts.append(s.feed(scene[front:front + nb]))
            assert s.pending() == (front + nb, (front + nb) % k)
            got = joined(parts)
            done = (front + nb) // k
            assert same_bits(got, (ones[0][:done], ones[1][:done], ones[2][:front + nb])), (n, k, front)
            if front == 0:
                w, l = meets_the_statement(got, scene[:nb], k, s.shift, None if rows is None else
                                           [j for j in rows if j < done], refs=refs)
                worst, late = max(worst, w), late + l
        shift = s.shift
    print("survey seams n=%d %s K=%d, %d blocks in chunks: largest rel-L2 %.3e (bound %.3e)"
          % (n, path, k, nb, worst, spectrum_bound(shift, n, refs[min(refs)])))
    assert not late, late


@pytest.mark.parametrize("k,nb", [(4, 29), (3, 29), (8, 29), (20, 45), (1, 20)])
def test_a_fused_call_in_chunks_is_the_oracle_and_its_blocks_one_at_a_time(k, nb):
    """k_survey16k through survey_run's chunk loop: K = 4 and K = 8 = the tile close rows on chunk ends, K = 3
    carries 2 and 1 open blocks, K = 20 carries one interval over three chunks (row 0 stays row 0 twice), K = 1
    closes a row per block and carries nothing"""
    cut_call_case(N, k, nb)


@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("n", FOLD_LENGTHS)
def test_a_fold_call_in_chunks_is_the_oracle_and_its_blocks_one_at_a_time(n, k):
    """k_survey_fold and k_survey_bytes behind the generic (64, 512, 131072), the small (1024, 2048, 8192) and the
    long (32768) carrier stage; 64 is the one length with the fold's k >= n guard and fewer than 256 words"""
    cut_call_case(n, k, 29)


def test_a_multipass_call_in_chunks_is_the_oracle_and_its_blocks_one_at_a_time():
    cut_call_case(N, 3, 29, path="multipass")


def test_k_1_at_the_accumulator_budget_1030_blocks_in_511_511_8():
    """64 MiB of uint64[16384] rows are 512 rows: chunks of 511 blocks.  Bytes and the tone bin on every row, the
    oracle on the rows around both chunk seams and at both ends"""
    cut_call_case(N, 1, 1030, max_batch=8192, rows=[0, 510, 511, 512, 1021, 1022, 1029])


def test_k_1_at_two_to_the_twenty_16_blocks_in_7_7_2():
    """8 rows of uint64[2^20] fill the 64 MiB: chunk_max = 7"""
    cut_call_case(1 << 20, 1, 16, max_batch=64)


# ------------------------------------------------------------------ b. streams
STREAMS = [(1024, 126, False), (1024, 132, False), (64, 62, False), (65536, 4922, False), (65536, 4922, True),
           (N, 4922, False), (N, 4922, True), (N, 16382, False)]


@pytest.mark.parametrize("n,h,windowed", STREAMS)
def test_a_stream_in_chunks_is_its_framed_blocks(n, h, windowed):
    """feed_stream over four chunks (src + done * step, bytes = (nb - 1) * step + blk) on the fold path and on
    the fused kernel, at strides 1796, 1784, 121228 and 22924 (multiples of 4, none of 16) and 4 (blocks two
    samples apart: history bytes count in both blocks), also through the input window in 64 KiB segments"""
    k, nb = 3, 29
    step = 2 * (n - h)
    assert step % 4 == 0 and step % 16 != 0
    stream = make("tone", 1, n=((nb - 1) * step + 2 * n) // 2, seed=n + h).ravel()
    blocks = survey_ref.blocks_of(stream, n, h)
    assert len(blocks) == nb and len(stream) == (nb - 1) * step + 2 * n
    with survey_on(n, k, h=h) as (e, s):
        want = s.feed(blocks)
        assert s.pending() == (nb, nb % k)
        s.reset()
        if windowed:
            # a mapping of its own, as thr_input_window asks for (the mmap of the input file): the window
            # page-locks whole pages, and a copy into a result array that began in the stream's last page
            # would be refused (a heap array's last page can hold the next allocation)
            pinned = np.frombuffer(mmap.mmap(-1, len(stream)), dtype=np.uint8)
            pinned[:] = stream
            assert pinned.ctypes.data % 4096 == 0 and 7 * step + 2 * n > (1 << 16)      # a chunk crosses a segment
            e.input_window(pinned, segment_bytes=1 << 16)
            try:
                got = s.feed_stream(pinned)
            finally:
                e.input_window(None)
        else:
            got = s.feed_stream(stream)
        assert s.pending() == (nb, nb % k)
        shift = s.shift
    assert same_bits(got, want)
    worst, late = meets_the_statement(got, blocks, k, shift, signature=False)
    print("survey seams stream n=%d H=%d (stride %d): largest rel-L2 %.3e" % (n, h, step, worst))
    assert not late, late


# ------------------------------------------------------------------ c. constant blocks
@pytest.mark.parametrize("value", [0, 127, 128, 255])
@pytest.mark.parametrize("n", [N, 1024])
def test_the_spectrum_of_constant_blocks(n, value):
    """all-0 holds the largest q the format is specified for: |X[0]| = 1.4076 N, q = 1.511e9 > 2^30"""
    k = 4
    blocks = np.full((2 * k, 2 * n), value, dtype=np.uint8)
    with survey_on(n, k) as (e, s):
        got = s.feed(blocks)
        shift = s.shift
    worst, late = meets_the_statement(got, blocks, k, shift, signature=False)
    print("survey seams constant %d n=%d: largest rel-L2 %.3e" % (value, n, worst))
    assert not late, late
    x0 = n * np.sqrt(2.0) * abs(value - float(np.float32(127.4))) / 128.0
    for j in range(2):
        q0 = int(got[0][j][0])
        assert int(got[0][j].argmax()) == 0
        if value == 0:
            assert q0 > k * 2 ** 30
            assert abs(q0 - k * 2.0 ** shift * x0) <= k * (0.5 + 5e-6 * 2.0 ** shift * x0), (q0, k * 2.0 ** shift * x0)


# ------------------------------------------------------------------ e. cap_intervals at the exact fit
@pytest.mark.parametrize("n", [N, 1024])
@pytest.mark.parametrize("nb", [5, 13])
def test_cap_intervals_at_the_exact_fit_behind_an_open_interval(n, nb):
    """3 open blocks and nb more complete (3 + nb) / 4 intervals: room for exactly that many is enough, room for
    one fewer is refused before anything runs (13 blocks would be two chunks)"""
    k = 4
    scene = survey_ref.signature_blocks(3 + nb, n, seed=nb)
    fit = (3 + nb) // k
    with survey_on(n, k) as (e, s):
        first = s.feed(scene[:3])
        assert s.pending() == (3, 3)
        with pytest.raises(_native.NativeError) as err:
            s.feed(scene[3:], cap_intervals=fit - 1)
        assert "(code %d)" % _native.ERR_ARG in str(err.value) and "room for %d" % (fit - 1) in str(err.value)
        assert s.pending() == (3, 3)
        more = s.feed(scene[3:], cap_intervals=fit)
        assert len(more[0]) == fit and s.pending() == (3 + nb, (3 + nb) % k)
        shift = s.shift
    worst, late = meets_the_statement(joined([first, more]), scene, k, shift)
    assert not late, late
