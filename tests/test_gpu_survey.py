"""The capture survey on the device (thr_survey_*, thrifty_amd.survey) against tests/survey_ref.py: byte
statistics exactly, the spectrum within the transform's asserted bound plus the quantisation of q, every cut
of a run bit for bit, and the fused 16384 kernel against the fold path on the multi-pass handle.

Measured (MI355X), rel-L2 of mean_mag against the float64 oracle, largest interval: 9.0e-8 (noise + tone) and
1.53e-6 (bytes 126..129) against bounds of 5.2e-6 and 1.0e-5; fold path 7.2e-8 at 1024 and 1.7e-7 at 65536; fused
against fold 5.3e-7.  Every case prints its figure before it asserts (pytest -s)."""
import io
import mmap
import os
import subprocess
import sys

import numpy as np
import pytest

import survey_ref
from thrifty_amd import _native, survey

pytestmark = pytest.mark.gpu

N = 16384
K = 4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def byte_ref(blocks, k):
    """(hist uint64 [J, 256], sums uint64 [B, 2]) from one np.bincount per block"""
    blocks = np.asarray(blocks, dtype=np.uint8)
    per_block = np.stack([np.bincount(b, minlength=256) for b in blocks]).astype(np.uint64)
    v = np.arange(256, dtype=np.uint64)
    sums = np.stack([per_block @ v, per_block @ (v * v)], axis=1)
    n_int = len(blocks) // k
    hist = per_block[:n_int * k].reshape(n_int, k, 256).sum(axis=1) if n_int else np.zeros((0, 256), np.uint64)
    return hist, sums


def make(kind, nb, n=N, seed=3):
    rng = np.random.default_rng(seed)
    total = nb * 2 * n
    if kind == "uniform":
        flat = rng.integers(0, 256, total).astype(np.uint8)
    elif kind in ("all127", "all0", "all255"):
        flat = np.full(total, int(kind[3:]), np.uint8)
    elif kind == "narrow":
        flat = rng.integers(126, 130, total).astype(np.uint8)
    elif kind == "mod251":
        flat = np.resize(np.arange(251, dtype=np.uint8), total)
    elif kind == "tone":      # noise of 10 LSB and a tone on bin 1234
        t = np.arange(nb * n, dtype=np.float64) % n
        z = 40.0 * np.exp(2j * np.pi * 1234 * t / n)
        iq = np.stack([z.real, z.imag], axis=1).ravel() + 10.0 * rng.standard_normal(total) + 127.4
        flat = np.clip(np.rint(iq), 0, 255).astype(np.uint8)
    else:
        raise ValueError(kind)
    return flat.reshape(nb, 2 * n)


@pytest.fixture(scope="module")
def eng():
    e = _native.Engine.gate(N, 0, max_batch=8192)
    yield e
    e.close()


@pytest.fixture(scope="module")
def sv(eng):
    s = _native.Survey(eng, K)
    yield s
    s.close()


@pytest.fixture(scope="module")
def eng_multipass():
    e = _native.Engine.gate(N, 0, max_batch=64, path="multipass")
    yield e
    e.close()


@pytest.fixture(scope="module")
def oracle():
    """the two spectrum inputs, 2 K blocks each, with the float64 reference (computed once)"""
    out = {}
    for kind in ("tone", "narrow"):
        blocks = make(kind, 2 * K, seed=17)
        out[kind] = (blocks,) + survey_ref.survey(blocks, K)
    return out


def spectrum_bound(shift, n, ref_row):
    """DESIGN.md section 4's asserted stage-dump bound (the same transform) plus what rounding |X| 2^S to an
    integer can add: half a step per bin, sqrt(n) of them in the L2 norm"""
    return 5e-6 + 2.0 ** -(shift + 1) * np.sqrt(n) / np.linalg.norm(ref_row)


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def mean_mag(spec, shift, k):
    return spec.astype(np.float64) / (k * 2.0 ** shift)


# ------------------------------------------------------------------ 1. bytes, exact
@pytest.mark.parametrize("nb", [1, K - 1, K, K + 1, 2 * K + 3])
@pytest.mark.parametrize("kind", ["uniform", "all127", "all0", "all255", "narrow", "mod251"])
def test_bytes_exact(sv, kind, nb):
    blocks = make(kind, nb)
    sv.reset()
    spec, hist, sums = sv.feed(blocks)
    want_hist, want_sums = byte_ref(blocks, K)
    assert spec.shape == (nb // K, N) and np.array_equal(hist, want_hist) and np.array_equal(sums, want_sums)
    assert sv.pending() == (nb, nb % K)
    if kind == "all255":
        assert int(sums[0, 1]) == 2130739200


def test_every_workgroup_loops_twice_and_one_block_more(eng):
    with _native.Survey(eng, 12) as s:       # intervals end inside tiles (12, 36, ...) and on tile edges (24, 48, ...)
        tile, wgs, fused = s.geometry()
        assert fused and tile >= 1 and wgs >= 1 and 12 % tile != 0 and 24 % tile == 0
        nb = 2 * tile * wgs + 1
        assert nb <= eng.max_batch
        blocks = make("mod251", nb)
        spec, hist, sums = s.feed(blocks)
        want_hist, want_sums = byte_ref(blocks, 12)
        assert np.array_equal(hist, want_hist) and np.array_equal(sums, want_sums) and len(spec) == nb // 12
        s.reset()
        parts = [s.feed(blocks[lo:lo + 1000]) for lo in range(0, nb, 1000)]      # other tiles, other grids
        assert np.array_equal(np.concatenate([p[0] for p in parts]), spec)
        assert np.array_equal(np.concatenate([p[1] for p in parts]), hist)
        assert np.array_equal(np.concatenate([p[2] for p in parts]), sums)


# ------------------------------------------------------------------ 2. raw stream
def test_raw_stream_equals_packed_blocks(sv):
    h = 4920
    step = 2 * (N - h)
    stream = make("uniform", 1, n=(10 * step + 2 * N) // 2, seed=9).ravel()
    blocks = survey_ref.blocks_of(stream, N, h)
    assert len(blocks) == 2 * K + 3
    sv.reset()
    want = sv.feed(blocks)
    e = _native.Engine.gate(N, h, max_batch=64)
    try:
        with _native.Survey(e, K) as s:
            got = s.feed_stream(stream)
            assert all(np.array_equal(a, b) for a, b in zip(got, want))
            # through the handle's input window (64 KiB segments: several per chunk)
            # (a mapping of its own: the window page-locks whole pages, and a heap array's last page can
            # hold the start of a result array, a copy into which would then be refused)
            pinned = np.frombuffer(mmap.mmap(-1, len(stream)), dtype=np.uint8)
            pinned[:] = stream
            e.input_window(pinned, segment_bytes=1 << 16)
            s.reset()
            again = s.feed_stream(pinned)
            e.input_window(None)
            assert all(np.array_equal(a, b) for a, b in zip(again, want))
    finally:
        e.close()


@pytest.mark.parametrize("h", [4920, 4921])
def test_capture_survey_reads_the_stream_in_place_or_packs_it(sv, h):
    """an even block_len - history_len is framed on the device, an odd one packed on the host: the same
    numbers as the same blocks fed packed"""
    step = 2 * (N - h)
    lead = -(-h // (N - h))
    total = lead + 2 * K + 1
    stream = make("uniform", 1, n=total * step // 2, seed=h).ravel()
    blocks = np.stack([stream[(i + 1) * step - 2 * N:(i + 1) * step] for i in range(lead, total)])
    sv.reset()
    spec, hist, sums = sv.feed(blocks)
    with survey.CaptureSurvey(N, h, integrate=K, batch_size=5) as cs:
        got = list(cs(io.BytesIO(stream.tobytes())))
    assert len(got) == 2 and [v.first_block for v in got] == [lead, lead + K]
    for j, v in enumerate(got):
        assert np.array_equal(v.mean_mag, mean_mag(spec[j], sv.shift, K)) and np.array_equal(v.hist, hist[j])
        assert np.array_equal(v.block_sums, sums[j * K:(j + 1) * K])


# ------------------------------------------------------------------ 3. cut-independence
def test_every_cut_gives_the_same_bits(sv):
    blocks = make("tone", 2 * K + 3, seed=23)
    sv.reset()
    want = sv.feed(blocks)
    assert len(want[0]) == 2 and want[0].any()

    def cut(sizes):
        sv.reset()
        parts, lo = [], 0
        for size in sizes:
            parts.append(sv.feed(blocks[lo:lo + size]))
            lo += size
        assert lo == len(blocks)
        return [np.concatenate([p[i] for p in parts]) for i in range(3)]

    for sizes in ([1] * len(blocks), [3, 2, 6], [5, 6], [9, 2]):     # inside a tile, inside an interval, both
        assert all(np.array_equal(a, b) for a, b in zip(cut(sizes), want)), sizes
    sv.reset()
    assert sv.pending() == (0, 0)
    assert all(np.array_equal(a, b) for a, b in zip(sv.feed_stream(blocks.ravel()), want))     # H = 0: a stream
    # reset starts over: without it the next blocks would complete the open interval
    assert sv.pending() == (len(blocks), 3)
    sv.reset()
    assert len(sv.feed(blocks[:K - 1])[0]) == 0


# ------------------------------------------------------------------ 4. spectrum against the oracle
@pytest.mark.parametrize("kind", ["tone", "narrow"])
def test_spectrum_against_the_float64_oracle(sv, oracle, kind):
    blocks, ref_mag, ref_hist, ref_sums = oracle[kind]
    sv.reset()
    spec, hist, sums = sv.feed(blocks)
    assert sv.shift == 30 - 14 and np.array_equal(hist, ref_hist) and np.array_equal(sums, ref_sums)
    got = mean_mag(spec, sv.shift, K)
    for j in range(len(ref_mag)):
        err, bound = rel_l2(got[j], ref_mag[j]), spectrum_bound(sv.shift, N, ref_mag[j])
        print("survey %s interval %d: rel-L2 %.3e (bound %.3e)" % (kind, j, err, bound))
        assert err <= bound
        if kind == "tone":
            assert int(np.argmax(got[j])) == 1234


# ------------------------------------------------------------------ 5. two implementations, one input
@pytest.mark.parametrize("kind", ["tone", "narrow"])
def test_fused_kernel_against_the_fold_path(sv, eng_multipass, oracle, kind):
    blocks, ref_mag, _, _ = oracle[kind]
    sv.reset()
    spec, hist, sums = sv.feed(blocks)
    with _native.Survey(eng_multipass, K) as s:
        assert s.geometry()[2] is False and sv.geometry()[2] is True
        spec2, hist2, sums2 = s.feed(blocks)
    assert np.array_equal(hist, hist2) and np.array_equal(sums, sums2)
    a, b = mean_mag(spec, sv.shift, K), mean_mag(spec2, sv.shift, K)
    for j in range(len(a)):
        err, bound = rel_l2(a[j], b[j]), 2 * spectrum_bound(sv.shift, N, ref_mag[j])
        print("survey fused vs fold %s interval %d: rel-L2 %.3e (bound %.3e)" % (kind, j, err, bound))
        assert err <= bound


@pytest.mark.parametrize("n", [1024, 65536])
def test_fold_path_alone(n):
    k = 2
    blocks = make("tone", 5, n=n, seed=n)
    blocks[2] = 255          # sum v^2 = 2 n 255^2: past 2^32 at 65536
    ref_mag, ref_hist, ref_sums = survey_ref.survey(blocks, k)
    e = _native.Engine.gate(n, 0, max_batch=8)
    try:
        with _native.Survey(e, k) as s:
            assert s.geometry()[2] is False and s.shift == 30 - int(np.log2(n))
            spec, hist, sums = s.feed(blocks[:3])
            more = s.feed(blocks[3:])
            spec, hist, sums = [np.concatenate([x, y]) for x, y in zip((spec, hist, sums), more)]
            shift = s.shift
    finally:
        e.close()
    assert np.array_equal(hist, ref_hist) and np.array_equal(sums, ref_sums) and len(spec) == 2
    if n == 65536:
        assert int(sums[2, 1]) > 2 ** 32
    got = mean_mag(spec, shift, k)
    for j in range(2):
        err, bound = rel_l2(got[j], ref_mag[j]), spectrum_bound(shift, n, ref_mag[j])
        print("survey fold n=%d interval %d: rel-L2 %.3e (bound %.3e)" % (n, j, err, bound))
        assert err <= bound


# ------------------------------------------------------------------ 6. errors
def _refused(call, needle):
    with pytest.raises(_native.NativeError) as err:
        call()
    assert "(code %d)" % _native.ERR_ARG in str(err.value) and needle in str(err.value), str(err.value)


def test_errors_are_arguments_and_leave_nothing_behind(eng, sv):
    _refused(lambda: _native.Survey(eng, 0), "integrate must be >= 1")
    blocks = make("narrow", 2 * K)
    sv.reset()
    sv.feed(blocks[:1])
    _refused(lambda: sv.feed(blocks, cap_intervals=1), "room for 1")
    _refused(lambda: sv.feed(np.zeros((1, N), dtype=np.complex64)), "u8")
    assert sv.pending() == (1, 1)          # nothing of the refused calls was fed
    odd = _native.Engine.gate(N, 4921, max_batch=8)
    try:
        with _native.Survey(odd, K) as s:
            _refused(lambda: s.feed_stream(blocks.ravel()), "even block_len - history_len")
            assert s.pending() == (0, 0)
    finally:
        odd.close()
    eng.sync()
    spec, hist, sums = sv.feed(blocks[1:])
    want_hist, want_sums = byte_ref(blocks, K)
    assert np.array_equal(hist, want_hist) and np.array_equal(sums, want_sums[1:]) and len(spec) == 2


def test_a_survey_gives_back_what_it_took(eng):
    before = _native.live_resources()
    s = _native.Survey(eng, K)
    during = _native.live_resources()
    s.feed(make("narrow", K))
    s.close()
    assert during[0] > before[0] and _native.live_resources() == before


# ------------------------------------------------------------------ 7. command line
def test_command_line(tmp_path):
    h = 4920
    step = 2 * (N - h)
    lead = -(-h // (N - h))
    stream = make("tone", 1, n=(lead + 2 * K) * step // 2, seed=31).ravel()
    capture, out = tmp_path / "capture.bin", tmp_path / "survey.npz"
    capture.write_bytes(stream.tobytes())
    with survey.CaptureSurvey(N, h, integrate=K) as cs:
        want = list(cs(open(str(capture), "rb")))
    assert len(want) == 2
    done = subprocess.run([sys.executable, "-m", "thrifty_amd.survey", str(capture), "-i", str(K), "--rms", "-o", str(out),
                           "--block-size", str(N), "--history", str(h)], cwd=ROOT, capture_output=True, text=True,
                          timeout=120)
    assert done.returncode == 0, done.stderr
    assert done.stdout.splitlines() == [repr(v.norm) for v in want]
    saved = np.load(str(out))
    assert saved["first_block"].tolist() == [lead, lead + K]
    assert np.array_equal(saved["mean_mag"], np.stack([v.mean_mag for v in want]))
    assert np.array_equal(saved["hist"], np.stack([v.hist for v in want]))
    assert np.array_equal(saved["block_sums"], np.stack([v.block_sums for v in want]))
    assert np.array_equal(saved["norm"], [v.norm for v in want])
