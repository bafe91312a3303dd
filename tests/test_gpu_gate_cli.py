"""The product path of the carrier gate, through the command lines:

    python -m thrifty_amd.fastcard -i x.bin -o x.card -t 0c0s -k 1
    python -m thrifty_amd.detect x.card -o a.toad        against        python -m thrifty_amd.detect --raw x.bin -o b.toad

The same detections, block index shifted by the skip (block_card = block_raw - 1, soa shifted by
block_len - history accordingly), every other field equal as text except the timestamp; and with a
real threshold a.toad is exactly the subset of those lines whose blocks the gate passed.  Each GPU
subprocess runs under its own timeout, once.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from thrifty_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = subprocess.run([sys.executable, "-m"] + args, cwd=str(cwd), env=env, timeout=240,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert res.returncode == 0, (args, res.stdout[-2000:], res.stderr[-2000:])
    return res


def _card_indices(path):
    return [int(ln.split(" ")[1]) for ln in open(str(path)) if ln.strip() and not ln.startswith("#")]


def test_fastcard_then_detect_equals_detect_raw(tmp_path):
    n, h = 16384, 4096
    new = n - h
    tpl = synth.gold_template(10, 2)
    rng = np.random.default_rng(31)
    nblk = 40
    stream = rng.normal(0, 0.02, new * nblk) + 1j * rng.normal(0, 0.02, new * nblk)
    ook = 0.3 * (np.asarray(tpl, float) + 1) / 2
    k = np.arange(len(tpl))
    starts = [(9000, 33.3), (30000, 71.8), (52000, 55.1), (150000, 20.4), (300123, 90.9), (444444, 64.2)]
    for start, car in starts:
        stream[start:start + len(tpl)] += ook * np.exp(2j * np.pi * car * (k + start) / n)
    (tmp_path / "x.bin").write_bytes(synth.quantise_iq(stream).tobytes())
    np.save(tmp_path / "template.npy", tpl)
    (tmp_path / "detector.cfg").write_text(
        "rxid: 9\nsample_rate: 2.4M\nblock_size: %d\nblock_history: %d\ncarrier_window: 7 - 110\n"
        "carrier_threshold: 15 * snr\ncorr_threshold: 15*snr\ntemplate: %s\n" % (n, h, tmp_path / "template.npy"))
    geom = ["-b", str(n), "-h", str(h), "-k", "1"]

    res = _run(["thrifty_amd.fastcard", "-i", "x.bin", "-o", "x.card", "-t", "0c0s"] + geom, tmp_path)
    assert "Read %d blocks." % (nblk - 1) in res.stdout and res.stdout.count("block #") == nblk - 1
    assert _card_indices(tmp_path / "x.card") == list(range(nblk - 1))
    assert open(str(tmp_path / "x.card")).readline().startswith("# arguments: { carrier_bin: '0--1', threshold: '0c+0s'")
    _run(["thrifty_amd.detect", "x.card", "--quiet", "-o", "a.toad", "-c", "detector.cfg"], tmp_path)
    _run(["thrifty_amd.detect", "x.bin", "--raw", "--quiet", "-o", "b.toad", "-c", "detector.cfg"], tmp_path)
    a = [ln.split() for ln in (tmp_path / "a.toad").read_text().strip().split("\n")]
    b = [ln.split() for ln in (tmp_path / "b.toad").read_text().strip().split("\n")]
    # raw block 0 is the skipped one (the reference's zero-history lead-in): not in the card
    b = [f for f in b if int(f[2]) >= 1]
    assert len(a) == len(b) >= len(starts) - 1
    for fa, fb in zip(a, b):
        # rxid t block soa sample offset energy noise cbin coffset cenergy cnoise
        assert fa[0] == fb[0] and int(fa[2]) == int(fb[2]) - 1
        assert abs(float(fa[3]) - (float(fb[3]) - new)) <= 2e-8
        assert fa[4:] == fb[4:], (fa, fb)

    # a real threshold: the tone-free blocks stay below 100 x noise in the window, the bursts far above
    res = _run(["thrifty_amd.fastcard", "-i", "x.bin", "-o", "y.card", "-t", "0c100s", "-w", "7-110", "-q"] + geom,
               tmp_path)
    assert "block #" not in res.stdout and "Read " not in res.stdout
    passed = _card_indices(tmp_path / "y.card")
    assert 0 < len(passed) < nblk - 1 and passed == sorted(passed)
    _run(["thrifty_amd.detect", "y.card", "--quiet", "-o", "c.toad", "-c", "detector.cfg"], tmp_path)
    c = [ln.split() for ln in (tmp_path / "c.toad").read_text().strip().split("\n")]
    want = [f for f in a if int(f[2]) in set(passed)]
    assert len(c) == len(want) > 0
    for fc, fw in zip(c, want):
        assert fc[0] == fw[0] and fc[2:] == fw[2:], (fc, fw)

    # the card to stdout, the info lines to stderr (fastcard_cli.c:105-111); re-gating the card is the identity
    res = _run(["thrifty_amd.fastcard", "-i", "y.card", "--card", "-o", "-", "-t", "0c0s", "-k", "0", "-b", str(n),
                "-h", str(h)], tmp_path)
    lines = [ln for ln in (tmp_path / "y.card").read_text().split("\n") if ln and not ln.startswith("#")]
    assert [ln for ln in res.stdout.split("\n") if ln[:1].isdigit()] == lines
    assert res.stderr.count("block #") == len(passed)


def test_fastcard_refuses_capture_hardware(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, "-m", "thrifty_amd.fastcard", "-i", "rtlsdr"], cwd=str(tmp_path), env=env,
                         timeout=60, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert res.returncode != 0 and "out of scope" in res.stderr
