"""Seeded scenes for thr_track: transmitters that move with a slowly changing velocity, positions with noise.

    scene(seed, tracks, rows, ...) -> dict with tx, timestamp, x, y, rx, ry, valid (input row order), the planted
    `outlier` rows, and q, v0: what a test passes on.

The knobs: number of tracks, rows per track (one number or one per track), the time-step law ("exp": exponential
with mean `step`, "fixed": `step`, "zero": every timestamp of a track equal), the share of duplicate timestamps, the
share of planted outliers (100 m .. 10 km off, never a track's first row), outliers at given rows of a track
(`outlier_rows`: (track, row) pairs, x moved by OUTLIER_X metres, never row 0; they draw no random number, so a scene
is the same rows with and without them), invalid rows (a share at random, and / or explicit ranges of a track's rows,
whose x is NaN), and whether the rows of the tracks are interleaved at random."""
import numpy as np

SIGMA = 3.0       # metres, the noise of one axis
ACCEL = 0.5       # m s^-3/2
V0 = 10.0
OUTLIER_X = 500.0     # metres, what an `outlier_rows` row is moved by on x


def scene(seed, tracks=1, rows=256, law="exp", step=1.0, t0=0.0, duplicates=0.0, outliers=0.0, invalid=0.0, invalid_ranges=(),
          interleave=True, first_tx=3, outlier_rows=()):
    rng = np.random.default_rng(seed)
    rows = [rows] * tracks if np.isscalar(rows) else list(rows)
    cols = {name: [] for name in ("tx", "timestamp", "x", "y", "rx", "ry", "valid", "outlier")}
    for c, n in enumerate(rows):
        if law == "exp":
            dt = rng.exponential(step, n)
        elif law == "fixed":
            dt = np.full(n, step)
        else:
            dt = np.zeros(n)
        dt[rng.random(n) < duplicates] = 0.0
        t = t0 + 10.0 * c + np.cumsum(dt) - (dt[0] if n else 0.0)
        dt_true = np.diff(t, prepend=t[:1])
        vel = rng.normal(0.0, 5.0, 2) + np.cumsum(rng.normal(0.0, 1.0, (n, 2)) * (ACCEL * np.sqrt(dt_true))[:, None], axis=0)
        pos = rng.uniform(-2e4, 2e4, 2) + np.cumsum(vel * dt_true[:, None], axis=0)
        sig = SIGMA * rng.uniform(0.5, 2.0, (n, 2))
        meas = pos + rng.normal(0.0, 1.0, (n, 2)) * sig
        out = rng.random(n) < outliers
        if n:
            out[0] = False
        off = rng.uniform(np.log(100.0), np.log(1e4), n)
        ang = rng.uniform(0.0, 2.0 * np.pi, n)
        meas[out] += (np.exp(off) * np.stack([np.cos(ang), np.sin(ang)]))[:, out].T
        for track, row in outlier_rows:
            if track == c:
                assert 0 < row < n, "an outlier is never a track's first row"
                meas[row, 0] += OUTLIER_X
                out[row] = True
        ok = rng.random(n) >= invalid
        for track, a, e in invalid_ranges:
            if track == c:
                ok[a:e] = False
        meas[~ok, 0] = np.nan
        cols["tx"].append(np.full(n, first_tx + 2 * c, np.int32))
        cols["timestamp"].append(t)
        cols["x"].append(meas[:, 0])
        cols["y"].append(meas[:, 1])
        cols["rx"].append(sig[:, 0] ** 2)
        cols["ry"].append(sig[:, 1] ** 2)
        cols["valid"].append(ok.astype(np.uint8))
        cols["outlier"].append(out & ok)
    s = {name: np.concatenate(v) if v else np.zeros(0) for name, v in cols.items()}
    s["tx"] = s["tx"].astype(np.int32)
    s["valid"] = s["valid"].astype(np.uint8)
    s["outlier"] = s["outlier"].astype(bool)
    if interleave:
        perm = rng.permutation(len(s["tx"]))
        s = {name: v[perm] for name, v in s.items()}
    s["q"], s["v0"] = ACCEL * ACCEL, V0
    return s


COLUMNS = ("tx", "timestamp", "x", "y", "rx", "ry", "valid")


def columns(s):
    return tuple(s[name] for name in COLUMNS)


# the scenes the tests name; tests/golden/make_golden_track.py records a tolerance for each
def gating(k):
    """The three scenes of tests/test_gpu_track.py: 1, 3 and 8 tracks, interleaved, duplicates, outliers, an invalid block."""
    tracks = (1, 3, 8)[k]
    return scene(GATING_SEEDS[k], tracks=tracks, rows=4096 // tracks - 5 * k, duplicates=0.02, outliers=0.02,
                 invalid_ranges=((0, 40, 75),))


GATING_SEEDS = (109, 103, 114)      # chosen so that the gate takes three rounds and no nis lies near it


def seams():
    """name -> scene: the smallest shapes at which the scans can go wrong (tests/test_gpu_track_seams.py)."""
    out = {}
    for n in (0, 1, 2, 255, 256, 257, 512, 513, 769):
        out["single_%d" % n] = scene(200 + n, rows=n)
    out["meet_inside"] = scene(301, tracks=2, rows=(100, 300), interleave=False)
    out["meet_at_last"] = scene(302, tracks=2, rows=(255, 300), interleave=False)
    out["meet_at_first"] = scene(303, tracks=2, rows=(256, 300), interleave=False)
    out["singles_300"] = scene(304, tracks=300, rows=1)
    out["long_between"] = scene(305, tracks=3, rows=(1, 600, 1))
    out["invalid_first3"] = scene(306, rows=300, invalid_ranges=((0, 0, 3),))
    out["no_valid_row"] = scene(307, tracks=3, rows=(40, 30, 280), invalid_ranges=((1, 0, 30),))
    out["invalid_255"] = scene(308, rows=600, invalid_ranges=((0, 255, 256),))
    out["invalid_256"] = scene(309, rows=600, invalid_ranges=((0, 256, 257),))
    out["reject_255"] = scene(575, rows=600, interleave=False, outlier_rows=((0, 255),))      # a row the gate rejects (valid,
    out["reject_256"] = scene(576, rows=600, interleave=False, outlier_rows=((0, 256),))      # mask 0, nis reported) on a tile's seam
    out["invalid_tile"] = scene(310, rows=800, invalid_ranges=((0, 200, 521),))
    out["equal_times"] = scene(311, tracks=2, rows=(300, 20), law="zero")
    out["epoch_ms"] = scene(312, tracks=2, rows=(400, 200), law="fixed", step=1e-3, t0=1.5e9)
    return out
