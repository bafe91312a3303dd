"""Seeded scenes for thr_track: transmitters that move with a slowly changing velocity, positions with noise.

    scene(seed, tracks, rows, ...) -> dict with tx, timestamp, x, y, rx, ry, valid (input row order), the planted
    `outlier` rows, and q, v0: what a test passes on.

The knobs: number of tracks, rows per track (one number or one per track), the time-step law ("exp": exponential
with mean `step`, "fixed": `step`, "zero": every timestamp of a track equal), the share of duplicate timestamps, the
share of planted outliers (100 m .. 10 km off, never a track's first row), outliers at given rows of a track
(`outlier_rows`: (track, row) pairs, x moved by OUTLIER_X metres, never row 0; they draw no random number, so a scene
is the same rows with and without them), invalid rows (a share at random, and / or explicit ranges of a track's rows,
whose x is NaN), and whether the rows of the tracks are interleaved at random.

What tests/test_gpu_track_clauses.py needs in addition, none of which draws a random number unless used, so that a
scene without them keeps its bytes: an outlier ON a track's start row (`start_outliers`: (track, metres) pairs, x of
the track's first row moved: the header's known way to lose a track), an additive `offset` (dx, dy) of every
position, `r_scale` (one factor or a pattern of factors repeated along a track's rows in time order, on rx and ry AND
on the noise that is drawn with them), `t0` below zero, explicit timestamps of a track (`times`: {track: array}), explicit
transmitter ids (`tx_ids`: one per track), and the scene's own `q` and `v0`."""
import numpy as np

SIGMA = 3.0       # metres, the noise of one axis
ACCEL = 0.5       # m s^-3/2
V0 = 10.0
OUTLIER_X = 500.0     # metres, what an `outlier_rows` row is moved by on x


def scene(seed, tracks=1, rows=256, law="exp", step=1.0, t0=0.0, duplicates=0.0, outliers=0.0, invalid=0.0, invalid_ranges=(),
          interleave=True, first_tx=3, outlier_rows=(), start_outliers=(), offset=None, r_scale=None, times=None, tx_ids=None,
          q=None, v0=None):
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
        if times is not None and c in times:
            t = np.asarray(times[c], dtype=np.float64)
            assert t.shape == (n,)
        dt_true = np.diff(t, prepend=t[:1])
        vel = rng.normal(0.0, 5.0, 2) + np.cumsum(rng.normal(0.0, 1.0, (n, 2)) * (ACCEL * np.sqrt(dt_true))[:, None], axis=0)
        pos = rng.uniform(-2e4, 2e4, 2) + np.cumsum(vel * dt_true[:, None], axis=0)
        sig = SIGMA * rng.uniform(0.5, 2.0, (n, 2))
        if r_scale is not None:
            sig = sig * np.sqrt(np.resize(np.atleast_1d(np.asarray(r_scale, dtype=np.float64)), n))[:, None]
        meas = pos + rng.normal(0.0, 1.0, (n, 2)) * sig
        if offset is not None:
            meas = meas + np.asarray(offset, dtype=np.float64)
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
        for track, metres in start_outliers:
            if track == c:
                meas[0, 0] += metres
        ok = rng.random(n) >= invalid
        for track, a, e in invalid_ranges:
            if track == c:
                ok[a:e] = False
        meas[~ok, 0] = np.nan
        cols["tx"].append(np.full(n, first_tx + 2 * c if tx_ids is None else tx_ids[c], np.int32))
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
    s["q"], s["v0"] = ACCEL * ACCEL if q is None else q, V0 if v0 is None else v0
    return s


def join(*scenes, seed=None, q=None, v0=None):
    """The rows of several scenes in one call, one after the other or (seed) interleaved at random; q and v0 are the
    first scene's unless given."""
    s = {name: np.concatenate([one[name] for one in scenes]) for name in COLUMNS + ("outlier",)}
    if seed is not None:
        perm = np.random.default_rng(seed).permutation(len(s["tx"]))
        s = {name: v[perm] for name, v in s.items()}
    s["q"], s["v0"] = scenes[0]["q"] if q is None else q, scenes[0]["v0"] if v0 is None else v0
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


# ------------------------------------------------------------------ the clauses of the definition that no seam reaches
START_OUTLIER = 800.0     # metres on x of a track's start row
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1

# a regime is one 600-row track with these knobs behind a 100-row ordinary track of a lower tx: three fragments of
# 156 / 256 / 188 rows, so both carries are in play
REGIMES = {
    "q_0": dict(q=0.0),
    "q_1e-8": dict(q=1e-8),
    "q_1e4": dict(q=1e4),
    "v0_1e-3": dict(v0=1e-3),
    "v0_1e5": dict(v0=1e5),
    "r_1e-8": dict(r_scale=1e-8),
    "r_1e8": dict(r_scale=1e8),
    "utm_offset": dict(offset=(6e6, -4e6)),
    "steps_1e4": dict(step=1e4),
    "duplicates_q_0": dict(duplicates=0.5, q=0.0),
    "gap_400_v0_1e5": dict(invalid_ranges=((0, 100, 500),), v0=1e5),
}
# regimes whose recorded error is not small against their own measurement noise (tests/golden/make_golden_track.py
# measures them and asserts that they fail its condition; DESIGN.md 3.18 has the numbers): in no test
OUT_OF_RANGE = {
    "r_alternating": dict(r_scale=(1e-6, 1e6)),
    "gap_1e6_s": dict(times={0: np.concatenate([np.arange(300.0), 1e6 + np.arange(300.0, 600.0)])}),
}


def regime(knobs):
    track = scene(721, rows=600, first_tx=5, **knobs)
    return join(scene(720, rows=100, first_tx=3), track, seed=7, q=track["q"], v0=track["v0"])


def _lost(seed, rows, tx, **kw):
    return scene(seed, rows=rows, first_tx=tx, start_outliers=((0, START_OUTLIER),), **kw)


def load_pair():
    """Independence under load: A, 700 rows with 2 % outliers (rows 40 ..), and behind it in (tx, timestamp) order B, a
    track that its start row loses and that needs 13 filter runs."""
    a = scene(401, rows=700, outliers=0.02, first_tx=2)
    return a, join(_lost(506, 40, 9), a, q=a["q"], v0=a["v0"])


def clauses():
    """name -> (scene, options of the call): tests/test_gpu_track_clauses.py.  The seeds of the lost tracks are chosen
    so that the counts named below hold in the reference (tests/test_track_host.py asserts them)."""
    out = {}
    ordinary = scene(700, rows=100, first_tx=3)
    # used, valid of the track with tx 5 after max_rounds + 1 runs: 30 of 60 | 30 of 61 | 15 of 40; 13 runs, 3 of 40
    out["lost_equal"] = (join(ordinary, _lost(500, 60, 5), _lost(501, 40, 7), seed=1), dict(max_rounds=4))
    out["lost_one_below"] = (join(ordinary, _lost(643, 61, 5), seed=2), dict(max_rounds=4))
    out["lost_unconverged"] = (join(ordinary, _lost(503, 40, 5), seed=3), dict(max_rounds=4))
    out["lost_late"] = (join(ordinary, _lost(506, 40, 5), seed=4), dict(max_rounds=16))
    out["lost_remedy"] = (join(_lost(503, 40, 3, invalid_ranges=((0, 0, 1),)), _lost(508, 40, 5), seed=5), dict(max_rounds=4))
    out["neg_times"] = (join(scene(710, rows=300, t0=-150.0, first_tx=3),
                             scene(711, rows=200, first_tx=5, times={0: -1.5e9 + 1e-3 * np.arange(200)}), seed=6), {})
    first, second = np.arange(60.0) - 3.0, np.arange(60.0) - 3.0
    first[3:5], second[3:5] = (-0.0, 0.0), (0.0, -0.0)
    out["signed_zero"] = (join(scene(713, rows=60, first_tx=5, interleave=False, times={0: second}),
                               scene(712, rows=60, first_tx=3, interleave=False, times={0: first})), {})
    out["tx_extremes"] = (scene(714, tracks=4, rows=70, tx_ids=(INT32_MIN, -1, 0, INT32_MAX)), {})
    out["all_valid"] = (scene(730, tracks=2, rows=(300, 150)), {})
    pair = load_pair()[1]
    out["under_load_16"] = (pair, dict(max_rounds=16))
    out["under_load_4"] = (pair, dict(max_rounds=4))
    for name, knobs in REGIMES.items():
        out[name] = (regime(knobs), dict(gate=0.0))
    return out
