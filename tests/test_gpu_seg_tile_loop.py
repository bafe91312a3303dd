"""The tile loop of the segmented stages -- thr_toadstats, thr_beaconsync, thr_tdoastats, thr_reldist, thr_track --
with more tiles than workgroups.  Every tile kernel runs on min(tiles, 2048) workgroups and walks
`for (tile = blockIdx.x; tile < n_tiles; tile += gridDim.x)`, so a second trip needs more than 524 288 rows.
thr_debug_seg_tile_grid moves the cap on the workgroups, which changes which workgroup walks which tile and nothing
else, so the later trips are met at a few tiles: the reuse of the two LDS scan buffers, pass 2's LDS histogram zeroed
again after it was flushed (a workgroup that alternates between a tile counted in LDS and one that falls back to global
counters included), the carry of a fragment in a tile that is not the workgroup's first, the axis in blockIdx.y.

Per scene, at the caps 0 (the default), 1, 2 and 3:
  (a) the counts and every fetched array are the bytes of the default run;
  (b) at cap 1, where one workgroup walks every tile, the result also passes the stage's own comparison with its
      reference (the helpers of the stage's seam tests, imported), so the many-trip run is pinned to the truth;
  (c) thr_debug_seg_tile_stats shows that the cap reached the launches: ceil(tiles / cap) trips, the scene's tile
      count at cap 1, one trip at the default.  (A scene of exactly three tiles takes one trip at cap 3 as well;
      every scene takes at least two at cap 2, and every scene of four tiles or more at cap 3.)
Then the production grid itself, once per kernel family, device against device: 2048 * 256 + 257 rows are 2050 tiles,
two workgroups take a second trip, the last tile holds one row; the same call with the cap at 4096 takes one trip, and
the two must agree in every byte.  No float reference runs at that size; the discrete truths are checked."""
import functools
import os

import numpy as np
import pytest

import reldist_ref
import reldist_scenes
import test_gpu_syncstats_seams as sync_seams
import test_gpu_toadstats_seams as toad_seams
import track_check
import track_scenes
from thrifty_amd import _native, build

pytestmark = pytest.mark.gpu

T = 256                 # the tile (checked below)
DEFAULT_GRID = 2048     # kMaxTileGrid (checked below)
CAPS = (0, 1, 2, 3)
BIG = DEFAULT_GRID * T + 257


@pytest.fixture(autouse=True)
def cap():
    """cap(n) sets the tile-grid cap for the test; the default is back when the test ends, however it ends."""
    _native.seg_tile_grid(0)
    yield _native.seg_tile_grid
    _native.seg_tile_grid(0)


def tiles_of(rows):
    return -(-int(rows) // T)


def trips_at(tiles, workgroups):
    grid = min(tiles, workgroups if workgroups else DEFAULT_GRID)
    return -(-tiles // grid)


def same_bytes(a, b, what):
    (ca, oa), (cb, ob) = a, b
    assert ca == cb, what
    assert set(oa) == set(ob)
    for key in oa:
        assert oa[key].dtype == ob[key].dtype and oa[key].tobytes() == ob[key].tobytes(), (what, key)


def every_cap(cap, what, run, checked, tiles, same=same_bytes):
    """run() -> (counts, arrays) of one device call; checked() the same through the stage's comparison with its
    reference; tiles(counts) the largest tile count of the call's launches."""
    base = None
    for workgroups in CAPS:
        cap(workgroups)
        assert _native.seg_tile_stats() == (0, 0)
        got = (checked if workgroups == 1 else run)()
        launches, trips = _native.seg_tile_stats()
        n = tiles(got[0])
        print("%s: cap %d, %d tiles, %d tile grids, at most %d trips" % (what, workgroups, n, launches, trips))
        assert n >= 3 and launches > 0
        assert trips == trips_at(n, workgroups), (what, workgroups)      # 1 at the default, the tile count at cap 1
        assert trips >= 2 or workgroups == 0 or workgroups >= n
        if base is None:
            base = got
        else:
            same(got, base, "%s, cap %d" % (what, workgroups))


def test_the_constants_the_cases_were_sized_for(cap):
    shared = open(os.path.join(build.CSRC, "seg_reduce.hpp")).read()
    assert "constexpr int kTile = %d;" % T in shared and "constexpr int kMaxTileGrid = %d;" % DEFAULT_GRID in shared
    assert "constexpr int kHist = %d;" % KHIST in open(os.path.join(build.CSRC, "toadstats.hip")).read()
    assert _native.toadstats_geometry()[0] == T and _native.track_geometry()[0] == T and _native.reldist_geometry()[0] == T
    assert _native.syncstats_geometry("beaconsync")[0] == T and _native.syncstats_geometry("tdoastats")[0] == T
    assert tiles_of(BIG) == DEFAULT_GRID + 2 and BIG % T == 1


def test_the_setter_takes_its_range_and_resets_the_counts(cap):
    for bad in (-1, 65537, 1 << 20):
        with pytest.raises(ValueError, match="thr_debug_seg_tile_grid"):
            cap(bad)
    cols = toad_seams.scene(3 * T, 2, 2, seed=30)
    for workgroups, trips in ((65536, 1), (2, 2), (0, 1)):
        cap(workgroups)
        assert _native.seg_tile_stats() == (0, 0)
        _native.toadstats(cols)
        launches, most = _native.seg_tile_stats()
        assert launches == 3 and most == trips              # pass 1, pass 2, pass 3
        _native.toadstats(cols)
        assert _native.seg_tile_stats() == (6, trips)        # they add up until the next set


# ------------------------------------------------------------------ thr_toadstats
KHIST = 4096            # the LDS counters of pass 2


def alternating_scene():
    """Five tiles: 0, 2 and 4 are each one fragment of one cell (the last one short of a tile), 1 and 3 hold 64 cells
    of four rows.  Rows in random order: the stable sort by (rxid, txid) puts them there."""
    small = np.repeat(np.arange(64), 4)
    rx = np.r_[np.zeros(T, int), np.ones(T, int), np.full(T, 2), np.full(T, 3), np.full(T - 9, 4)]
    tx = np.r_[np.zeros(T, int), small, np.zeros(T, int), small, np.zeros(T - 9, int)]
    order = np.random.default_rng(31).permutation(len(rx))
    return toad_seams.scene(len(rx), rx[order], tx[order], seed=31)


TOAD_SCENES = {"one_cell": lambda: toad_seams.scene(3 * T + 5, [4], [2], seed=1),
               "three_tiles": lambda: toad_seams.scene(2 * T + 1, 2, 3, seed=2 * T + 1),
               "alternating": alternating_scene}


@pytest.mark.parametrize("name", sorted(TOAD_SCENES))
def test_toadstats(cap, name):
    cols = TOAD_SCENES[name]()
    kept = {}

    def checked():
        counts, out, ref = toad_seams.run_and_check(cols, what=name)
        kept["ref"] = ref
        return counts, out

    every_cap(cap, name, lambda: _native.toadstats(cols), checked, lambda counts: tiles_of(counts["rows"]))
    ref = kept["ref"]
    if name == "one_cell":
        assert ref["cell_ptr"].tolist() == [0, 3 * T + 5]
        assert np.all(np.diff(ref["minute_ptr"]) + np.diff(ref["bin_ptr"]) + 10 <= KHIST)      # every tile counts in LDS
    if name == "alternating":
        ptr = ref["cell_ptr"]
        assert ptr[-1] == 5 * T - 9 and len(ptr) - 1 == 3 + 2 * 64
        for tile in range(5):
            inside = np.count_nonzero((ptr[:-1] >= tile * T) & (ptr[:-1] < (tile + 1) * T))      # cells that start in it
            assert inside == (64 if tile % 2 else 1) and tile * T in ptr.tolist()
        big = np.flatnonzero(np.diff(ptr) >= T - 9)
        assert len(big) == 3 and ptr[big].tolist() == [0, 2 * T, 4 * T]
        # the one-fragment tiles fit the LDS counters: the cell's minutes bound the tile's window
        assert np.all(np.diff(ref["minute_ptr"])[big] + np.diff(ref["bin_ptr"])[big] + 10 <= KHIST)
        for key in ("minute_hist", "bin_hist", "offset_hist"):      # run_and_check held every count to these, at cap 1
            assert ref[key].sum() == 5 * T - 9


# ------------------------------------------------------------------ thr_beaconsync, thr_tdoastats
def beacon_scene(name):
    """-> (scene, deg, rows, cells)"""
    if name == "one_cell":
        n = 3 * T + 40
        jumps = [T - 1, T, 2 * T - 1, 2 * T, 3 * T - 1, 3 * T]       # dsdoa on both sides of each tile boundary
        return sync_seams.scene([(5, 1, 4, n, jumps)], seed=32), 3, n, 1
    pairs = [(b, r0, r1) for b in range(43) for r0 in range(3) for r1 in range(r0 + 1, 4)][:T + 1]
    return sync_seams.scene([key + (2, []) for key in pairs], seed=33), 2, 2 * (T + 1), T + 1


@pytest.mark.parametrize("name", ["one_cell", "cell_per_pair"])
def test_beaconsync(cap, name):
    (cols, ptr, idx), deg, rows, cells = beacon_scene(name)
    every_cap(cap, name, lambda: _native.beaconsync(cols, ptr, idx, deg),
              lambda: sync_seams.run_and_check(cols, ptr, idx, deg=deg, what=name), lambda counts: tiles_of(counts["rows"]))
    counts = _native.beaconsync(cols, ptr, idx, deg, outputs=())[0]
    assert counts["rows"] == rows and counts["cells"] == cells


def test_tdoastats_robust(cap):
    sizes = [T, 2 * T, 3 * T, 4 * T]
    cols = sync_seams.tdoa_scene(sizes, seed=34)
    every_cap(cap, "tdoa", lambda: _native.tdoastats(cols, robust=True),
              lambda: sync_seams.run_tdoa(cols, "tdoa, one workgroup", robust=True), lambda counts: tiles_of(counts["rows"]))
    out = _native.tdoastats(cols, robust=True)[1]
    assert sorted(np.diff(out["cell_ptr"]).tolist()) == sizes and out["mask"].any()


# ------------------------------------------------------------------ thr_reldist
@functools.lru_cache(maxsize=None)
def reldist_inputs():
    return reldist_scenes.seam_inputs(T)


@pytest.mark.parametrize("name", ["sizes_nearest", "sizes_linpol", "smooth_frac_0.5"])
def test_reldist(cap, name):
    args, kwargs = reldist_inputs()[name]
    want = reldist_ref.reldist_ref(*args, **kwargs)
    lengths = np.diff(args[1])
    pairs = int(np.sum(lengths * (lengths - 1) // 2))       # the stage's first layout holds every pair of every match

    def checked():
        got = _native.reldist(*args, **kwargs)
        reldist_ref.assert_same(got, want, what=name)
        return got

    assert pairs > want[0]["rows"] >= 3 * T
    every_cap(cap, name, lambda: _native.reldist(*args, **kwargs), checked, lambda counts: tiles_of(pairs))


# ------------------------------------------------------------------ thr_track
TRACK_SEAMS = ("single_769", "long_between", "meet_at_last", "invalid_tile", "reject_255", "reject_256")


def track_same(got, base, what):
    track_check.same_bytes(got, base)


@pytest.mark.parametrize("name", TRACK_SEAMS + ("gating_0",))
def test_track(cap, name):
    s, ref = track_check.gating(0) if name == "gating_0" else track_check.seam(name)
    track_check.assert_margin(ref)

    def checked():
        counts, out = track_check.device(s)
        track_check.compare(name, counts, out, ref)
        return counts, out

    every_cap(cap, name, lambda: track_check.device(s), checked, lambda counts: tiles_of(counts["rows"]), same=track_same)
    if name == "gating_0":
        assert tiles_of(len(s["tx"])) == 16 and ref["counts"]["rounds"] == 3


def test_track_one_round_on_one_workgroup(cap):
    """The extra run of a call that did not converge, with one workgroup walking the sixteen tiles."""
    s, _ = track_check.gating(0)
    ref = track_check.gating_0_one_round()
    track_check.assert_margin(ref)
    base = track_check.device(s, max_rounds=1)
    cap(1)
    counts, out = track_check.device(s, max_rounds=1)
    assert _native.seg_tile_stats()[1] == 16
    assert counts["converged"] == 0 and counts["rounds"] == 2
    track_check.compare("gating_0_one_round", counts, out, ref)
    track_check.same_bytes((counts, out), base)


# ------------------------------------------------------------------ the production grid, device against device
def default_and_wide(cap, run, same):
    """run() at the default cap (two trips for the first two workgroups) and at 4096 (one trip): the same bytes."""
    cap(0)
    base = run()
    assert _native.seg_tile_stats()[0] > 0 and _native.seg_tile_stats()[1] == 2
    cap(2 * DEFAULT_GRID)
    wide = run()
    assert _native.seg_tile_stats()[0] > 0 and _native.seg_tile_stats()[1] == 1
    same(wide, base, "cap 4096 against the default")
    return base


def test_toadstats_at_the_production_grid(cap):
    cols = toad_seams.scene(BIG, 6, 7, seed=35)
    counts, out = default_and_wide(cap, lambda: _native.toadstats(cols), same_bytes)
    key, rows = np.unique(cols["rxid"].astype(np.int64) * 100 + cols["txid"], return_counts=True)
    assert 24 <= len(key) <= 48 and counts["cells"] == len(key) and counts["rows"] == BIG
    assert np.array_equal(out["cell_ptr"], np.r_[0, np.cumsum(rows)])
    assert np.array_equal(out["cell_rx"].astype(np.int64) * 100 + out["cell_tx"], key)
    assert out["minute_hist"].sum() == BIG == out["bin_hist"].sum() == out["offset_hist"].sum()
    assert np.array_equal(out["order"], np.argsort(cols["rxid"].astype(np.int64) * 100 + cols["txid"], kind="stable"))


def test_tdoastats_at_the_production_grid(cap):
    g = np.random.default_rng(36)
    cell = g.integers(0, 12, BIG)
    centre = g.uniform(-300, 300, 12)
    cols = {"rx0": (cell % 3 - 1).astype(np.int32), "rx1": (cell % 3 + cell // 3).astype(np.int32), "tx": (cell // 2).astype(np.int32),
            "timestamp": 1.7e9 + np.arange(BIG) * 0.5, "det0_idx": 2 * np.arange(BIG, dtype=np.int64),
            "det1_idx": 2 * np.arange(BIG, dtype=np.int64) + 1, "tdoa": g.normal(centre[cell], 4.0) / sync_seams.R.LIGHT}
    counts, out = default_and_wide(cap, lambda: _native.tdoastats(cols, robust=True), same_bytes)
    key = (cols["rx0"].astype(np.int64) + 1) * 10000 + cols["rx1"] * 100 + cols["tx"]
    kinds, rows = np.unique(key, return_counts=True)
    assert counts["rows"] == BIG and counts["cells"] == len(kinds) == 12
    assert np.array_equal(out["cell_ptr"], np.r_[0, np.cumsum(rows)])
    assert np.array_equal((out["cell_key"][:, 0].astype(np.int64) + 1) * 10000 + out["cell_key"][:, 1] * 100 + out["cell_key"][:, 2], kinds)
    assert np.array_equal(out["order"], np.argsort(key, kind="stable"))
    masked = rows - out["robust_count"]
    assert np.all(masked > 0) and np.all(masked < rows // 50)        # |z| > 3.5 of a normal sample: some rows, few
    assert np.array_equal(np.add.reduceat(out["mask"].astype(np.int64), out["cell_ptr"][:-1]), masked)


def test_track_at_the_production_grid(cap):
    s = track_scenes.scene(37, tracks=3, rows=(BIG // 2, BIG // 3, BIG - BIG // 2 - BIG // 3), outliers=0.01)
    counts, out = default_and_wide(cap, lambda: track_check.device(s), track_same)
    tx, rows = np.unique(s["tx"], return_counts=True)
    assert len(set(rows.tolist())) == 3 and counts["rows"] == BIG and counts["tracks"] == 3
    assert np.array_equal(out["track_tx"], tx) and np.array_equal(out["track_ptr"], np.r_[0, np.cumsum(rows)])
    assert all(len(np.unique(s["timestamp"][s["tx"] == t])) == n for t, n in zip(tx, rows))      # distinct: one order
    assert np.array_equal(out["order"], np.lexsort((s["timestamp"], s["tx"])))
    assert counts["used"] + counts["rejected"] == BIG and 0 < counts["rejected"] < BIG // 20
    assert np.count_nonzero(out["used"]) == counts["used"] and np.isfinite(out["nis"]).all()
