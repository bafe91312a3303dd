"""One small valid call for each post-detect entry point, and what the host-contract tests need to know about it
(tests/test_gpu_post_resources.py, test_gpu_post_fetch.py, test_gpu_post_threads.py, test_post_contract_host.py).

A `Case` is the `_native` wrapper, its `*_times` function, the input arrays (read-only: a call that wrote into one would
raise), one host refusal, the early stops and the call with nothing in it.  For the families that hand out a result
handle it also names the fetch / free pair and the `*_OUTPUTS` table.

The raw `lib.thr_X(...)` argument list of a case is not written out a second time here: `raw_call` runs the wrapper
with a tap in the library's place that passes everything through except the entry point itself, where it takes the
argument list the wrapper built from `_native`'s own ctypes structures (ThrPosq3Opts, ThrPosq3Counts, ...), changes
what the test asks it to change, makes the call, and hands back the status, the handle and the counts WITHOUT letting
the wrapper fetch and free.  The list can therefore not drift from the wrapper's, and the handle is the library's own.

The inputs are the suite's generators at the smallest shapes that still take every launch of the stage; none needs more
than a second on the device.  thr_toadstats, thr_beaconsync, thr_tdoastats and thr_reldist refuse a call without rows
("the selection is empty"); thr_coverage has no row count at all, its smallest call is one cell."""
import collections
import ctypes as C
import threading

import numpy as np

import coverage_golden
import pos3_golden
import pos_golden
import posg3_golden
import posg_golden
import posq3_golden
import posq_golden
import postdetect_scene
import reldist_scenes
import tdoa_golden
import track_scenes
from thrifty_amd import _native, kitchen_sink, pos_3d, tdoa_est

KINDS = ("device buffers", "pinned buffers", "streams", "events")
RESULT_EVENTS = 2       # `Event ev[2]` of seg::Result (csrc/seg_reduce.hpp) and of thr_post (csrc/postdetect.hip)

Family = collections.namedtuple("Family", "stem outputs")
Refusal = collections.namedtuple("Refusal", "match args kwargs mutate")
Refusal.__new__.__defaults__ = (None, None, None)


def arrays_of(obj):
    """Every ndarray in a nest of tuples, lists and dicts."""
    if isinstance(obj, np.ndarray):
        yield obj
    elif isinstance(obj, dict):
        for v in obj.values():
            yield from arrays_of(v)
    elif isinstance(obj, (tuple, list)):
        for v in obj:
            yield from arrays_of(v)


def own(value):
    """A copy the case may freeze: the generators' caches stay writable for the other tests."""
    if isinstance(value, np.ndarray):
        return value.copy()
    if isinstance(value, dict):
        return {k: own(v) for k, v in value.items()}
    if isinstance(value, (tuple, list)):
        return type(value)(own(v) for v in value)
    return value


class Case(object):
    def __init__(self, name, entry, fn, times, args, kwargs=None, family=None, refusal=None, stops=None, zero=None,
                 zero_refused=None, n_times=3):
        self.name, self.entry, self.fn, self.times, self.n_times = name, entry, fn, times, n_times
        self.args, self.kwargs = tuple(args), dict(kwargs or {})
        self.family, self.refusal = family, refusal
        self.stops = dict(stops or {})       # name -> (args or None, kwargs changes)
        self.zero, self.zero_refused = zero, zero_refused        # (args, kwargs changes) of the call with no rows
        for a in arrays_of((self.args, self.kwargs, [self.refusal.args, self.refusal.kwargs] if refusal else None,
                            list(self.stops.values()), self.zero)):
            a.setflags(write=False)

    def run(self, args=None, **changes):
        return self.fn(*(self.args if args is None else args), **dict(self.kwargs, **changes))

    def inputs(self, args=None, changes=None):
        return list(arrays_of((self.args if args is None else args, dict(self.kwargs, **(changes or {})))))

    def __repr__(self):
        return self.name


def flatten(result):
    """What a wrapper returns -> {name: array}: the tuple of identify and match, the dict of tdoa, pos and pos3, the
    (counts, outputs) pair of the handle families (the counts as one more array)."""
    if isinstance(result, dict):
        return dict(result)
    if len(result) == 2 and isinstance(result[0], dict):
        out = dict(result[1])
        out["(counts)"] = np.array([float(result[0][k]) for k in sorted(result[0])])
        return out
    return {"(%d)" % k: np.asarray(v) for k, v in enumerate(result)}


def same_bytes(got, want):
    """The names whose arrays differ in type, shape or bytes."""
    bad = [k for k in sorted(set(got) | set(want)) if k not in got or k not in want]
    return bad + [k for k in sorted(set(got) & set(want))
                  if got[k].dtype != want[k].dtype or got[k].shape != want[k].shape or got[k].tobytes() != want[k].tobytes()]


# ------------------------------------------------------------------ the raw call
class _Held(Exception):
    pass


class _Tap(object):
    def __init__(self, lib, entry, mutate, hold):
        self._lib, self._entry, self._mutate, self._hold = lib, entry, mutate, hold
        self.called, self.rc, self.error, self.handle, self.counts = False, None, "", None, None

    def __getattr__(self, name):
        real = getattr(self._lib, name)
        if name != self._entry:
            return real

        def call(*args):
            args = list(args)
            if self._mutate is not None:
                self._mutate(args)
            self.called = True
            self.rc = real(*args)
            self.error = self._lib.thr_last_error().decode() if self.rc else ""
            if hasattr(args[-2], "_obj") and isinstance(args[-2]._obj, C.c_void_p):       # a handle family
                self.handle, self.counts = args[-2]._obj, args[-1]._obj
            if self._hold and self.rc == 0:
                raise _Held()
            return self.rc
        return call


_tap_lock = threading.Lock()


class Raw(object):
    """The outcome of one raw call: rc, error (thr_last_error() if rc != 0), handle (c_void_p) and counts (the ctypes
    structure) of a handle family, result / exception of the wrapper where it ran on."""

    def __init__(self, case, tap, result, exception):
        self.case, self.rc, self.error, self.handle, self.counts = case, tap.rc, tap.error, tap.handle, tap.counts
        self.result, self.exception = result, exception

    def counts_dict(self):
        return {name: int(getattr(self.counts, name)) for name, kind in self.counts._fields_ if kind is C.c_size_t}

    def free(self):
        getattr(_native.load_library(), "thr_%s_free" % self.case.family.stem)(self.handle)
        self.handle = C.c_void_p()


def raw_call(case, args=None, mutate=None, hold=True, **changes):
    """The case's call with the library's entry point tapped (the module docstring).  `mutate(arguments)` may change the
    raw argument list in place.  hold: a successful call stops before the wrapper fetches and frees (the caller frees
    Raw.handle); otherwise, and after a refusal, the wrapper runs on and its result or exception is kept."""
    lib = _native.load_library()
    tap = _Tap(lib, case.entry, mutate, hold)
    result = exception = None
    with _tap_lock:
        _native._lib = tap
        try:
            result = case.run(args, **changes)
        except _Held:
            pass
        except Exception as exc:      # noqa: BLE001 -- kept for the test to look at
            exception = exc
        finally:
            _native._lib = lib
    assert tap.called, "%s: the wrapper never reached %s (%r)" % (case, case.entry, exception)
    return Raw(case, tap, result, exception)


def output_specs(case, counts, args=None):
    """{name: (index, dtype, shape)} of a handle family for the counts of one call."""
    if case.family.stem == "post":
        a = case.args if args is None else args
        n, dims = len(a[0]), int(case.kwargs["settings"][0].dims)
        return {name: (which, np.dtype(kind), tuple(shape(n, counts, dims))) for name, (which, kind, shape) in case.family.outputs.items()}
    return {name: (which, np.dtype(kind), tuple(shape(counts))) for name, (which, kind, shape) in case.family.outputs.items()}


def fetch(case, handle, which, dst, nbytes):
    """thr_<stem>_fetch -> its status; dst: an array or None."""
    fn = getattr(_native.load_library(), "thr_%s_fetch" % case.family.stem)
    return fn(handle, int(which), None if dst is None else dst.ctypes.data, int(nbytes))


def fetch_all(case, raw, args=None):
    """Every output of a held handle, fetched with the size `_native`'s shape table gives -> {name: array}."""
    out = {}
    for name, (which, kind, shape) in output_specs(case, raw.counts_dict(), args).items():
        out[name] = np.zeros(shape, dtype=kind)
        rc = fetch(case, raw.handle, which, out[name], out[name].nbytes)
        assert rc == 0, (case, name, shape, _native.load_library().thr_last_error().decode())
    return out


# ------------------------------------------------------------------ the inputs
def _csr_zero(args, n_cols=5):
    """group_ptr [0] and empty row columns in front of the rest of a CSR entry point's arguments."""
    kinds = (np.int32, np.int32, np.float64, np.float64)
    return (np.zeros(1, np.int64),) + tuple(np.zeros(0, k) for k in kinds) + tuple(args[n_cols:])


def _identify_cases():
    n = 200
    rng = np.random.default_rng(n)
    centres = np.array([30, 61, 93])
    tx = rng.integers(0, 3, n)
    rxid = rng.integers(0, 4, n).astype(np.int32)
    cbin = (centres[tx] + rxid + np.round(rng.normal(0, 0.7, n))).astype(np.int32)
    coff = rng.uniform(-0.5, 0.5, n)
    block = rng.integers(0, max(2, n // 3), n).astype(np.int32)
    ts = 1.7e9 + block * 0.00512 + rng.uniform(0, 1e-3, n)
    energy = rng.uniform(50, 200, n)
    args = (rxid, block, ts, cbin, coff, energy)
    fm = [(r, t, centres[t] + r - 2.6, centres[t] + r + 2.6) for r in range(4) for t in range(3)]
    zero = (tuple(a[:0].copy() for a in args), {})
    wide = cbin.copy()
    wide[0], wide[1] = np.iinfo(np.int32).min, np.iinfo(np.int32).max

    def no_map(raw):        # (device_id, n, six columns, map, n_map, ...): a map of 12 rows at NULL
        raw[8] = None
    yield Case("identify_map", "thr_identify", _native.identify, None, own(args), dict(freq_ranges=fm), zero=own(zero),
               refusal=Refusal("thr_identify: null frequency map", mutate=no_map))
    yield Case("identify_auto", "thr_identify", _native.identify, None, own(args), dict(freq_ranges=None), zero=own(zero),
               refusal=Refusal("thr_identify: carrier bins span", args=(rxid, block, ts, wide, coff, energy)))


def match_columns(n=65, n_rx=3, n_tx=2, seed=65):
    """n detections of n_rx receivers and n_tx transmitters in timestamp order, on a 0.25 s grid with ties."""
    rng = np.random.default_rng(seed)
    ts = np.sort(0.25 * rng.integers(0, max(2, n // 6), n))
    return (rng.integers(0, n_rx, n).astype(np.int32), rng.integers(0, n_tx, n).astype(np.int32), ts,
            rng.integers(1, 4, n).astype(np.float64))


def _match_case():
    cols = match_columns()

    def no_timestamps(raw):     # (device_id, n, rxid, txid, timestamp, ...)
        raw[4] = None
    return Case("match", "thr_match", _native.match, _native.match_times, cols + (0.5,), dict(min_match=2),
                zero=(tuple(c[:0].copy() for c in cols) + (0.5,), {}),
                refusal=Refusal("thr_match: null argument", mutate=no_timestamps))


def tdoa_arguments(cols, match_ptr, match_idx, rx_pos, beacon_pos, window=8.0, sample_rate=2.4e6):
    """Detection columns with receiver ids, the matches as CSR and the two position tables -> _native.tdoa's positional
    arguments (tdoa_est.tdoa_columns' preparation)."""
    receivers, beacons = sorted(rx_pos), sorted(beacon_pos)
    ptr, idx = np.asarray(match_ptr, dtype=np.int64), np.asarray(match_idx, dtype=np.int64)
    first_tx = np.asarray(cols["txid"])[idx[ptr[:-1]]]
    match_beacon = np.array([beacons.index(t) if t in beacons else -1 for t in first_tx.tolist()], dtype=np.int32)
    dist = np.array([[tdoa_est._distance(rx_pos[r], beacon_pos[b]) for b in beacons] for r in receivers], dtype=np.float64)
    dense = np.searchsorted(receivers, cols["rxid"]).astype(np.int32)
    return (dense,) + tuple(np.asarray(cols[k], dtype=np.float64) for k in ("timestamp", "soa", "energy", "noise")) + (
        ptr, idx, match_beacon, dist.reshape(len(receivers), len(beacons)), float(window), float(sample_rate))


def _tdoa_cases():
    g = tdoa_golden.load("tdoa_ties")
    rx_pos, beacon_pos = tdoa_golden.positions(g)
    args = own(tdoa_arguments(g, g["match_ptr"], g["match_idx"], rx_pos, beacon_pos, float(g["window"]), float(g["sample_rate"])))
    # no task: five transmissions of a beacon and none of a mobile (test_gpu_tdoa_seams.py::
    # test_no_beacon_match_and_no_mobile_match, its second scene)
    from test_gpu_tdoa_seams import BEACON_POS, RX_POS, Scene
    scene = Scene()
    for k in range(5):
        scene.send(0, float(k), [0, 1, 2])
    ptr = np.cumsum([0] + [len(m) for m in scene.matches])
    no_task = tdoa_arguments(scene.cols(), ptr, [i for m in scene.matches for i in m], RX_POS, BEACON_POS)
    zero = (np.zeros(0, np.int32),) + (np.zeros(0),) * 4 + (np.zeros(1, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int32)) + args[8:]
    other = args[7].copy()
    other[0] = args[8].shape[1]        # the first match names a beacon past the table
    bad = args[:7] + (other,) + args[8:]
    for name, model in (("tdoa", None), ("tdoa_nearest", "nearest"), ("tdoa_linear", "linear"), ("tdoa_weighted", "weighted_poly")):
        entry = "thr_tdoa" if model is None else "thr_tdoa_model"
        yield Case(name, entry, _native.tdoa, _native.tdoa_times, args,
                   dict(deg=int(g["deg"]), model=None if model is None else _native.TDOA_MODELS[model]),
                   stops={"no_task": (own(no_task), {})}, zero=(own(zero), {}),
                   refusal=Refusal("thr_tdoa: match 0 names beacon", args=own(bad)))


def _pos_cases():
    for name in ("pos_three", "pos_line"):
        g = pos_golden.load(name)
        args = own((g["group_ptr"], pos_golden.dense(g, g["rx0"]), pos_golden.dense(g, g["rx1"]), g["tdoa"], g["snr"], g["rx_xyz"]))
        yield Case(name, "thr_pos", _native.pos, _native.pos_times, args, zero=(_csr_zero(args), {}),
                   refusal=Refusal("thr_pos: max_iter must not be negative", kwargs=dict(max_iter=-1)))


def _pos3_cases():
    for name in ("z_four", "h_ring4"):
        g = pos3_golden.load(name)
        table = g["rx_xyz"]
        dense = {int(r): k for k, r in enumerate(g["rx_ids"])}
        rx0, rx1 = (np.array([dense[int(v)] for v in g[key]], dtype=np.int32) for key in ("rx0", "rx1"))
        if pos3_golden.free_z(g):
            z0, z_range = pos_3d.start_height(table, float(g["z0"]), tuple(g["z_range"].tolist()) if len(g["z_range"]) else None)
            kwargs = dict(group_h=None, x0=(0.1, 0.1, float(z0)), z_range=None if z_range is None else np.asarray(z_range, dtype=np.float64))
            mode = _native.POS3_FREE_Z
        else:
            kwargs, mode = dict(group_h=g["group_h"]), _native.POS3_KNOWN_HEIGHT
        args = own((g["group_ptr"], rx0, rx1, g["tdoa"], g["snr"], table, mode))
        yield Case(name, "thr_pos3", _native.pos3, _native.pos3_times, args, own(kwargs),
                   zero=(_csr_zero(args), dict(group_h=None if kwargs["group_h"] is None else np.zeros(0))),
                   refusal=Refusal("thr_pos3: max_iter must not be negative", kwargs=dict(max_iter=-1)))


def post_columns(cols):
    return tuple(cols[name] for name in kitchen_sink.COLUMNS)


def _postdetect_case():
    st = postdetect_scene.settings()
    native, _ = kitchen_sink._native_settings(st, 2, 2, (0.1, 0.1), 100, False)
    bad_deg, _ = kitchen_sink._native_settings(st, 2, 0, (0.1, 0.1), 100, False)
    cols = postdetect_scene.columns(60)
    seams = postdetect_scene.columns(140)        # the scenes of tests/test_gpu_postdetect_seams.py
    stops = {
        "nothing_kept": (post_columns(dict(seams, carrier_bin=np.full_like(seams["carrier_bin"], 5))), {}),
        "all_misses": (post_columns(postdetect_scene.columns(60, only=[0], extras=False)), {}),
        "beacon_matches_only": (post_columns(postdetect_scene.columns(60, tx_order=(0, 1))), {}),
        "every_group_underdetermined": (post_columns(postdetect_scene.columns(80, only=[0, 1], extras=False)), {}),
    }
    return Case("postdetect", "thr_postdetect", _native.postdetect, _native.post_times, post_columns(cols), dict(settings=native),
                family=Family("post", _native.POST_OUTPUTS), stops=stops, n_times=6,
                zero=(post_columns(postdetect_scene.head(cols, 0)), {}),
                refusal=Refusal("thr_postdetect: deg must be 1, 2 or 3", kwargs=dict(settings=bad_deg)))


def _stats_cases():
    from test_gpu_syncstats_seams import scene as bsync_scene, tdoa_scene
    from test_gpu_tdoa_matrix_seams import beacon_times, scene as tdmat_scene
    from test_gpu_toadstats_seams import scene as tstats_scene
    n = 65
    cols = tstats_scene(n, 2, 3, seed=n)
    empty = {k: np.asarray(v)[:0].copy() for k, v in cols.items()}
    yield Case("toadstats", "thr_toadstats", _native.toadstats, _native.toadstats_times, (own(cols),), n_times=5,
               family=Family("tstats", _native.TSTATS_OUTPUTS), zero=((empty,), {}), zero_refused="the selection is empty",
               refusal=Refusal("thr_toadstats: sel[1] = 65 is out of range", kwargs=dict(sel=np.array([0, n], np.int64))))
    cols, ptr, idx = bsync_scene([(0, 0, 1, n, [n // 3, n // 3 + 14])], seed=n)
    empty = {k: np.asarray(v)[:0].copy() for k, v in cols.items()}
    yield Case("beaconsync", "thr_beaconsync", _native.beaconsync, lambda: _native.syncstats_times("beaconsync"), own((cols, ptr, idx)),
               dict(deg=2), family=Family("bsync", _native.BSYNC_OUTPUTS), n_times=5,
               zero=((empty, np.zeros(1, np.int64), np.zeros(0, np.int64)), {}), zero_refused="the selection is empty",
               refusal=Refusal("thr_beaconsync: deg must be 1, 2 or 3", kwargs=dict(deg=0)))
    cols = tdoa_scene([1, 2, 3, 4, 63], seed=1)
    empty = {k: np.asarray(v)[:0].copy() for k, v in cols.items()}
    yield Case("tdoastats", "thr_tdoastats", _native.tdoastats, lambda: _native.syncstats_times("tdoastats"), (own(cols),),
               dict(robust=True), family=Family("tdstats", _native.TDSTATS_OUTPUTS), n_times=5,
               zero=((empty,), {}), zero_refused="the selection is empty",
               refusal=Refusal("thr_tdoastats: the detection id range is empty", kwargs=dict(detidx=(21, 20))))
    cols, ptr, idx = reldist_scenes.sized_cells([2, 3, 9])
    empty = {k: np.asarray(v)[:0].copy() for k, v in cols.items()}
    yield Case("reldist", "thr_reldist", _native.reldist, _native.reldist_times, own((cols, ptr, idx)), dict(beacons=[0]),
               family=Family("reldist", _native.RELDIST_OUTPUTS), n_times=5,
               zero=((empty, np.zeros(1, np.int64), np.zeros(0, np.int64)), {}), zero_refused="the selection is empty",
               refusal=Refusal("thr_reldist: smooth_frac must lie in [0, 1]", kwargs=dict(smooth_frac=1.5)))
    cols, ptr, idx = tdmat_scene(15, 2, {0: beacon_times(20), 7: np.linspace(5.2, 14.7, 5).tolist()})
    empty = {k: np.asarray(v)[:0].copy() for k, v in cols.items()}
    yield Case("tdoamatrix", "thr_tdoamatrix", _native.tdoamatrix, _native.tdoamatrix_times, own((cols, ptr, idx)),
               dict(beacons=[0], targets=[7]), family=Family("tdmat", _native.TDMAT_OUTPUTS), n_times=5,
               zero=((empty, np.zeros(1, np.int64), np.zeros(0, np.int64)), {}),
               refusal=Refusal("thr_tdoamatrix: deg must be 1, 2 or 3", kwargs=dict(deg=0)))


def _csr(s):
    return own((s["group_ptr"], s["rx0"], s["rx1"], s["tdoa"], s["snr"], s["table"]))


def underdetermined(s):
    """The scene with two rows of one receiver pair per group: no group names three receivers."""
    n = len(s["group_ptr"]) - 1
    first = np.asarray(s["group_ptr"][:-1])
    rows = np.stack([first, first], axis=1).reshape(-1)
    return (2 * np.arange(n + 1, dtype=np.int64),) + tuple(np.asarray(s[k])[rows].copy() for k in ("rx0", "rx1", "tdoa", "snr")) + (
        s["table"].copy(),)


TINY_GATE = 1e-9        # metres: every group that may be flagged is


def _quality_cases():
    s = posq_golden.scene(6, 6, 33, every=2)
    args = _csr(s)
    yield Case("posq", "thr_posq", _native.posq, _native.posq_times, args, dict(gate_m=3.0), n_times=6,
               family=Family("posq", _native.POSQ_OUTPUTS), zero=(_csr_zero(args), {}),
               stops={"gate_0": (None, dict(gate_m=0.0)), "tiny_gate": (None, dict(gate_m=TINY_GATE))},
               refusal=Refusal("thr_posq: ratio must lie in (0, 1]", kwargs=dict(ratio=1.5)))
    for name, free_z in (("posq3_known_height", False), ("posq3_free_z", True)):
        s = posq3_golden.scene(7, 7, 7, every=1, tag_z=1.0 if free_z else np.linspace(0.5, 2.5, 7))
        args = _csr(s)
        if free_z:
            mode, kwargs = _native.POS3_FREE_Z, dict(group_h=None, x0=(0.1, 0.1, float(s["table"][:, 2].min()) - 1.0), z_range=None)
        else:
            mode, kwargs = _native.POS3_KNOWN_HEIGHT, dict(group_h=s["mobile"][:, 2].copy(), x0=(0.1, 0.1, 0.0), z_range=None)
        yield Case(name, "thr_posq3", _native.posq3, _native.posq3_times, args + (mode,), dict(kwargs, gate_m=3.0), n_times=6,
                   family=Family("posq3", _native.POSQ3_OUTPUTS),
                   zero=(_csr_zero(args) + (mode,), dict(group_h=None if free_z else np.zeros(0))),
                   stops={"gate_0": (None, dict(gate_m=0.0)), "tiny_gate": (None, dict(gate_m=TINY_GATE))},
                   refusal=Refusal("thr_posq3: ratio must lie in (0, 1]", kwargs=dict(ratio=1.5)))


def _global_cases():
    s = posg_golden.scene(0, 4, 9, 0.3)
    args = _csr(s)
    kwargs = dict(margin_m=posg_golden.margin_of(s["table"]), grid=32, starts=4, map_first=0, map_count=1)
    yield Case("posg", "thr_posg", _native.posg, _native.posg_times, args, kwargs, family=Family("posg", _native.POSG_OUTPUTS), n_times=6,
               zero=(_csr_zero(args), dict(map_count=0)), stops={"every_group_underdetermined": (own(underdetermined(s)), {})},
               refusal=Refusal("thr_posg: grid must be 16, 32 or 64, not 48", kwargs=dict(grid=48)))
    for name, free_z in (("posg3_free_z", True), ("posg3_known_height", False)):
        s = posg3_golden.ring_scene(6, 6, 300.0, (2.0, 42.0), 3e-9, 6)
        args = _csr(s)
        table = s["table"]
        kwargs = dict(margin_m=float(np.max(table[:, :2].max(axis=0) - table[:, :2].min(axis=0))), grid=16, starts=1, map_first=0,
                      map_count=1)
        if free_z:
            mode = _native.POS3_FREE_Z
            kwargs.update(grid_z=2, z_grid=posg3_golden.default_z_grid(table), x0=(0.1, 0.1, float(table[:, 2].min()) - 1.0))
        else:
            mode = _native.POS3_KNOWN_HEIGHT
            kwargs.update(grid_z=1, group_h=s["planted"][:, 2].copy())
        few = own(underdetermined(s))
        yield Case(name, "thr_posg3", _native.posg3, _native.posg3_times, args + (mode,), kwargs, n_times=6,
                   family=Family("posg3", _native.POSG3_OUTPUTS),
                   zero=(_csr_zero(args) + (mode,), dict(map_count=0, **({} if free_z else {"group_h": np.zeros(0)}))),
                   stops={"every_group_underdetermined": (few + (mode,), {})},
                   refusal=Refusal("thr_posg3: grid must be 16 or 32, not 64", kwargs=dict(grid=64)))


def _track_case():
    s = track_scenes.scene(3, tracks=2, rows=256)
    args = own(track_scenes.columns(s))
    invalid = args[:6] + (np.zeros(len(args[0]), np.uint8),)
    return Case("track", "thr_track", _native.track, _native.track_times, args, dict(q=s["q"], v0=s["v0"]), n_times=6,
                family=Family("track", _native.TRACK_OUTPUTS), zero=(tuple(a[:0].copy() for a in args), {}),
                stops={"every_row_invalid": (invalid, {})},
                refusal=Refusal("thr_track: q must be finite and not negative", kwargs=dict(q=-1.0)))


def _coverage_case():
    args = (coverage_golden.ring(3, 5), np.full(5, 0.05), (-40.0, -35.0), (40.0, 35.0), 4, 3, 1.0)
    return Case("coverage", "thr_coverage", _native.coverage, _native.coverage_times, args, dict(trials=5, keep_count=2, seed=11),
                family=Family("coverage", _native.COVERAGE_OUTPUTS), stops={"no_covered_cell": (None, dict(range_m=1.0))}, n_times=6,
                refusal=Refusal("thr_coverage: trials must lie in 1 ..", kwargs=dict(trials=0)))


def _build():
    cases = list(_identify_cases()) + [_match_case()] + list(_tdoa_cases()) + list(_pos_cases()) + [_postdetect_case()]
    cases += list(_stats_cases()) + list(_quality_cases()) + [_track_case()] + list(_global_cases()) + [_coverage_case()]
    cases += list(_pos3_cases())
    return cases


CASES = _build()
BY_NAME = {case.name: case for case in CASES}
assert len(BY_NAME) == len(CASES)
FAMILIES = [case for case in CASES if case.family]
ENTRIES = sorted({case.entry for case in CASES})


def stops_of(cases=None):
    """(case, stop name) for every early stop, the empty call ("zero") among them."""
    out = []
    for case in (CASES if cases is None else cases):
        out += [(case, "zero")] if case.zero is not None else []
        out += [(case, name) for name in sorted(case.stops)]
    return out


def stop_call(case, name):
    """(args or None, kwargs changes) of an early stop."""
    return case.zero if name == "zero" else case.stops[name]
