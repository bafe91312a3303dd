"""The coverage fixtures (tests/golden/coverage/*.npz, made by tests/golden/make_golden_coverage.py), the scenes the
host and GPU tests of `thr_coverage` share, and the derived bounds they hold the device and the statement to."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "coverage")
SETS = ("ring5", "range6", "far4", "mixed5")
C = 2.997e8
U = 2.0 ** -53
RADIUS = 100.0
# sqrt(-2 ln u1) at the smallest u1 = 2^-32: no normal is larger
R_MAX = float(np.sqrt(64.0 * np.log(2.0)))
_cache = {}


def ring(seed, n_rx, offset=(0.0, 0.0)):
    """The jittered ring of tests/posg_golden.py: radius 100 m, 5 m of jitter."""
    rng = np.random.default_rng(seed)
    ang = np.linspace(0, 2 * np.pi, n_rx, endpoint=False) + 0.3
    return np.c_[np.cos(ang), np.sin(ang)] * RADIUS + rng.normal(0, RADIUS * 0.05, (n_rx, 2)) + np.asarray(offset)


def pos_tolerance():
    """The position tolerance the pos fixtures record: the largest ref_err_max of the ring scenes (some 1e-7 m)."""
    worst = 0.0
    for name in ("pos_ring4", "pos_ring6", "pos_ring8"):
        with np.load(os.path.join(ROOT, "tests", "golden", "pos", name + ".npz")) as g:
            worst = max(worst, float(g["ref_err_max"]))
    return worst


def scenes():
    """name -> the arguments of coverage_ref / _native.coverage (table, sigma, lo, hi, nx, ny, gross_m, trials, range_m,
    seed, x0).  far4 takes the receivers of the posg fixture of that name."""
    with np.load(os.path.join(ROOT, "tests", "golden", "posg", "far4.npz")) as g:
        far = np.array(g["rx_xy"])
    centre = far.mean(axis=0)
    ring5 = ring(3, 5)
    return {
        # small noise, every cell well inside the ring: the prediction must describe the trials
        "ring5": dict(table=ring5, sigma=np.full(5, 0.05), lo=(-40.0, -35.0), hi=(40.0, 35.0), nx=6, ny=5, gross_m=1.0,
                      trials=70, range_m=0.0, seed=0x1234567887654321, x0=(0.1, 0.1)),
        # a range that leaves cells with 0, 2, 3, 4 and 6 hearing receivers (asserted by the generator)
        "range6": dict(table=ring(5, 6), sigma=np.full(6, 0.3), lo=(-330.0, -300.0), hi=(300.0, 310.0), nx=9, ny=8,
                       gross_m=5.0, trials=8, range_m=140.0, seed=7, x0=(0.1, 0.1)),
        # the array far from the origin: the fixed start loses cells
        "far4": dict(table=far, sigma=np.full(4, 0.3), lo=tuple(centre - 50.0), hi=tuple(centre + 50.0), nx=6, ny=6,
                     gross_m=10.0, trials=16, range_m=0.0, seed=11, x0=(0.1, 0.1)),
        # one sigma per receiver, one of them zero
        "mixed5": dict(table=ring5, sigma=np.array([0.05, 0.0, 0.1, 0.05, 0.2]), lo=(-30.0, -20.0), hi=(30.0, 20.0), nx=3,
                       ny=2, gross_m=2.0, trials=8, range_m=0.0, seed=1 << 40, x0=(0.1, 0.1)),
    }


def load(name):
    if name not in _cache:
        with np.load(os.path.join(GOLDEN, name + ".npz")) as g:
            _cache[name] = {key: g[key] for key in g.files}
        for value in _cache[name].values():
            value.setflags(write=False)
    return _cache[name]


def arguments(g):
    """A fixture's scene as keyword arguments of coverage_ref.coverage_ref (and, with lo / hi / nx / ny positional, of
    _native.coverage)."""
    return dict(table=g["table"], sigma=g["sigma"], lo=tuple(g["lo"].tolist()), hi=tuple(g["hi"].tolist()), nx=int(g["nx"]),
                ny=int(g["ny"]), gross_m=float(g["gross_m"]), trials=int(g["trials"]), range_m=float(g["range_m"]),
                seed=int(g["seed"]), x0=tuple(g["x0"].tolist()))


def native_call(g, **changes):
    """_native.coverage on a fixture's scene -> (counts, outputs)."""
    from thrifty_amd import _native
    a = dict(arguments(g), **changes)
    return _native.coverage(a.pop("table"), a.pop("sigma"), a.pop("lo"), a.pop("hi"), a.pop("nx"), a.pop("ny"), a.pop("gross_m"), **a)


# ---------------------------------------------------------------- bounds
def noise_bound(sigma):
    """|n_device - n_statement| per receiver.  z = R c with R = sqrt(-2 log u1), c = cos(6.28.. u2); u1, u2 and the
    product 6.28.. u2 are the same bits on both sides.  Documented errors: log <= 1 ulp, cos <= 2 ulp (device math
    library; glibc is tighter), sqrt and the products correctly rounded.  Per side, with ulp <= 2^-52 relative:
    -2 log u1 carries 2^-52, its square root half of that plus 2^-53 -> R: 2^-52; c: 2 * 2^-52 absolute (|c| <= 1);
    R c: R (2^-52 + 2 * 2^-52) + 2^-53 R; sigma * z: 2^-53 more -> 4 * 2^-52 R per side, 8 * 2^-52 R between the two,
    R <= R_MAX = sqrt(-2 ln 2^-32) = 6.66.  Absolute, proportional to sigma_r; sigma_r = 0 gives 0 exactly."""
    return 8.0 * 2.0 ** -52 * R_MAX * np.asarray(sigma, dtype=np.float64)


def tdoa_bound(sigma, rx0, rx1, tdoa):
    """The distances are the same bits on both sides, so a row differs by its two noises' bounds, through one subtraction,
    one addition and one division (4 roundings of at most the row's own magnitude)."""
    nb = noise_bound(sigma)
    return (nb[rx0] + nb[rx1]) / C * (1 + 2.0 ** -50) + 4 * U * np.abs(tdoa)


def pred_k(m_rows, n_rx):
    return 4.0 * (m_rows + n_rx) + 200.0


def pred_bound(pred, cond, m_rows, n_rx):
    """Forward-error bound of the float64 analytic columns, k 2^-53 cond(N) |value| with k = 4 (m + n_rx) + 200 -> [5]
    (dop, sxx, sxy, syy, rms).  See tests/test_coverage_host.py::test_pred_within_the_forward_bound for the derivation;
    the covariance entries are bounded norm-wise (|value| = sxx + syy, the trace), dop and rms carry half the relative
    error of their squares."""
    dop, sxx, sxy, syy, rms = pred
    e = pred_k(m_rows, n_rx) * U * cond
    return np.array([0.5 * e * abs(dop), e * (sxx + syy), e * (sxx + syy), e * (sxx + syy), 0.5 * e * abs(rms)])


def exact_mean(values):
    """The correctly rounded sum of the float64 `values` (math.fsum), divided by their number."""
    import math
    values = np.asarray(values, dtype=np.float64).tolist()
    return math.fsum(values) / len(values)


def mean_bound(values):
    """pos_golden.snr_bound's form: (m - 1) 2^-53 sum|v| / m, the bound of a float64 mean of m values against the exact
    one for any summation order."""
    v = np.abs(np.asarray(values, dtype=np.float64))
    return (len(v) - 1) * U * float(v.sum()) / len(v)
