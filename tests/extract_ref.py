"""Plain float64 numpy reference of template extraction's choice and cut -- no engine involved.

The fold and the keep of csrc/template_extract.hip move bytes and indices, so their reference is exact:
numpy on the records a run returned.  The cut's reference is the float64 host formula
thrifty_amd.template_extract.direct_template, which tests/test_template_extract_host.py ties to the
reference's own output.
"""
import numpy as np

from thrifty_amd import _native, template_extract

# Tolerance of a template of W <= 1023 samples against expected_template(), absolute: derived in the
# docstring of tests/test_gpu_template_extract.py.
TOL = 1e-12


def qualifying(records, max_offset):
    """Boolean mask: the correlation stage detected and |corr_offset| <= max_offset (inclusive)."""
    flags = np.asarray(records["flags"])
    offset = np.abs(np.asarray(records["corr_offset"], dtype=np.float64))
    return ((flags & _native.FLAG_CORR) != 0) & (offset <= float(max_offset))


def expected_pick(records, max_offset):
    """`records`: a run's records concatenated in feed order -> (position, n_qualifying): the first
    index of the largest float32 corr_energy among the qualifying records, or None if none qualifies."""
    ok = qualifying(records, max_offset)
    if not ok.any():
        return None
    energy = np.asarray(records["corr_energy"], dtype=np.float32)
    at = np.flatnonzero(ok)
    return int(at[np.argmax(energy[at])]), int(ok.sum())       # (argmax: the first of equals)


def expected_template(block, corr_sample, w):
    return template_extract.direct_template(block, int(corr_sample), int(w))


def window_of(n, h, w):
    """The lags [lo, hi) a block owns (tests/golden/make_golden_template_extract.py: window_of)."""
    pad = h - w + 1
    left = pad // 2
    return left, (n - w + 1) - (pad - left)


def cuts(total, sizes):
    """Batch boundaries: `sizes` is one int (batches of that size) or the list of sizes."""
    sizes = [sizes] * -(-total // sizes) if isinstance(sizes, int) else sizes
    at, out = 0, []
    for s in sizes:
        out.append((at, min(total, at + s)))
        at += s
    assert out[-1][1] == total
    return out


def same(a, b):
    """Two results of the engine: identical record, bit-identical template, same count."""
    return a[0].tobytes() == b[0].tobytes() and a[2].tobytes() == b[2].tobytes() and a[3] == b[3]
