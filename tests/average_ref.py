"""The averaged template's statement (include/thrifty_hip.h, "Averaged templates") in plain Python integers and
float64 NumPy -- no engine involved.

The sums are exact integers, so their reference is exact: math.isqrt on Python integers, over the records a run
returned (tests/extract_ref.qualifying is the extraction's rule).  The finish restates the extraction kernel's
arithmetic with NumPy's own sums; the device sums in a fixed tree, so the template and the standard error are
compared within the bound tests/test_gpu_template_extract.py uses for the cut.
"""
import math

import numpy as np

from extract_ref import qualifying

E_UNIT = 671088640.0      # 2^20 * 640: what e counts in
Q_UNIT = 409600.0         # 640^2: what q counts in
MAX_CLASSES = 16


def q_table():
    """q of every byte pair, [256 (bI)][256 (bQ)] int64: (5 bI - 637)^2 + (5 bQ - 637)^2."""
    d = (5 * np.arange(256, dtype=np.int64) - 637) ** 2
    return d[:, None] + d[None, :]


def e_of_q(q):
    """floor(sqrt(q * 2^40)) of one Python integer, exactly."""
    return math.isqrt(int(q) << 40)


_tables = {}


def tables():
    """-> (q[256][256] int64, e[256][256] int64), built once: math.isqrt on every distinct q."""
    if not _tables:
        q = q_table()
        roots = {int(v): e_of_q(v) for v in np.unique(q)}
        _tables["q"] = q
        _tables["e"] = np.vectorize(roots.__getitem__, otypes=[np.int64])(q)
    return _tables["q"], _tables["e"]


def class_of(value, classes):
    """The LAST k with lo[k] <= value <= hi[k]; no range given: 0; no match: -1."""
    if len(classes) == 0:
        return 0
    k = -1
    for c, (lo, hi) in enumerate(classes):
        if float(lo) <= value <= float(hi):
            k = c
    return k


def record_value(rec):
    return float(np.float64(rec["carrier_bin"]) + np.float64(rec["carrier_offset"]))


def accumulate(blocks, records, w, max_offset, classes=()):
    """`blocks` u8 [B][2N] and the records the engine returned for them, in any order ->
    (acc_e [K][w], acc_q [K][w], count [K], n_unclassified) as uint64 / Python ints, K = max(1, len(classes))."""
    q_tab, e_tab = tables()
    n_k = max(1, len(classes))
    acc_e = np.zeros((n_k, w), dtype=np.uint64)
    acc_q = np.zeros((n_k, w), dtype=np.uint64)
    count = [0] * n_k
    n_unclassified = 0
    for b in np.flatnonzero(qualifying(records, max_offset)):
        k = class_of(record_value(records[b]), classes)
        if k < 0:
            n_unclassified += 1
            continue
        s = int(records[b]["corr_sample"])
        pairs = np.asarray(blocks[b], dtype=np.uint8)[2 * s:2 * (s + w)].reshape(w, 2)
        acc_e[k] += e_tab[pairs[:, 0], pairs[:, 1]].astype(np.uint64)
        acc_q[k] += q_tab[pairs[:, 0], pairs[:, 1]].astype(np.uint64)
        count[k] += 1
    return acc_e, acc_q, count, n_unclassified


def finish(acc_e, acc_q, count):
    """One class's sums -> (template, sem, scale), float64."""
    cnt = np.float64(count)
    m = acc_e.astype(np.float64) / (cnt * E_UNIT)
    scale = 2.0 / (m.mean() + m.std())
    template = m * scale
    template = template - template.mean()
    var = np.maximum(acc_q.astype(np.float64) / (cnt * Q_UNIT) - m * m, 0.0)
    return template, np.sqrt(var / cnt) * scale, scale


def benefit_capture(seed=20, n_tx=64, amp=0.3, sigma=0.04):
    """A synthetic capture made for extraction, at the geometry of fixture extract_1024 (N 1024, H 512, W 127):
    one transmitter sends the fixture's Gold waveform, low-pass filtered ([1 2 1] / 4: the edges a real
    transmitter's filter leaves), `n_tx` times as an OOK burst on a carrier, each in a block of its own with fresh
    receiver noise.  -> dict: blocks u8 [n_tx][2N], position [n_tx], base (the unfiltered template a detector
    starts from), clean (the noise-free envelope, scaled and centred like a template), n, h, w."""
    import conftest
    from thrifty_amd import synth
    from extract_ref import window_of
    g = conftest.load_golden("template_extract/extract_1024")
    base = np.asarray(g["template"], dtype=np.float64)
    n, h, w = int(g["block_len"]), int(g["history_len"]), len(base)
    shaped = np.convolve(np.concatenate([base[:1], base, base[-1:]]), [0.25, 0.5, 0.25], mode="valid")
    rng = np.random.default_rng(seed)
    blocks, truth = synth.synth_blocks(rng, n_tx, n, shaped, window_of(n, h, w), amp=amp, sigma=sigma,
                                       carriers=rng.uniform(29.9, 30.1, n_tx))
    envelope = amp * (shaped + 1) / 2
    clean = envelope * (2.0 / (envelope.mean() + envelope.std()))
    return {"blocks": blocks, "position": truth["position"], "base": base, "clean": clean - clean.mean(),
            "n": n, "h": h, "w": w}


def fit_error(template, clean):
    """r.m.s. of template * a - clean at the scalar a that makes it smallest."""
    template, clean = np.asarray(template, dtype=np.float64), np.asarray(clean, dtype=np.float64)
    a = float(np.dot(template, clean) / np.dot(template, template))
    return float(np.sqrt(np.mean((template * a - clean) ** 2)))


def tolerance(w, values):
    """The cut's bound of tests/test_gpu_template_extract.py: a float64 sum of w terms, never below 1e-12."""
    return max(1e-12, 4 * w * 2.0 ** -53 * float(np.max(np.abs(values))))
