"""The dossier fixtures (tests/golden/dossier/<scene>.npz, made by tests/golden/make_golden_dossier.py from
the reference's recorded drawings) and the comparison of a `Dossier`'s views against them."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SCENES = ("small", "c2", "c2_stddev", "c1")


def load(scene):
    return np.load(os.path.join(HERE, "golden", "dossier", scene + ".npz"), allow_pickle=False)


def load_scene(scene):
    return np.load(os.path.join(HERE, "golden", scene + ".npz"), allow_pickle=False)


def rel_l2(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return float(np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-300))


def view_errors(dossier, fx, k, views=None):
    """Compare kept block `k`'s views with the fixture -> list of (what, relative error); labels, counts and
    lengths are asserted on the way.  Long series are compared where the fixture stores them."""
    out = []
    for v in (views if views is not None else [str(x) for x in fx["views"]]):
        view = dossier.view(v)
        assert [line[0] for line in view.lines] == [str(x) for x in fx[v + "|labels"]], v
        assert [h[0] for h in view.hlines] == [str(x) for x in fx[v + "|hlabels"]], v
        want_h, want_v = fx[v + "|hlines"][k], fx[v + "|vlines"][k]
        assert len(view.vlines) == len(want_v), v
        for (label, value), want in zip(view.hlines, want_h):
            out.append(("%s hline %s" % (v, label), abs(value - want) / abs(want)))
        for (_, value), want in zip(view.vlines, want_v):
            out.append(("%s vline" % v, abs(value - want) / max(abs(want), 1.0)))
        for j, (label, x, y) in enumerate(view.lines):
            want_len = int(fx["%s|%d|len" % (v, j)][k])
            assert len(x) == len(y) == want_len, (v, j, len(x), len(y), want_len)
            key = "%s|%d|y" % (v, j)
            if key not in fx.files or k >= len(fx[key]):
                continue
            wx, wy = fx["%s|%d|x" % (v, j)][k][:want_len], fx[key][k][:want_len]
            out.append(("%s line %d x" % (v, j), rel_l2(x, wx) if np.any(wx) else float(np.max(np.abs(x)))))
            out.append(("%s line %d y" % (v, j), rel_l2(y, wy)))
    return out


_REF = {}


def ref_numbers(scene, **override):
    """dossier_ref.numbers() of every block of a scene, computed once per process and shared (read only)."""
    import dossier_ref as R
    key = (scene, tuple(sorted(override.items())))
    if key not in _REF:
        g = load_scene(scene)
        settings = R.scene_settings(g, **override)
        _REF[key] = (settings, [R.numbers(b, int(i), settings) for i, b in zip(g["block_idx"], g["blocks"])])
    return _REF[key]
