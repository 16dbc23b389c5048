"""The cases of tests/test_gpu_homography_consensus_op.py and their fp64 references (tests/homography_consensus_ref.py), shared with
tests/test_homography_consensus_host.py, which checks on the CPU that every case keeps its margins: then the GPU test leaves no
case out.  The generators restate those of tests/test_gpu_homography_op.py.

Shapes, the smallest at which the consensus phase can go wrong: ld 4 (one row set), 5, 24, 48, 257 and 300 (past the 256-thread
stride of the weight pass), 1 and 3 pairs with different usable counts, unusable rows first / in the middle / last, a row the winner
maps behind the camera, an exactly collinear set (every hypothesis skipped), 3 usable rows (no hypothesis at all); with 1 (part of a
round), 64, 256 (one round), 257 (one hypothesis into the second round) and 512 hypotheses, and 0 and 4 re-weightings behind them."""
import numpy as np

import homography_consensus_ref as cr
import homography_ref as hr

LAM = 0.35
ZHAT = 0.61
SMIN = 0.004
SEED = 1                 # (under this seed every case keeps the margins tests/test_homography_consensus_host.py asks for)
N_HYPS = (1, 64, 256, 257, 512)
N_ITERS = (0, 4)


def pair(seed, rows, usable=None, outliers=0, noise=0.002, rot=0.3):
    """One pair's (m, ms, usable): a seeded pose, points on the plane z = 0.61 seen from it (+ noise) and from the goal, `outliers`
    usable rows moved by 0.1 - 0.4 per axis."""
    rng = np.random.default_rng(seed)
    R, t = hr.rodrigues(rng.normal(0.0, rot, 3)), rng.normal(0.0, 0.05, 3)
    X = np.stack([rng.uniform(-0.3, 0.3, rows), rng.uniform(-0.3, 0.3, rows), np.full(rows, 0.61)], 1)
    m, ms = hr.project(X, R, t) + rng.standard_normal((rows, 2)) * noise, X[:, :2] / 0.61
    usable = np.ones(rows, np.int32) if usable is None else np.asarray(usable, np.int32)
    live = np.nonzero(usable > 0)[0]
    if outliers:
        bad = rng.choice(live, outliers, replace=False)
        m[bad] += rng.uniform(0.1, 0.4, (outliers, 2)) * rng.choice([-1.0, 1.0], (outliers, 2))
    m[usable <= 0], ms[usable <= 0] = 0.0, 0.0
    return m, ms, usable


def flags(rows, where, n_off):
    """`n_off` unusable rows first / in the middle / last (flags 0 and -1 alternate: both mean unusable)."""
    u = np.ones(rows, np.int32)
    start = {"first": 0, "middle": (rows - n_off) // 2, "last": rows - n_off}[where]
    u[start:start + n_off] = np.where(np.arange(n_off) % 2 == 0, 0, -1)
    return u


def case(*pairs, degenerate=False):
    m, ms, u = (np.stack(x) for x in zip(*pairs))
    return dict(m=m, ms=ms, usable=u, degenerate=degenerate)


def collinear(rows):
    """Points of one line of the plane, seen from a seeded pose and from the goal."""
    s = np.linspace(-0.3, 0.3, rows)
    X = np.stack([s, 0.05 - 0.6 * s, np.full(rows, 0.61)], 1)
    R, t = hr.rodrigues([0.1, -0.2, 0.3]), np.array([0.03, -0.02, 0.04])
    return hr.project(X, R, t), X[:, :2] / 0.61


BEHIND_ROW = 5


def behind():
    """24 noisy rows of which one current point lies so far out that the homography of the others maps it behind the camera."""
    _, ms, u = pair(12, 24, rot=0.0)
    R, t = hr.rodrigues([0.0, 0.5, 0.0]), np.array([0.02, -0.01, 0.03])
    X = np.concatenate([ms * 0.61, np.full((24, 1), 0.61)], 1)
    m = hr.project(X, R, t) + np.random.default_rng(13).standard_normal((24, 2)) * 0.002
    m[BEHIND_ROW] = (6.0, 0.3)
    return m, ms, u


def _cases():
    out = {}
    out["1x4"] = case(pair(1, 4))
    out["1x5"] = case(pair(2, 5))
    out["3x24"] = case(pair(3, 24, flags(24, "first", 5), outliers=6),                   # 19 usable
                       pair(4, 24, flags(24, "middle", 4), outliers=5),                  # 20 usable
                       pair(5, 24, flags(24, "last", 3)))                                # 21 usable
    out["1x48"] = case(pair(6, 48, outliers=16))
    out["1x257"] = case(pair(7, 257, flags(257, "middle", 9), outliers=80))
    out["3x300"] = case(pair(8, 300, flags(300, "first", 3), outliers=90),
                        pair(9, 300, flags(300, "last", 41), outliers=60),
                        pair(10, 300, flags(300, "middle", 11)))
    out["1x24_behind"] = case(behind())
    out["1x24_three_usable"] = case(pair(9, 24, flags(24, "first", 21)), degenerate=True)
    m, ms = collinear(24)
    out["1x24_collinear"] = case((m, ms, np.ones(24, np.int32)), degenerate=True)
    return out


CASES = _cases()
_REFS = {}


def reference(name, n_hyp, n_iter):
    """One fp64 reference per (case, hypotheses, N), computed once and shared."""
    key = (name, n_hyp, n_iter)
    if key not in _REFS:
        c = CASES[name]
        _REFS[key] = [cr.homography_consensus_law(c["m"][b], c["ms"][b], c["usable"][b], LAM, ZHAT, n_iter, SMIN, n_hyp, SEED)
                      for b in range(len(c["m"]))]
    return _REFS[key]
