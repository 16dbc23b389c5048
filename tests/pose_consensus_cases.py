"""The cases of tests/test_gpu_pose_consensus_op.py and their fp64 references (tests/pose_consensus_ref.py), shared with
tests/test_pose_consensus_host.py, which checks on the CPU that every case keeps its margins: then the GPU test leaves no case out.
The generator restates that of tests/test_gpu_pose_op.py.

Shapes, the smallest at which the consensus phase can go wrong: ld 3 (one row set), 4, 24, 48, 257 and 300 (past the 256-thread
stride of the weight pass and past four 64-row steps of the list), 1 and 3 pairs with different usable counts, unusable rows (padded
ones and holes) first / in the middle / last, an exactly collinear cloud (every hypothesis skipped: the start without consensus), 2
usable rows (no hypothesis at all); with 1 (part of a round), 64, 256 (one round), 257 (one hypothesis into the second round) and
512 hypotheses, and 0 and 4 re-weightings behind them."""
import numpy as np

import pose_consensus_ref as cr
import pose_ref as pr

LAM = 0.35
SMIN = 0.019             # the default configuration's floor at the clouds' median depth: T = 4.6851 SMIN = 8.9 cm
SEED = 1                 # (under this seed every case keeps the margins tests/test_pose_consensus_host.py asks for)
N_HYPS = (1, 64, 256, 257, 512)
N_ITERS = (0, 4)


def pair(seed, rows, angle=0.4, usable=None, outliers=0, noise=0.002):
    """One pair's (P, Q, usable): a seeded pose at the given rotation angle, Q at 0.5 - 0.8 m, P = the same points in the camera +
    noise, `outliers` usable rows moved by 0.15 - 0.4 m."""
    rng = np.random.default_rng(seed)
    R, t = pr.rodrigues(pr.unit(rng.standard_normal(3)) * angle), rng.uniform(-0.08, 0.08, 3)
    Z = rng.uniform(0.5, 0.8, rows)
    Q = np.stack([rng.uniform(-0.4, 0.4, rows) * Z, rng.uniform(-0.3, 0.3, rows) * Z, Z], 1)
    P = pr.points_in_camera(Q, R, t) + rng.standard_normal((rows, 3)) * noise
    usable = np.ones(rows, np.int32) if usable is None else np.asarray(usable, np.int32)
    live = np.nonzero(usable > 0)[0]
    if outliers:
        bad = rng.choice(live, outliers, replace=False)
        P[bad] += np.stack([pr.unit(d) for d in rng.standard_normal((outliers, 3))]) * rng.uniform(0.15, 0.4, (outliers, 1))
    P[usable <= 0], Q[usable <= 0] = 0.0, 0.0
    return P, Q, usable


def case(*pairs, degenerate=False):
    P, Q, u = (np.stack(x) for x in zip(*pairs))
    return dict(P=P, Q=Q, usable=u, degenerate=degenerate)


def collinear(rows):
    line = np.outer(np.linspace(-0.3, 0.3, rows), pr.unit([1.0, -1.0, 0.2])) + np.array([0.0, 0.0, 0.6])
    R, t = pr.rodrigues(pr.unit([0.2, 0.5, -0.3]) * 0.5), np.array([0.03, -0.02, 0.04])
    return pr.points_in_camera(line, R, t), line


def _cases():
    out = {}
    out["1x3"] = case(pair(1, 3, 1.0))
    out["1x4"] = case(pair(2, 4, 2.0))
    out["3x24"] = case(pair(3, 24, 0.4, pr.unusable_flags(24, "first", 5), outliers=8),              # 19 usable
                       pair(4, 24, 2.0, pr.unusable_flags(24, "middle", 4), outliers=6),             # 20 usable
                       pair(5, 24, 3.0, pr.unusable_flags(24, "last", 3)))                           # 21 usable
    out["1x48"] = case(pair(6, 48, 0.7, outliers=20))
    out["1x257"] = case(pair(7, 257, 1.3, pr.unusable_flags(257, "middle", 9), outliers=100))
    out["3x300"] = case(pair(8, 300, 0.2, pr.unusable_flags(300, "first", 3), outliers=120),
                        pair(9, 300, 2.5, pr.unusable_flags(300, "last", 41), outliers=80),
                        pair(10, 300, 1.0, pr.unusable_flags(300, "middle", 11)))
    out["1x24_two_usable"] = case(pair(11, 24, 0.5, pr.unusable_flags(24, "first", 22)), degenerate=True)
    P, Q = collinear(24)
    out["1x24_collinear"] = case((P, Q, np.ones(24, np.int32)), degenerate=True)
    return out


CASES = _cases()
_REFS = {}


def reference(name, n_hyp, n_iter):
    """One fp64 reference per (case, hypotheses, N), computed once and shared."""
    key = (name, n_hyp, n_iter)
    if key not in _REFS:
        c = CASES[name]
        with np.errstate(all="ignore"):
            _REFS[key] = [cr.pose_consensus_law(c["P"][b], c["Q"][b], c["usable"][b], LAM, n_iter, SMIN, n_hyp, SEED)
                          for b in range(len(c["P"]))]
    return _REFS[key]
