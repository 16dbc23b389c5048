"""The roll search in numpy: the statement csrc/roll.hip is tested against.

A quarter turn of a square frame is lossless, and with a token grid that is symmetric under it ((S - patch) % stride == 0) the
token at position o of the copy turned by k quarter turns is token P_k[o] of the unturned frame,

    P_k = numpy.rot90(arange(T).reshape(g, g), k).reshape(-1).

Candidate k is the current frame turned by k quarter turns (``numpy.rot90(frame, k)``) matched against the goal.  Its score is the
fp64 mean of sim_1 over its mutual nearest neighbours; it is valid when 0 < n_mutual < T (the law's own "none" rule) or under the
law's same-image shortcut; the winner is the largest score, the smallest k on an exact tie, -1 when nobody is valid.  The winner's
tables are carried back into the unturned frame: nn_1'[i] = P[nn_1[i]], nn_2'[P[j]] = nn_2[j], sim_1' = sim_1.
"""
from __future__ import annotations

import numpy as np


def perm(g: int, k: int) -> np.ndarray:
    """P_k [T]: the unturned frame's token at every position of the copy turned by k quarter turns."""
    return np.rot90(np.arange(g * g).reshape(g, g), k).reshape(-1)


def perm_closed_form(g: int, k: int) -> np.ndarray:
    """P_k as the kernel computes it, position by position."""
    o = np.arange(g * g)
    r, c = o // g, o % g
    return [o, c * g + (g - 1 - r), (g - 1 - r) * g + (g - 1 - c), (g - 1 - c) * g + r][k % 4]


def same_image(sim_1: np.ndarray) -> bool:
    """The law's shortcut test, mean(sim_1) > 0.99 in fp32, summed as servo.hip sums it: thread t of 256 adds entries t, t + 256,
    ... in order, every wave of 64 threads is a balanced binary tree over adjacent lanes, the four waves are added in order."""
    s = np.asarray(sim_1, np.float32).reshape(-1)
    T = s.size
    rows = np.zeros(((T + 255) // 256) * 256, np.float32)
    rows[:T] = s
    acc = np.zeros(256, np.float32)
    for row in rows.reshape(-1, 256):
        acc = acc + row
    v = acc.reshape(4, 64)
    while v.shape[1] > 1:
        v = v[:, 0::2] + v[:, 1::2]
    f = v[:, 0]
    total = np.float32(np.float32(np.float32(f[0] + f[1]) + f[2]) + f[3])
    return bool(np.float32(total / np.float32(T)) > np.float32(0.99))


def mutual(nn_1: np.ndarray, nn_2: np.ndarray) -> np.ndarray:
    """The tokens i with 0 <= nn_1[i] < T and nn_2[nn_1[i]] == i, as a mask."""
    nn_1, nn_2 = np.asarray(nn_1, np.int64), np.asarray(nn_2, np.int64)
    T = nn_1.size
    inside = (nn_1 >= 0) & (nn_1 < T)
    return inside & (nn_2[np.clip(nn_1, 0, T - 1)] == np.arange(T))


def candidate(nn_1, nn_2, sim_1) -> dict:
    """n_mutual, same_image, valid and score (NaN: not valid, or nothing to average) of one candidate's tables."""
    m = mutual(nn_1, nn_2)
    n, T = int(m.sum()), m.size
    same = same_image(sim_1)
    valid = same or 0 < n < T
    score = float(np.asarray(sim_1, np.float32)[m].astype(np.float64).mean()) if valid and n > 0 else float("nan")
    return dict(n_mutual=n, same_image=same, valid=valid, score=score)


def remap(nn_1, nn_2, sim_1, g: int, k: int):
    """Candidate k's tables carried back into the unturned frame.  Entries of nn_1 outside 0 .. T - 1 stay as they are."""
    nn_1, nn_2 = np.asarray(nn_1), np.asarray(nn_2)
    T = g * g
    P = perm(g, k)
    inside = (nn_1 >= 0) & (nn_1 < T)
    out_1 = np.where(inside, P[np.clip(nn_1, 0, T - 1)], nn_1).astype(nn_1.dtype)
    out_2 = np.empty_like(nn_2)
    out_2[P] = nn_2
    return out_1, out_2, np.array(sim_1, copy=True)


def pick(nn_1, nn_2, sim_1, g: int) -> dict:
    """The pick over the four candidates' tables [4][T] -> dict(roll (k*, -1: nobody valid), scores [4], n_mutual [4], same_image
    (of k*), roll_info [8] as the kernel writes it, nn_1 / nn_2 / sim_1: pair 0's tables afterwards)."""
    cands = [candidate(nn_1[k], nn_2[k], sim_1[k]) for k in range(4)]
    best = -1
    for k, c in enumerate(cands):
        if not np.isnan(c["score"]) and (best < 0 or c["score"] > cands[best]["score"]):
            best = k
    t1, t2, s1 = remap(nn_1[max(best, 0)], nn_2[max(best, 0)], sim_1[max(best, 0)], g, max(best, 0))
    same = bool(best >= 0 and cands[best]["same_image"])
    n_mutual = np.array([c["n_mutual"] for c in cands], np.int32)
    info = np.array([best, *n_mutual, int(same), 0, 0], np.int32)
    return dict(roll=best, scores=np.array([c["score"] for c in cands]), n_mutual=n_mutual, same_image=same, roll_info=info,
                nn_1=t1, nn_2=t2, sim_1=s1)


def turned_tables(nn_1, nn_2, g: int, k: int):
    """The inverse of ``remap`` for the index tables: what a matcher sees in the copy turned by k quarter turns when the unturned
    frame's tables are nn_1 (goal token -> current token) and nn_2 (current token -> goal token)."""
    P = perm(g, k)
    inv = np.empty_like(P)
    inv[P] = np.arange(P.size)
    return inv[np.asarray(nn_1)], np.asarray(nn_2)[P]
