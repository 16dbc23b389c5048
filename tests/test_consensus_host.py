"""What the consensus starts of the pose law and the homography law share, on the CPU: the draw of
tests/consensus_ref.py against its rule in plain integers, for the three rows of a pose hypothesis and the four of a homography."""
from __future__ import annotations

import numpy as np
import pytest

import consensus_ref as cs
import homography_consensus_ref as hcr
import pose_consensus_ref as pcr


def _mix(x):
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    return x ^ (x >> 16)


@pytest.mark.parametrize("k", [3, 4])
def test_the_draw(k):
    """k distinct positions below n_us for n_us in k .. 300 and j < 4096 (none skipped there), a function of (seed, j, n_us) alone,
    and the rule as stated, in plain integers; the laws' own draws are this one at their k."""
    for n_us in range(k, 301):
        pos, ok = cs.draw(0, 4096, n_us, k)
        assert ok.all(), n_us
        assert (pos >= 0).all() and (pos < n_us).all() and (np.diff(pos, axis=1) > 0).all(), n_us
    for seed, n_us in ((0, k), (1, k + 1), (0xFFFFFFFF, 24), (123456789, 297)):
        pos, ok = cs.draw(seed, 300, n_us, k)
        again, _ = cs.draw(seed, 100, n_us, k)                   # (not of the number of hypotheses)
        assert np.array_equal(pos[:100], again)
        for j in (0, 1, 99, 299):
            base, got, c = _mix((seed * 0x9E3779B9 + j) & 0xFFFFFFFF), [], 0
            while len(got) < k:
                r = _mix((base + c) & 0xFFFFFFFF) % n_us
                c += 1
                if r not in got:
                    got.append(r)
            assert c <= 64 and sorted(got) == list(pos[j]), (seed, n_us, j)
        law = (pcr if k == 3 else hcr).draw(seed, 300, n_us)
        assert np.array_equal(law[0], pos) and np.array_equal(law[1], ok)
    assert not np.array_equal(cs.draw(0, 64, 24, k)[0], cs.draw(1, 64, 24, k)[0])
    assert not np.array_equal(cs.draw(0, 64, 24, k)[0], cs.draw(0, 64, 25, k)[0])
