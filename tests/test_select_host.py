"""Selection mode BEST on the CPU: the properties of its numpy statement (tests/select_ref.py, what csrc/select.hip is tested
against), the property that motivates the image cells, and the host plumbing of ``selection="best"`` on stand-in engines."""
import os
import re

import numpy as np
import pytest
import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib, config, servo
import select_ref as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_tables(rng, T, n_mutual):
    """nn_1 / nn_2 with exactly the tokens `m` mutual (a permutation among themselves), the rest pointing at a token whose
    nn_2 points elsewhere; sim_1 uniform."""
    ids = rng.permutation(T)
    m, rest = ids[:n_mutual], ids[n_mutual:]
    nn1 = np.zeros(T, np.int64)
    nn2 = np.zeros(T, np.int64)
    targets = rng.permutation(T)
    nn1[m] = targets[:n_mutual]
    nn2[targets[:n_mutual]] = m
    free = targets[n_mutual:]                                    # current-frame tokens no mutual pair uses
    nn1[rest] = rng.choice(targets[:n_mutual], size=len(rest)) if n_mutual else free[rng.integers(0, len(free), len(rest))]
    nn2[free] = rng.choice(m, size=len(free)) if n_mutual else (rest[rng.integers(0, len(rest), len(free))] + 1) % T
    sim = rng.uniform(0.2, 0.95, T).astype(np.float32)
    return nn1, nn2, sim


@pytest.mark.parametrize("T,cells", [(16, 1), (16, 16), (196, 4), (289, 4), (484, 16), (1024, 2)])
def test_order_is_a_permutation_with_class_zero_first(T, cells):
    rng = np.random.default_rng(T + cells)
    nn1, nn2, sim = _random_tables(rng, T, T // 3)
    order = sref.best_order(nn1, nn2, sim, cells)
    assert order.dtype == np.int32 and sorted(order.tolist()) == list(range(T))
    m = sref.mutual_mask(nn1, nn2)
    assert int(m.sum()) == T // 3
    cls = np.where(m, 0, 1)[order]
    assert np.all(np.diff(cls) >= 0)                             # class 1 never precedes class 0


def test_one_cell_is_the_most_similar_mutuals_then_the_rest():
    rng = np.random.default_rng(5)
    T = 196
    nn1, nn2, sim = _random_tables(rng, T, 70)
    m = sref.mutual_mask(nn1, nn2)
    by_sim = np.lexsort((np.arange(T), -sim.astype(np.float64)))
    want = np.concatenate([by_sim[m[by_sim]], by_sim[~m[by_sim]]])
    assert np.array_equal(sref.best_order(nn1, nn2, sim, 1), want)
    assert np.array_equal(sref.selected(nn1, nn2, sim, 24, 1), want[:24])


def test_ties_break_by_id():
    T = 196
    ident = np.arange(T)
    nn1, nn2 = (ident + 1) % T, (ident + 2) % T                  # no token mutual: one class
    sim = np.full(T, 0.5, np.float32)
    assert np.array_equal(sref.best_order(nn1, nn2, sim, 1), ident)
    cell, c = sref.cells_of(T, 4)
    order = sref.best_order(nn1, nn2, sim, 4)
    # equal similarities: rho is the rank by id within the cell, and a round visits the cells' tokens in id order
    cls, _, rho = sref.ranks(nn1, nn2, sim, 4)
    assert np.array_equal(order, np.lexsort((ident, rho)))
    for cid in range(c * c):
        ids = ident[cell == cid]
        assert np.array_equal(rho[ids], np.arange(len(ids)))
    # +0 and -0 are one value
    sim2 = sim.copy()
    sim2[:] = 0.0
    sim2[::2] = -0.0
    assert np.array_equal(sref.best_order(nn1, nn2, sim2, 4), order)


@pytest.mark.parametrize("g,cells", [(14, 4), (17, 4), (22, 16), (4, 16)])
def test_first_picks_lie_in_distinct_cells(g, cells):
    T = g * g
    rng = np.random.default_rng(100 * g + cells)
    nn1, nn2, sim = _random_tables(rng, T, T // 2)
    cell, c = sref.cells_of(T, cells)
    assert c == min(cells, g)
    m = sref.mutual_mask(nn1, nn2)
    non_empty = len(np.unique(cell[m]))
    for k in (5, 24, 130):
        sel = sref.selected(nn1, nn2, sim, k, cells)
        first = sel[:min(k, non_empty)]
        assert len(set(cell[first].tolist())) == len(first), (k, "a cell was visited twice before every cell was visited once")


def test_cells_are_clamped_to_the_grid_and_uneven_when_they_do_not_divide_it():
    cell, c = sref.cells_of(16, 16)
    assert c == 4 and np.array_equal(cell, np.arange(16))        # one cell per token
    cell, c = sref.cells_of(289, 4)
    assert c == 4
    rows = (np.arange(17) * 4) // 17                             # 17 rows over 4 cells: 5, 4, 4, 4
    assert np.bincount(rows).tolist() == [5, 4, 4, 4]
    assert np.array_equal(cell.reshape(17, 17), rows[:, None] * 4 + rows[None, :])
    assert sorted(np.bincount(cell).tolist()) == sorted([a * b for a in (5, 4, 4, 4) for b in (5, 4, 4, 4)])


# ----------------------------------------------------------------------------- why cells: the conditioning of L_e
def _interaction(ids, g, Z=0.6):
    """L_e (2 rows per point) of the patch centres of tokens `ids` on a g x g grid, normalised to the unit square's field of view."""
    r, col = ids // g, ids % g
    x = ((col + 0.5) / g - 0.5) * 1.2
    y = ((r + 0.5) / g - 0.5) * 0.9
    L = np.zeros((2 * len(ids), 6))
    L[0::2] = np.stack([-1 / Z + 0 * x, 0 * x, x / Z, x * y, -(1 + x * x), y], 1)
    L[1::2] = np.stack([0 * x, -1 / Z + 0 * x, y / Z, 1 + y * y, -x * y, -x], 1)
    return L


def test_cells_spread_the_selection_and_condition_the_law_better():
    """T = 196, 24 pairs, 64 seeded tables: 40 mutual matches at similarity 0.90-0.95 inside the corner block (rows 0-6 x columns
    0-6) and 12 at 0.70-0.80 anywhere else.  One cell takes the 24 best, all in the corner; 4 x 4 cells reach the others: the
    smallest singular value of L_e (points at Z = 0.6) is larger in every seed."""
    g, T, k = 14, 196, 24
    ratios = []
    for seed in range(64):
        rng = np.random.default_rng(9000 + seed)
        corner = np.array([r * g + c for r in range(7) for c in range(7)])
        others = np.setdiff1d(np.arange(T), corner)
        a = rng.choice(corner, size=40, replace=False)
        b = rng.choice(others, size=12, replace=False)
        m = np.concatenate([a, b])
        ident = np.arange(T)
        nn1, nn2 = (ident + 1) % T, (ident + 2) % T              # nothing mutual ...
        tgt = rng.permutation(T)[:len(m)]
        nn1[m] = tgt                                             # ... but the planted matches
        nn2[tgt] = m
        # (a planted target may have been some other token's nn_1 before: that token stays non-mutual, nn_2 points at m)
        sim = rng.uniform(0.2, 0.6, T).astype(np.float32)
        sim[a] = rng.uniform(0.90, 0.95, 40).astype(np.float32)
        sim[b] = rng.uniform(0.70, 0.80, 12).astype(np.float32)
        assert set(np.nonzero(sref.mutual_mask(nn1, nn2))[0].tolist()) == set(m.tolist())
        s1 = np.linalg.svd(_interaction(sref.selected(nn1, nn2, sim, k, 1), g), compute_uv=False)[-1]
        s4 = np.linalg.svd(_interaction(sref.selected(nn1, nn2, sim, k, 4), g), compute_uv=False)[-1]
        assert s4 > s1, (seed, s1, s4)
        ratios.append(s4 / s1)
    print(f"smallest singular value of L_e, cells=4 over cells=1: median ratio {np.median(ratios):.2f}, smallest {min(ratios):.2f}")


# ----------------------------------------------------------------------------- host plumbing on stand-in engines
class _HostEngine:
    """Stands in for Engine on Controller's one-call host path."""
    tokens, max_rows, max_pairs = 16, 48, 4
    device = torch.device("cpu")
    frame_size = (8, 8)

    class cfg:
        img_size = 8

    def __init__(self, params):
        self.params = params
        self.calls = []
        self.goals = []
        self.options = []

    def set_frame_size(self, *a):
        return self

    def set_option(self, *a):
        self.options.append(a)
        return self

    def apply_law_params(self, params):
        self.applied = params
        return self

    def compute_velocity_host(self, cur, des, z, K, mode=None, selection=None, n_selected=None, des_shared=False, num_pairs=None):
        self.calls.append(dict(mode=mode, selection=selection, num_pairs=num_pairs))
        self.goals.append((des.ctypes.data, np.array(des, copy=True)))        # the address handed over, and what it held then
        return np.full((1, 6), 0.5), np.zeros(1, np.int32)

    def compute_velocity(self, cur, des, z, K, mode=None, selection=None, des_shared=False, num_pairs=None):
        n = cur.shape[0]
        self.calls.append(dict(n=n, mode=mode, selection=selection, num_pairs=num_pairs))
        return torch.full((n, 6), 0.25, dtype=torch.float64), torch.zeros(n, dtype=torch.int32)

    def last_features(self, n):
        return dict(s_uv=np.zeros((n, 48, 4), np.int32), info=np.zeros((n, 8), np.int32), feat=np.zeros((n, 48, 4)))


def test_controller_best_is_one_host_call_with_no_selection():
    params = config.ServoParams(dino_input_size=8, use_feature_binning=False, num_pairs=5)
    eng = _HostEngine(params)
    frame = np.zeros((8, 8, 3), np.uint8)
    ctl = servo.Controller(eng, frame, selection="best")
    ctl.image_callback_rgb(frame + 3)
    ctl.image_callback_depth(np.ones((params.v_max, params.u_max), np.uint16))
    state = torch.random.get_rng_state()
    ctl.ibvs()
    assert torch.equal(torch.random.get_rng_state(), state)      # nothing was drawn
    assert eng.calls == [dict(mode=_lib.SELECT_BEST, selection=None, num_pairs=5)]
    assert np.array_equal(ctl.v_c, np.full(6, 0.5))


def test_controller_stages_the_goal_it_holds_now():
    """The reference reads ``self.goal_image`` on every update (vitvs_v2.py:482-487).  The controller hands the engine a private copy
    whose ADDRESS tells the library that the goal frame staged before is still the goal (option "reuse_goal_frames"): the copy
    follows the goal's content, not the goal object's id.  An unchanged goal: the same address on every update.  A goal rewritten
    in place, a replacement of equal shape, a goal that returns to an earlier content: an array equal to the goal as it is now,
    with the option set again (which makes the library forget the address staged before, recycled or not)."""
    params = config.ServoParams(dino_input_size=8, use_feature_binning=False, num_pairs=5)
    eng = _HostEngine(params)
    rng = np.random.default_rng(4)
    first, other, third = (rng.integers(0, 256, size=(8, 8, 3), dtype=np.uint8) for _ in range(3))
    goal = first.copy()
    ctl = servo.Controller(eng, goal, selection="best")
    ctl.image_callback_rgb(np.zeros((8, 8, 3), np.uint8) + 3)
    ctl.image_callback_depth(np.ones((params.v_max, params.u_max), np.uint16))

    def update():
        ctl.ibvs()
        return eng.goals[-1]

    addr, held = update()
    assert np.array_equal(held, first) and addr != goal.ctypes.data          # a private copy, not the caller's buffer
    assert eng.options.count(("reuse_goal_frames", 1)) == 1
    for _ in range(3):                                                       # unchanged goal: the same buffer, nothing staged again
        assert update()[0] == addr
    assert eng.options.count(("reuse_goal_frames", 1)) == 1
    goal[...] = other                                                        # rewritten in place: same object, same id, same shape
    addr2, held = update()
    assert np.array_equal(held, other)
    assert eng.options.count(("reuse_goal_frames", 1)) == 2                  # the library forgets the staged address
    assert update()[0] == addr2 and eng.options.count(("reuse_goal_frames", 1)) == 2
    goal[3, 4, 1] ^= 1                                                       # one byte
    assert np.array_equal(update()[1], goal) and eng.options.count(("reuse_goal_frames", 1)) == 3
    ctl.goal_image = third.copy()                                            # a replacement goal of equal shape
    addr3, held = update()
    assert np.array_equal(held, third) and eng.options.count(("reuse_goal_frames", 1)) == 4
    assert update()[0] == addr3
    replacement = third.copy()                                               # another object, equal content: nothing to stage
    ctl.goal_image = replacement
    assert update()[0] == addr3 and eng.options.count(("reuse_goal_frames", 1)) == 4
    ctl.goal_image = first.copy()                                            # back to an earlier content
    assert np.array_equal(update()[1], first) and eng.options.count(("reuse_goal_frames", 1)) == 5


def test_multi_controller_best_calls_once_with_no_selection():
    params = config.ServoParams(dino_input_size=8, use_feature_binning=False, num_pairs=5)
    eng = _HostEngine(params)
    frame = np.zeros((8, 8, 3), np.uint8)
    mc = servo.MultiController(eng, [frame, frame, frame], selection="best")
    for i in (0, 2):
        mc.image_callback_rgb(i, frame + 1)
        mc.image_callback_depth(i, np.ones((params.v_max, params.u_max), np.uint16))
    state = torch.random.get_rng_state()
    mc.ibvs()
    assert torch.equal(torch.random.get_rng_state(), state)
    assert eng.calls == [dict(n=2, mode=_lib.SELECT_BEST, selection=None, num_pairs=5)]
    assert mc.v_c[1] is None and np.array_equal(mc.v_c[0], np.full(6, 0.25))
    with pytest.raises(ValueError):
        servo.MultiController(eng, [frame], selection="reference")


def test_functional_api_passes_best_through():
    params = config.ServoParams(dino_input_size=8, use_feature_binning=False)
    eng = _HostEngine(params)
    frames = np.zeros((2, 8, 8, 3), np.uint8)
    v, st = servo.compute_velocity_batch(eng, frames, frames, None, selection="best", num_pairs=7)
    assert eng.calls == [dict(n=2, mode=_lib.SELECT_BEST, selection=None, num_pairs=7)] and v.shape == (2, 6)


def test_select_cells_is_validated_and_read_from_the_config():
    assert config.ServoParams().select_cells == 4
    for bad in (0, 17, -1):
        with pytest.raises(ValueError, match="select_cells"):
            config.ServoParams(select_cells=bad)
    assert config.ServoParams(select_cells=1).select_cells == 1 and config.ServoParams(select_cells=16).select_cells == 16
    keys = dict(u_max=1280, v_max=720, lambda_=0.01, min_error=100, max_error=70000, f_x=695.9951, f_y=695.9951,
                num_pairs=18, image_path="goal.jpg", dino_input_size=518, thresh_filter_keypoints=1,
                use_feature_binning=False, num_samples=500, num_circles=4, circle_radius_aug=0.08,
                velocity_convergence_threshold=8e-5, velocity_threshold_translation=5e-19,
                velocity_threshold_rotation=5e-19, error_threshold_ratio=0.001,
                error_threshold_absolute_translation=0.1, error_threshold_absolute_rotation=0.1, min_iterations=300,
                max_iterations=700)
    assert config.load_reference_config(keys).servo.select_cells == 4
    rc = config.load_reference_config(dict(keys, select_cells=2))
    assert rc.servo.select_cells == 2 and "select_cells" not in rc.extras
    with pytest.raises(ValueError, match="select_cells"):
        config.load_reference_config(dict(keys, select_cells=17))


def test_the_mode_is_three_in_the_binding_and_in_the_header():
    assert (_lib.SELECT_EXPLICIT, _lib.SELECT_ORDER, _lib.SELECT_DENSE, _lib.SELECT_BEST) == (0, 1, 2, 3)
    with open(os.path.join(ROOT, "include", "vitvs.h")) as fh:
        text = fh.read()
    assert re.search(r"VITVS_SELECT_BEST\s*=\s*3\b", text)
    assert "vitvs_last_order" in _lib.PROTOTYPES and "vitvs_op_best_order_dev" in _lib.PROTOTYPES
