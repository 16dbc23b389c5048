"""The roll search without a GPU: the token permutation of a quarter turn, the carry-back, the evidence the search
rests on (the CPU oracle's forward on the closed-loop tests' weights and scene), the geometry of an exact quarter turn through
the pose law's numpy statement, and the controllers' refusals."""
import numpy as np
import pytest
import torch
from PIL import Image

import vitvs_amd  # noqa: F401
from vitvs_amd import config, servo, synth, weights
from oracle import servo_ref as sr
from oracle import vit_ref
import closed_loop as cl
import pose_ref as pr
import robust_ref as rr
import roll_ref as rf
from planar_sim import PlanarScene, rodrigues


@pytest.mark.parametrize("g", [1, 2, 4, 14, 37])
def test_the_token_permutation_of_a_quarter_turn(g):
    T = g * g
    ids = np.arange(T).reshape(g, g)
    for k in range(4):
        P = rf.perm(g, k)
        assert np.array_equal(P, np.rot90(ids, k).reshape(-1))
        assert np.array_equal(rf.perm_closed_form(g, k), P), (g, k)
        assert sorted(P.tolist()) == list(range(T))
        # a frame whose every patch is painted with its token id: turning the frame moves the ids as P says
        patch = 3
        frame = np.kron(ids, np.ones((patch, patch), np.int64))
        turned = np.rot90(frame, k)
        assert np.array_equal(turned[patch // 2::patch, patch // 2::patch].reshape(-1), P)
    # the carry-back of a planted permutation table gives back the planted table
    rng = np.random.default_rng(g)
    nn_1 = rng.permutation(T)                                    # goal token -> current token, in the unturned frame
    nn_2 = np.empty(T, np.int64)
    nn_2[nn_1] = np.arange(T)
    sim = rng.uniform(0.3, 0.9, T).astype(np.float32)
    for k in range(4):
        t1, t2 = rf.turned_tables(nn_1, nn_2, g, k)              # what a perfect matcher sees in the turned copy
        assert rf.mutual(t1, t2).all()
        b1, b2, s = rf.remap(t1, t2, sim, g, k)
        assert np.array_equal(b1, nn_1) and np.array_equal(b2, nn_2) and np.array_equal(s, sim)
    # entries outside 0 .. T - 1 are never mutual and stay as they are
    wild = nn_1.copy()
    wild[0] = T + 5
    assert not rf.mutual(wild, nn_2)[0] and rf.remap(wild, nn_2, sim, g, 1)[0][0] == T + 5


def test_pick_rules():
    g, T = 4, 16
    ident = np.arange(T)
    none_1, none_2 = (ident + 1) % T, (ident + 2) % T
    half = ident.copy()
    half[8:] = (ident[8:] + 1) % T                               # 8 mutual tokens
    half_2 = ident.copy()
    sim = np.full(T, 0.5, np.float32)
    # invalid: nothing mutual, everything mutual; valid: some mutual; the same image with everything mutual
    c = [rf.candidate(none_1, none_2, sim), rf.candidate(ident, ident, sim), rf.candidate(half, half_2, sim),
         rf.candidate(ident, ident, np.full(T, 0.995, np.float32))]
    assert [x["valid"] for x in c] == [False, False, True, True] and [x["n_mutual"] for x in c] == [0, T, 8, T]
    assert np.isnan(c[0]["score"]) and np.isnan(c[1]["score"]) and c[2]["score"] == 0.5 and c[3]["same_image"]
    # the largest score wins, the smallest k on an exact tie, -1 when nobody is valid
    hi = np.full(T, 0.75, np.float32)
    p = rf.pick(np.stack([half, half, half, half]), np.stack([half_2] * 4), np.stack([sim, hi, sim, hi]), g)
    assert p["roll"] == 1 and p["scores"][1] == p["scores"][3] == 0.75
    assert np.array_equal(p["nn_1"], rf.perm(g, 1)[half])
    p = rf.pick(np.stack([none_1, ident, none_1, ident]), np.stack([none_2, ident, none_2, ident]), np.stack([sim] * 4), g)
    assert p["roll"] == -1 and np.isnan(p["scores"]).all() and np.array_equal(p["nn_1"], none_1) and p["roll_info"][0] == -1
    # the fp32 mean of the shortcut, summed in the kernel's order, on either side of 0.99
    assert not rf.same_image(np.full(3136, 0.99, np.float32)) and rf.same_image(np.full(3136, 0.9900001, np.float32))


# ----------------------------------------------------------------------------- the evidence, as a test
KEY = "vits16_224"
_WORLD = {}


def _world():
    if not _WORLD:
        cfg = config.baseline_config(KEY)
        _WORLD.update(cfg=cfg, sd=weights.synthetic_state_dict(cfg, 0), tex=synth.texture(128, 11))
    return _WORLD["cfg"], _WORLD["sd"], _WORLD["tex"]


def _square(frame, S):
    """The reference's resize in front of the path: PIL's default (bicubic) to S x S."""
    if frame.shape[:2] == (S, S):
        return frame
    return np.asarray(Image.fromarray(frame).resize((S, S)), dtype=np.uint8)


def _inlier_share(nn_1, nn_2, g, S, params, R, t):
    """Of the mutual matches (tables in the UNTURNED current frame), the share whose current-side pixel lies within one patch pitch
    of where the plane puts the goal-side pixel: (mutual matches, share)."""
    ids = np.nonzero(rf.mutual(nn_1, nn_2))[0]
    if len(ids) == 0:
        return 0, 0.0
    goal_uv = rr.token_pixels(ids, g, S, params.u_max, params.v_max).astype(np.float64)
    cur_uv = rr.token_pixels(nn_1[ids], g, S, params.u_max, params.v_max).astype(np.float64)
    fx, fy, cx, cy = params.intrinsics()
    X = np.stack([(goal_uv[:, 0] - cx) / fx, (goal_uv[:, 1] - cy) / fy, np.ones(len(ids))], 1) * cl.PLANE_Z   # on the plane, goal frame
    Xc = pr.points_in_camera(X, R, t)
    true_uv = np.stack([fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy], 1)
    pitch_u, pitch_v = 16.0 * params.u_max / S, 16.0 * params.v_max / S
    d = np.hypot((cur_uv[:, 0] - true_uv[:, 0]) / pitch_u, (cur_uv[:, 1] - true_uv[:, 1]) / pitch_v)
    return len(ids), float((d <= 1.0).mean())


@pytest.mark.parametrize("camera", [(480, 480), (640, 480)])
def test_the_search_finds_the_quadrant_and_better_matches(camera):
    """Oracle forward, ViT-S/16 224², synthetic weights, the 128-px texture of the closed-loop tests, the start pose of those tests
    composed with a roll about the optical axis.  At 95, 180 and 275 degrees the winner must be k = 3, 2 and 1, and the winner's
    inlier share must exceed the unsearched candidate's (k = 0) by at least 0.15.  The gaps measured when the search was proposed were
    0.27 .. 0.52 for these cases; the bar is half the smallest, so the fp32 rounding of another thread count cannot flip it."""
    cfg, sd, tex = _world()
    S, g = cfg.img_size, cfg.grid
    params = config.ServoParams(dino_input_size=S, use_feature_binning=False, u_max=camera[0], v_max=camera[1])
    scene = PlanarScene(tex, cl.SPAN / tex.shape[0], params, plane_z=cl.PLANE_Z, device="cpu")
    goal = _square(scene.render(np.eye(3), np.zeros(3))[0], S)
    R0, t0 = cl.start_pose()
    for roll, want in ((95.0, 3), (180.0, 2), (275.0, 1)):
        R = R0 @ rodrigues(np.array([0.0, 0.0, np.deg2rad(roll)]))
        cur = _square(scene.render(R, t0)[0], S)
        frames = np.stack([goal] + [np.ascontiguousarray(np.rot90(cur, k)) for k in range(4)])
        toks = vit_ref.block_tokens(sd, frames, patch=cfg.patch, stride=cfg.stride, heads=cfg.heads, layer=cfg.layer, mean=cfg.mean,
                                    std=cfg.std)[:, 1:]
        nn_1, nn_2, sim_1 = [], [], []
        for k in range(4):
            s1, n1, _, n2 = sr.nearest_neighbours(sr.cosine_matrix(toks[0], toks[1 + k], exact_order=False))
            nn_1.append(n1.numpy()), nn_2.append(n2.numpy()), sim_1.append(s1.numpy())
        nn_1, nn_2, sim_1 = np.stack(nn_1), np.stack(nn_2), np.stack(sim_1)
        p = rf.pick(nn_1, nn_2, sim_1, g)
        n0, share0 = _inlier_share(nn_1[0], nn_2[0], g, S, params, R, t0)
        nw, sharew = _inlier_share(p["nn_1"], p["nn_2"], g, S, params, R, t0)
        print(f"camera {camera[0]}x{camera[1]}, roll {roll:.0f} deg: winner k = {p['roll']}, scores {np.round(p['scores'], 4)}, "
              f"inlier share unsearched {share0:.2f} ({n0} mutual) -> winner {sharew:.2f} ({nw} mutual)")
        assert p["roll"] == want, (camera, roll, p["scores"])
        assert sharew - share0 >= 0.15, (camera, roll, share0, sharew)


# ----------------------------------------------------------------------------- an exact quarter turn
@pytest.mark.parametrize("g", [4, 14])
def test_an_exact_quarter_turn_through_the_pose_law(g):
    """A square camera exactly a quarter turn from the goal over a fronto-parallel plane: its frame is rot90(goal, 1), candidate 3
    IS the goal image, and a perfect matcher gives candidate 3 the identity tables.  Carried back and aligned, they say: 90 degrees
    about the optical axis.  The same tables as they are (the shortcut pairing every token with itself) say: at the goal."""
    T, S = g * g, 16 * g
    params = config.ServoParams(dino_input_size=S, u_max=480, v_max=480)
    fx, fy, cx, cy = params.intrinsics()
    ident = np.arange(T)
    cand = [rf.turned_tables(rf.perm(g, 3), np.argsort(rf.perm(g, 3)), g, k) for k in range(4)]      # the truth, seen in each copy
    assert np.array_equal(cand[3][0], ident) and np.array_equal(cand[3][1], ident)
    nn_1, nn_2, _ = rf.remap(ident, ident, np.ones(T, np.float32), g, 3)
    assert np.array_equal(nn_1, rf.perm(g, 3))

    def align(table):
        goal_uv = rr.token_pixels(ident, g, S, 480, 480).astype(np.float64)
        cur_uv = rr.token_pixels(table, g, S, 480, 480).astype(np.float64)
        Z = 0.61
        Q = np.stack([(goal_uv[:, 0] - cx) / fx, (goal_uv[:, 1] - cy) / fy, np.ones(T)], 1) * Z
        P = np.stack([(cur_uv[:, 0] - cx) / fx, (cur_uv[:, 1] - cy) / fy, np.ones(T)], 1) * Z
        return pr.pose_law(P, Q, np.ones(T, np.int32), 0.03)
    turned = align(nn_1)
    assert turned["status"] == pr.OK
    w = turned["v"][3:] / -0.03                                   # v = -lambda (R^T t, theta u)
    assert abs(np.linalg.norm(w) - np.pi / 2) <= 1e-9 and abs(abs(w[2]) - np.pi / 2) <= 1e-9, w
    assert np.linalg.norm(turned["t"]) <= 1e-9
    # the camera is turned by +90 degrees about its optical axis: X_goal = Rz(+90) X_cam
    assert np.allclose(turned["R"], rodrigues(np.array([0.0, 0.0, np.pi / 2])), atol=1e-9)
    same = align(ident)
    assert same["status"] == pr.OK and np.linalg.norm(same["v"]) <= 1e-12


# ----------------------------------------------------------------------------- refusals
class _FakeEngine:
    """What servo.Controller's constructor reads of an engine."""

    def __init__(self, max_pairs, params):
        self.max_pairs, self.params = max_pairs, params
        self.cfg = config.baseline_config(KEY)
        self.engines = [self]

    def apply_law_params(self, params):
        self.params = params

    def set_goal_depth(self, z):
        pass


def test_the_controllers_refusals():
    S = 224
    goal = np.zeros((S, S, 3), np.uint8)
    with pytest.raises(ValueError, match="subpatch"):
        config.ServoParams(dino_input_size=S, roll_search=True, subpatch=True)
    on = config.ServoParams(dino_input_size=S, roll_search=True)
    with pytest.raises(ValueError, match="reference"):
        servo.Controller(_FakeEngine(4, on), goal, on, selection="reference")
    with pytest.raises(ValueError, match="max_pairs"):
        servo.Controller(_FakeEngine(3, on), goal, on, selection="best")
    ctl = servo.Controller(_FakeEngine(4, on), goal, on, selection="best")
    assert ctl.last_roll is None
    with pytest.raises(ValueError, match="roll_search"):
        servo.MultiController(_FakeEngine(8, on), [goal, goal], on)
    from vitvs_amd.pipeline import UpdatePipeline
    with pytest.raises(ValueError, match="roll_search"):
        UpdatePipeline(config.baseline_config(KEY), on, {}, precision="fp32")
    # best_roll needs room for the four copies too, and a frame
    off = config.ServoParams(dino_input_size=S)
    plain = servo.Controller(_FakeEngine(1, off), goal, off, selection="best")
    with pytest.raises(ValueError, match="image_callback_rgb"):
        plain.best_roll()
    plain.image_callback_rgb(goal)
    with pytest.raises(ValueError, match="max_pairs"):
        plain.best_roll()
    # the key of a reference-style configuration file
    assert config.ServoParams().roll_search is False
