"""Host-side mirror of the reference's interface around the HIP hot path.

Same names, argument meaning and error behaviour as the reference's callables, without ROS:

  compute_velocity(I_cur, I_des, Z, K)        the north-star seam = detect_features() + ibvs() up to the raw
                                              twist (reference: vitvs_v2.py:464-523, 588-622)
  find_correspondences_batch(desc1, desc2)    reference: vitvs_v2.py:72-155 (same return shapes, same RNG stream)
  Controller.detect_features() / .ibvs()      reference: vitvs_v2.py:464-523, 588-632 (EMA :325-343, failure
                                              counter :500-505, twist remap :661-676)
  Controller.best_rotation(frames)            reference: find_and_set_best_pose, vitvs_v2.py:1151-1189
  Controller.best_roll()                      the same question answered from ONE frame (the roll search)
  ServoLoop (vit-vs_amd/loop.py)              reference: Controller.run / is_visual_servoing_done, :702-819, :345-421

All arithmetic of the path runs on the GPU through ``Engine`` (C ABI); what stays on the host is what the
reference also does on the host: PIL resize, the RNG draw, the EMA state and the twist remap.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from .config import ServoParams
from .engine import Engine, VitvsError

STATUS_NAMES = {0: "ok", 1: "no_correspondence", 2: "too_few_features", 3: "no_depth"}


# ------------------------------------------------------------------------------------------ functional API
def compute_velocity(engine: Engine, I_cur, I_des, Z, K=None, *, selection="order",
                     generator: Optional[torch.Generator] = None, num_pairs: Optional[int] = None):
    """One servo update for one frame pair: raw (pre-EMA) ``v_c`` float64[6] and a status int.

    ``I_cur`` / ``I_des``: uint8 RGB frames already at the extractor's input size (the reference resizes with
    PIL before the path); ``Z``: the sensor's uint16 millimetre depth image; ``K`` = (fx, fy, cx, cy), default
    from the engine's parameters.  ``selection``:
      "order"      a fresh random visiting order (CPU generator); the first num_pairs mutual-NN tokens met are used,
                   everything stays on the device (one graph replay)
      "reference"  the reference's exact procedure and RNG stream (torch sort + randperm on the host between the
                   correspondence and the control law; two device round trips, as in the reference)
      "dense"      every mutual-NN token
      "best"       the device's own deterministic choice (``SELECT_BEST``): the mutual-NN tokens ranked by similarity and taken
                   round-robin over ``params.select_cells`` x ``select_cells`` image cells; no draw, nothing from the host
      array-like   explicit token ids of the desired frame
    ``num_pairs``: feature pairs of the law for this call (the reference's ``Controller.num_pairs``; default: the
    engine's parameters).
    """
    one = lambda a: a[None] if torch.is_tensor(a) else np.asarray(a)[None]   # noqa: E731  (device tensors stay there)
    des = None if I_des is None else one(I_des)            # None: the goal cached by Engine.set_goal
    v, st = compute_velocity_batch(engine, one(I_cur), des, None if Z is None else one(Z), K, selection=selection,
                                   generator=generator, num_pairs=num_pairs)
    return v[0], int(st[0])


def compute_velocity_batch(engine: Engine, I_cur, I_des, Z, K=None, *, selection="order", des_shared: bool = False,
                           generator: Optional[torch.Generator] = None, num_pairs: Optional[int] = None):
    """``B`` pairs in one call → (v_c float64 [B,6], status int32 [B]) as numpy arrays."""
    p = engine.params
    K = p.intrinsics() if K is None else K
    n = int(I_cur.shape[0]) if torch.is_tensor(I_cur) else np.asarray(I_cur).shape[0]
    if isinstance(selection, str) and selection == "reference":
        if n != 1:
            raise ValueError('selection="reference" follows the reference: one pair per call')
        return _reference_update(engine, I_cur, I_des, Z, K, generator, num_pairs)
    mode, sel = _engine_selection(selection, n, engine.tokens, generator)
    v, st = engine.compute_velocity(I_cur, I_des, Z, K, mode=mode, selection=sel, des_shared=des_shared,
                                    num_pairs=None if mode == _lib.SELECT_DENSE else num_pairs)   # (dense: the engine's own num_pairs)
    return v.cpu().numpy(), st.cpu().numpy()


def _engine_selection(selection, n: int, tokens: int, generator=None):
    """The ``selection`` keyword as the ``(mode, selection)`` an ``Engine`` call of ``n`` pairs takes: "order": one fresh visiting
    order per pair, int32 [n, tokens] on the host, one ``torch.randperm`` each, drawn in pair (camera) order; "dense" and "best":
    nothing to draw, no selection; anything else: explicit token ids, one list per pair (or the one pair's ids)."""
    if isinstance(selection, str) and selection == "order":
        draws = [torch.randperm(tokens, generator=generator) for _ in range(n)]
        # (one pair, every Controller update: a view of the draw, no stacked copy)
        return _lib.SELECT_ORDER, (draws[0][None] if n == 1 else torch.stack(draws)).to(torch.int32)
    if isinstance(selection, str) and selection in ("dense", "best"):
        return (_lib.SELECT_DENSE if selection == "dense" else _lib.SELECT_BEST), None
    return _lib.SELECT_EXPLICIT, list(selection) if isinstance(selection, (list, tuple)) and n > 1 else [selection]


def _candidate_order(nn_1: torch.Tensor, nn_2: torch.Tensor, grid: int, distance_threshold: float = 1.0):
    """Tokens that pass the reference's cyclic-consistency filter, in the order its descending sort leaves them
    (so that a following ``randperm`` picks the same tokens as the reference does with the same seed)."""
    t = nn_1.numel()
    back = nn_2[nn_1]                                    # where each token's best match points back to
    here = torch.arange(t)
    delta = torch.stack((back // grid - here // grid, back % grid - here % grid), dim=-1)
    dist = -torch.linalg.vector_norm((delta + 1e-6).to(torch.float32), 2, dim=-1)
    spread = dist - dist.min()
    spread = spread / (spread.max() + 1e-8)
    vals, order = spread.sort(dim=-1, descending=True)
    return order[vals >= distance_threshold]


def find_correspondences_batch(engine: Engine, descriptors1: torch.Tensor, descriptors2: torch.Tensor,
                               num_pairs: int = 18, distance_threshold: float = 1):
    """Drop-in for the reference function: descriptors ``[1,1,T,D']`` → ``(points1, points2, sim)`` with
    ``points*`` int64 ``[K,2]`` (row, col) and ``sim`` ``[1,K]``, or ``(None, None, None)``.
    Similarities and arg-maxes run on the GPU; the draw uses torch's global CPU RNG like the reference."""
    d1 = descriptors1.reshape(-1, descriptors1.shape[-1])
    d2 = descriptors2.reshape(-1, descriptors2.shape[-1])
    t = d1.shape[0]
    grid = int(np.sqrt(t))
    nn_1, nn_2, sim_1 = (x.cpu() for x in engine.correspond(d1, d2))
    nn_1, nn_2 = nn_1.long(), nn_2.long()
    rc = lambda idx: torch.stack((idx // grid, idx % grid), dim=-1)  # noqa: E731
    if sim_1.mean().item() > 0.99:                       # same-image shortcut
        k = min(num_pairs, t)
        pts = rc(torch.randperm(t)[:k])
        return pts, pts.clone(), torch.ones(k)
    cand = _candidate_order(nn_1, nn_2, grid, distance_threshold)
    k = min(num_pairs, cand.numel())
    if k == 0:
        return None, None, None
    chosen = cand[torch.randperm(cand.numel())[:k]]
    return rc(chosen), rc(nn_1[chosen]), sim_1[chosen].unsqueeze(0)


def _reference_update(engine: Engine, I_cur, I_des, Z, K, generator, num_pairs=None):
    """The reference's own sequence with ONE forward: similarity + arg-max on the device, the reference's sort + ``randperm``
    draw on the host (same torch RNG stream), then the control law on the device for the drawn tokens.

    Host arrays in the engine's frame geometry (what the ``Controller``'s callbacks hold) take the two-call form: the host-pointer
    update (``vitvs_compute_velocity``; its own law, on a fixed visiting order, is thrown away) leaves the arg-max tables in host
    memory, the draw runs, and ``vitvs_reselect`` evaluates the law for the drawn tokens on the keys, depth image and intrinsics
    the first call left in the handle.  Device tensors (``Controller._resized``) and other geometries go through the descriptor
    seams (``extract_descriptors`` -> ``correspond`` -> ``servo_from_nn``), as before."""
    k = engine.params.num_pairs if num_pairs is None else int(num_pairs)

    def draw(nn_1, nn_2, sim_1):
        return _draw_like_the_reference(nn_1, nn_2, sim_1, engine.cfg.grid, k, generator)

    host = (not torch.is_tensor(I_cur) and not torch.is_tensor(I_des) and I_des is not None
            and tuple(np.asarray(I_cur).shape[-3:-1]) == tuple(engine.frame_size)
            and (Z is None or (not torch.is_tensor(Z) and np.asarray(Z).dtype == np.uint16)))
    if host:
        order = np.arange(engine.tokens, dtype=np.int32)
        _, st0 = engine.compute_velocity_host(I_cur, I_des, Z, K, _lib.SELECT_ORDER, order, num_pairs=k)
        tab = engine.last_tables(1)
        ids = draw(tab["nn_1"][0], tab["nn_2"][0], tab["sim_1"][0])
        if ids is None:                                   # (None, None, None) in the reference
            return np.zeros((1, 6)), np.array([_lib.STATUS_NO_CORRESPONDENCE], np.int32)
        v, st = engine.reselect_host(_lib.SELECT_EXPLICIT, [ids.to(torch.int32).numpy()], num_pairs=k)
        return v, st
    both = torch.cat([torch.as_tensor(I_des).to(engine.device), torch.as_tensor(I_cur).to(engine.device)])
    desc = engine.extract_descriptors(both)
    d1, d2 = desc[0, 0], desc[1, 0]
    nn_1, nn_2, sim_1 = engine.correspond(d1, d2)
    ids = draw(nn_1.cpu().long(), nn_2.cpu().long(), sim_1.cpu())
    z = None if Z is None else torch.as_tensor(Z).reshape(engine.params.v_max, engine.params.u_max)
    if ids is None:                                       # (None, None, None) in the reference
        return np.zeros((1, 6)), np.array([_lib.STATUS_NO_CORRESPONDENCE], np.int32)
    v, st = engine.servo_from_nn(nn_1, nn_2, sim_1, z, K, mode=_lib.SELECT_EXPLICIT, selection=[ids.to(torch.int32)],
                                 num_pairs=k)
    return v.cpu().numpy()[None], np.array([int(st)], np.int32)


_GRID_CACHE: dict = {}


def _candidate_order_host(nn_1: np.ndarray, nn_2: np.ndarray, grid: int) -> torch.Tensor:
    """``_candidate_order`` on host arrays: the integer part (index arithmetic) in numpy, every floating-point step — the shifted
    norm, the normalised spread, the descending sort whose tie order the draw inherits — through the same torch calls on the same
    values, so the result is the same tensor (tests/test_servo_host.py compares the two over random and degenerate tables).  The
    ``Controller``'s default selection runs this between two device calls on every update: ~15 small torch ops were 0.1 ms of it."""
    t = int(nn_1.shape[0])
    here = _GRID_CACHE.get((t, grid))
    if here is None:
        idx = np.arange(t, dtype=np.int64)
        here = _GRID_CACHE[(t, grid)] = (idx // grid, idx % grid)
    back = nn_2[nn_1].astype(np.int64, copy=False)
    delta = np.empty((t, 2), np.int64)
    np.subtract(back // grid, here[0], out=delta[:, 0])
    np.subtract(back % grid, here[1], out=delta[:, 1])
    dist = -torch.linalg.vector_norm((torch.from_numpy(delta) + 1e-6).to(torch.float32), 2, dim=-1)
    spread = dist - dist.min()
    spread = spread / (spread.max() + 1e-8)
    vals, order = spread.sort(dim=-1, descending=True)
    return order[vals >= 1.0]


def _draw_like_the_reference(nn_1, nn_2, sim_1, grid: int, num_pairs: int, generator=None):
    """Token ids of the desired frame as ``find_correspondences_batch`` draws them (vitvs_v2.py:84-141), or None.  ``generator``:
    the torch CPU generator standing in for the reference's global RNG (``torch.randperm(n, generator=g)`` draws what
    ``torch.randperm(n)`` draws from a global RNG in the same state; None: the global RNG itself).  Tensors or host arrays."""
    if not torch.is_tensor(nn_1):
        nn_1, nn_2, sim_1 = np.asarray(nn_1), np.asarray(nn_2), np.asarray(sim_1)
        t = int(nn_1.shape[0])
        if float(torch.from_numpy(sim_1).mean()) > 0.99:     # same-image shortcut (torch's fp32 mean, like the reference's)
            return torch.randperm(t, generator=generator)[:min(num_pairs, t)]
        cand = _candidate_order_host(nn_1, nn_2, grid)
    else:
        t = nn_1.numel()
        if sim_1.mean().item() > 0.99:                       # same-image shortcut
            return torch.randperm(t, generator=generator)[:min(num_pairs, t)]
        cand = _candidate_order(nn_1, nn_2, grid)
    k = min(num_pairs, cand.numel())
    if k == 0:
        return None
    return cand[torch.randperm(cand.numel(), generator=generator)[:k]]


def ema_update(state: list, v: Sequence[float], alpha: float) -> np.ndarray:
    """Per-component exponential moving average with the reference's first-sample initialisation."""
    out = np.empty(6)
    for i, x in enumerate(np.asarray(v, dtype=np.float64).reshape(6)):
        state[i] = x if state[i] is None else alpha * x + (1 - alpha) * state[i]
        out[i] = state[i]
    return out


def twist_from_velocity(v_c, max_velocity: float):
    """Camera optical frame → (linear xyz, angular xyz) as the reference publishes them (clipped)."""
    c = lambda x: float(min(max(x, -max_velocity), max_velocity))  # noqa: E731
    return (c(v_c[2]), c(-v_c[0]), c(-v_c[1])), (c(v_c[5]), c(-v_c[3]), c(-v_c[4]))


def twist_matrix(R, t) -> np.ndarray:
    """The 6 x 6 twist transform W from a rig frame to a camera's optical frame (ViSP's ``cVe``), fp64.  The camera has pose
    (R, t) in the rig frame, X_rig = R X_cam + t; a rig twist v_r = (v, w) expressed in the rig frame moves the camera with
    v_c = W v_r in its own frame:  W = [[R^T, -R^T [t]x], [0, R^T]]."""
    R = np.asarray(R, np.float64).reshape(3, 3)
    t = np.asarray(t, np.float64).reshape(3)
    tx = np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])
    W = np.zeros((6, 6))
    W[:3, :3] = R.T
    W[:3, 3:] = -R.T @ tx
    W[3:, 3:] = R.T
    return W


# ------------------------------------------------------------------------------------------ frames in
def _is_pil(img) -> bool:
    return hasattr(img, "convert") and not isinstance(img, np.ndarray)


def _as_array(img):
    """A PIL image or anything array-like as a uint8 array; a tensor passes through (device tensors stay there)."""
    if _is_pil(img):
        img = np.asarray(img.convert("RGB"), dtype=np.uint8)
    return img if torch.is_tensor(img) else np.asarray(img, dtype=np.uint8)


def _resized(engine: Engine, img):
    """The reference's ``image.resize((S, S))`` (PIL default filter: bicubic, vitvs_v2.py:474-475), done on the
    device by ``Engine.resize_frames`` — bit-identical to PIL, no host round trip.  Accepts a uint8 HxWx3 array or
    a PIL image; returns uint8 [S,S,3] (a device tensor when a resize was needed)."""
    arr, s = _as_array(img), engine.cfg.img_size
    return arr if tuple(arr.shape[:2]) == (s, s) else engine.resize_frames(arr)[0]


def _engine_frames(engines, imgs, rejected=None):
    """The frames as the engines take them.  When all share one geometry (the usual case: one camera, one kind of camera in a
    rig), the frames themselves: ``Engine.set_frame_size`` makes the launch that builds the patch rows apply the reference's
    ``image.resize((S, S))`` (vitvs_v2.py:474-475) on the way, bit-identical to PIL and without a resized image in
    memory.  Mixed geometries, a geometry in ``rejected`` (the set of those the fused resize has refused), or ``rejected`` None
    (the caller needs the square frames in memory): the engines' frame size is reset and every frame of another geometry goes
    through the stand-alone resize launch on its own (``_resized``, on the first engine)."""
    arrs = [_as_array(img) for img in imgs]
    shapes = {tuple(a.shape[:2]) for a in arrs}
    if rejected is not None and len(shapes) == 1 and not shapes & rejected:
        try:
            for e in engines:
                e.set_frame_size(*next(iter(shapes)))
            return arrs
        except VitvsError:
            # a geometry the fused resize cannot take (too many camera rows per patch for its LDS rows, or no memory for
            # the staging buffers): the engine kept its previous geometry (vitvs_set_frame_size changes nothing on
            # failure); fall back to the stand-alone resize launch below — and do not ask again for this geometry: every
            # attempt builds Pillow's tables, allocates and synchronises the device
            rejected |= shapes
    for e in engines:
        e.set_frame_size()
    return [_resized(engines[0], a) for a in arrs]


# ------------------------------------------------------------------------------------------ Controller adapter
class Controller:
    """ROS-free stand-in for the reference ``Controller``'s hot-path half: feed it frames, call ``ibvs()``
    in the control loop, read ``v_c``.  Attribute names follow the reference so its ``run()`` logic ports 1:1."""

    def __init__(self, engine: Engine, goal_image, params: Optional[ServoParams] = None,
                 selection: str = "reference", goal_depth=None):
        self.engine = engine
        self.params = params or engine.params
        if params is not None:
            engine.apply_law_params(params)               # the law of the params this controller was given
        self.goal_depth = None                            # uint16 millimetres at the goal pose (interaction "desired" / "mean", law "pose")
        if self.params.law == "pose":
            # the pose law aligns the current 3-D points with the goal's: it needs Z* from a goal depth image and Z in
            # the feature rows, which interaction "desired" replaces by Z*
            if goal_depth is None:
                raise ValueError('law="pose" needs goal_depth: the depth image taken at the goal pose')
            if self.params.interaction == "desired":
                raise ValueError('law="pose" does not combine with interaction="desired" (its feature rows hold Z*, not Z)')
        if self.params.roll_search:
            # every update goes through the roll search (Engine.roll_velocity): the four quarter-turned copies of the
            # current frame in one batch, so the handle needs room for four pairs; the draw must be the device's or an order / ids
            if self.params.subpatch:
                raise ValueError("roll_search does not combine with subpatch: the sub-patch offsets of a turned copy would have to be turned too")
            if isinstance(selection, str) and selection == "reference":
                raise ValueError('roll_search does not combine with selection="reference": the reference draws on the host between the '
                                 'correspondence and the law, the roll search picks and carries back on the device in between')
            if engine.max_pairs < 4:
                raise ValueError(f"roll_search matches four turned copies in one batch: engine.max_pairs is {engine.max_pairs}, needs >= 4")
        if self.params.photometric_handover > 0 and self.params.roll_search:
            raise ValueError("photometric_handover does not combine with roll_search: the hand-over watches the plain update's twist")
        if self.params.photometric_handover > 0 and goal_image is not None:
            # the photometric law runs on the camera-resolution frames with the camera's intrinsics: a goal of another size could
            # never be handed over to
            size = tuple(_as_array(goal_image).shape[:2])
            if size != (self.params.v_max, self.params.u_max):
                raise ValueError(f"photometric_handover needs the goal image at the camera's v_max x u_max "
                                 f"({self.params.v_max} x {self.params.u_max}), got {size[0]} x {size[1]}")
        self.photometric_active = False                   # photometric_handover: the photometric law has the robot
        self.last_photometric = None                      # dict(status, cost = sum e^2 / n, n) of its last call; its robust form
                                                          # (photometric_illumination / _robust_iterations): and gain, bias, sigma, rejected;
                                                          # its tile form (photometric_tiles): and sigma, rejected, dead_tiles, gain_min, gain_max;
                                                          # its surface form (photometric_surface): and sigma, rejected, dead, gain_min, gain_max
        self._photo_goal_src = None                       # the PIL goal image _photo_goal was converted from
        self._photo_goal = None                           # (host copy, device tensor) of the goal frame at camera resolution, and
        self._photo_goal_depth = None                     # of the goal depth: uploaded once, compared by content like _goal_np
        self.last_roll = None                             # roll_search: the winner k of the last update (-1: no valid candidate), and
        self.last_roll_info = None                        # Engine.roll_velocity's info dict of it
        if goal_depth is not None:
            self.set_goal_depth(goal_depth)
        self.last_pose_status = None                      # law "pose": the pose law's status of the last update, and its
        self.last_pose = None                             # (R [3, 3], t [3]): the current camera in the goal camera's frame
        self.last_homography_status = None                # law "homography": the homography law's status of the last update, and
        self.last_homography = None                       # its H [3, 3] (m* ~ H m, det 1); needs no goal_depth and no depth callback
        self.num_pairs = self.params.num_pairs
        self.dino_input_size = engine.cfg.img_size
        self.goal_image = goal_image                      # PIL image or uint8 array, any size
        self.latest_image = None                          # uint8 HxWx3 RGB (the reference keeps BGR + a PIL copy)
        self.latest_pil_image = None
        self.latest_image_depth = None                    # uint16 millimetres, v_max x u_max
        self.selection = selection
        self.feature_failure_count = 0
        self.ema_velocities = [None] * 6
        self.v_c = None                                   # like the reference (vitvs_v2.py:224): unset until the first update
        self.velocity_vector_history = []
        self.max_velocity_vector_history = 200            # config.yaml:37
        self.last_status = None
        self.generator = None                             # torch.Generator of the "order" / "reference" draws (None: torch's global RNG)
        self._goal_np = None                              # a private, never-written copy of the goal frame: its address tells the
                                                          # library that the staged goal is still the goal (option "reuse_goal_frames")
        self._rejected_geometries = set()                 # camera geometries the fused resize refused (set_frame_size), per engine

    def set_goal_depth(self, depth_u16):
        """The depth image taken at the goal pose (uint16 millimetres, v_max x u_max): Z* of the "desired" and "mean" interaction
        matrices.  With "desired" the run then needs no depth image at all.  ``None`` clears it."""
        self.goal_depth = None if depth_u16 is None else np.asarray(depth_u16)
        self.engine.set_goal_depth(self.goal_depth)

    # -- inputs (the reference's ROS callbacks)
    def image_callback_rgb(self, rgb_u8):
        self.latest_image = np.asarray(rgb_u8)
        self.latest_pil_image = self.latest_image

    def image_callback_depth(self, depth_u16):
        self.latest_image_depth = np.asarray(depth_u16)

    def _resized(self, img):
        return _resized(self.engine, img)

    def _path_frames(self, *imgs):
        """The frames as the engine takes them: themselves where the fused resize takes their one geometry (``_engine_frames``)."""
        return _engine_frames([self.engine], imgs, self._rejected_geometries)

    # -- the hot path
    def detect_features(self):
        """→ ((s_uv_star, s_uv), sim_selected) with int arrays [num_pairs,2] in camera pixels, or (None, None).
        The 10th consecutive failure raises RuntimeError("Persistent feature detection failure")."""
        if self.latest_image is None:
            return None, None
        if self.params.roll_search:
            return self._detect_features_rolled()
        cur, des = self._path_frames(self.latest_pil_image, self.goal_image)
        if not torch.is_tensor(des):
            # the goal image does not change from update to update (vitvs_v2.py:264): hand the library the SAME private buffer every
            # time, so that it forwards the goal frame already in device memory instead of staging it again (its tokens are still
            # recomputed on every update, like the reference does).  The copy is keyed on the goal's CONTENT (one comparison of S x S x 3
            # bytes: microseconds), as the reference reads self.goal_image on every update: a goal rewritten in place or replaced,
            # at whatever address, is copied and staged again (setting the option forgets the address staged before)
            if self._goal_np is None or self._goal_np.shape != des.shape or not np.array_equal(self._goal_np, des):
                self._goal_np = np.array(des, dtype=np.uint8, copy=True, order="C")
                self.engine.set_option("reuse_goal_frames", 1)
            des = self._goal_np
        depth = self.latest_image_depth
        # the law needs a depth image; detect_features itself does not, so feed a dummy one if it is missing
        z = depth if depth is not None else np.zeros((self.params.v_max, self.params.u_max), np.uint16)
        eng = self.engine
        if isinstance(self.selection, str) and self.selection in ("order", "dense", "best") and not torch.is_tensor(cur) \
                and not torch.is_tensor(des) and tuple(cur.shape[:2]) == tuple(eng.frame_size) and np.asarray(z).dtype == np.uint16:
            # the callbacks' own arrays straight into the host-pointer entry point: one C call, no torch tensor, the feature
            # rows come back with it (Engine.last_features reads them from the handle's pinned block)
            mode, order = _engine_selection(self.selection, 1, eng.tokens, self.generator)
            v, st = eng.compute_velocity_host(cur, des, z, self.params.intrinsics(), mode, None if order is None else order.numpy(),
                                              num_pairs=self.num_pairs)
            if not self._absorb(v[0], int(st[0])):
                return None, None
            return self._features(eng.last_features(1), 0)
        v, st = compute_velocity(eng, cur, des, z, self.params.intrinsics(), selection=self.selection,
                                 generator=self.generator, num_pairs=self.num_pairs)
        if not self._absorb(v, st):
            return None, None
        return self._features(eng.last_features(1), 0)

    def _square_frames(self, *imgs):
        """The frames at S x S for the roll search: the engine's frame size is reset and every frame of another geometry goes
        through the stand-alone resize launch on its own (``_resized``; a quarter turn needs the square frame in memory)."""
        return _engine_frames([self.engine], imgs)

    def _roll_call(self, num_pairs, depth):
        """One ``Engine.roll_velocity`` on the latest frame with this controller's selection."""
        eng = self.engine
        cur, des = self._square_frames(self.latest_pil_image, self.goal_image)
        z = depth if depth is not None else np.zeros((self.params.v_max, self.params.u_max), np.uint16)
        mode, sel = _engine_selection(self.selection, 1, eng.tokens, self.generator)
        return eng.roll_velocity(cur, des, z, self.params.intrinsics(), mode, sel, num_pairs=num_pairs)

    def _detect_features_rolled(self):
        """``detect_features`` with ``params.roll_search``: the update through the roll search, then the configured law as ever."""
        v, st, info = self._roll_call(self.num_pairs, self.latest_image_depth)
        self.last_roll, self.last_roll_info = info["roll"], info
        if not self._absorb(v.cpu().numpy(), int(st)):
            return None, None
        return self._features(self.engine.last_features(1), 0)

    def best_roll(self):
        """``(k, scores)`` for the latest frame: the quarter turn k (``numpy.rot90(frame, k)``) under which it matches the goal best,
        and the four candidates' scores (None where a candidate is not valid); ``(None, scores)`` when none is.  It answers
        ``best_rotation``'s question from ONE frame, without the robot moving (``Engine.roll_velocity``; needs ``max_pairs >= 4``).
        The controller's own state (EMA, counters, ``last_roll``) is not touched."""
        if self.latest_image is None:
            raise ValueError("best_roll needs a frame: image_callback_rgb first")
        if self.engine.max_pairs < 4:
            raise ValueError(f"the roll search matches four turned copies in one batch: engine.max_pairs is {self.engine.max_pairs}, needs >= 4")
        if isinstance(self.selection, str) and self.selection == "reference":
            raise ValueError('best_roll draws on the device: selection "order", "dense", "best" or explicit ids')
        _, _, info = self._roll_call(self.num_pairs, None)
        scores = [None if np.isnan(s) else float(s) for s in info["scores"]]
        return (info["roll"] if info["roll"] >= 0 else None), scores

    def _absorb(self, v, st) -> bool:
        """Bookkeeping of one finished update (whoever computed it: this controller's engine, or a ``MultiController``'s batched
        call / pipeline slot): raw twist, status, the consecutive-failure counter of vitvs_v2.py:500-505."""
        self._raw_v, self.last_status = v, st
        if self.params.law == "pose":
            self._pose_step(st)
        elif self.params.law == "homography":
            self._homography_step(st)
        if st == _lib.STATUS_NO_CORRESPONDENCE:
            self.feature_failure_count += 1
            if self.feature_failure_count >= 10:
                raise RuntimeError("Persistent feature detection failure")
            return False
        self.feature_failure_count = 0
        return True

    def _pose_step(self, st):
        """law "pose": the pose law behind this update's law evaluation (one more launch on what it left in the handle).  When its
        status is OK its twist replaces the raw ``v_c`` that the EMA, the remap and the history see; otherwise the update stays the
        image-based law's."""
        p = self.params
        if st == _lib.STATUS_NO_CORRESPONDENCE:           # (the reference draw may have ended before any law evaluation)
            self.last_pose_status, self.last_pose = int(st), None
            return
        v, info = self.engine.pose_velocity_host(p.intrinsics(), [st], p.pose_robust_iterations, p.pose_consensus,
                                                 p.pose_consensus_seed)
        self.last_pose_status = int(info["status"][0])
        self.last_pose = (info["R"][0].copy(), info["t"][0].copy())
        if self.last_pose_status == _lib.STATUS_OK:
            self._raw_v = v[0]

    def _homography_step(self, st):
        """law "homography": the homography law behind this update's law evaluation (one more launch on the matched image points it
        left in the handle; a camera status of NO_DEPTH does not stop it).  When its status is OK its twist replaces the raw ``v_c``
        that the EMA, the remap and the history see; otherwise the update stays the image-based law's where that had a depth image
        to read, and is the homography law's zero twist where it had none."""
        p = self.params
        if st == _lib.STATUS_NO_CORRESPONDENCE:           # (the reference draw may have ended before any law evaluation)
            self.last_homography_status, self.last_homography = int(st), None
            return
        v, info = self.engine.homography_velocity_host(p.intrinsics(), [st], p.homography_depth, p.homography_robust_iterations,
                                                        p.homography_consensus, p.homography_consensus_seed)
        self.last_homography_status = int(info["status"][0])
        self.last_homography = info["H"][0].copy()
        if self.last_homography_status == _lib.STATUS_OK or (self.latest_image_depth is None and p.interaction != "desired"):
            self._raw_v = v[0]                            # (not OK and no depth image for the image-based law either: its zero twist)

    def _features(self, det, b: int = 0):
        """``detect_features``' return value from pair ``b`` of an engine's ``last_details``."""
        k = self.num_pairs
        s_uv_star = det["s_uv"][b, :k, 0:2].astype(int)
        s_uv = det["s_uv"][b, :k, 2:4].astype(int)
        n_matched = int(det["info"][b, 3])
        sim = torch.from_numpy(det["feat"][b, :max(n_matched, 0), 3].astype(np.float32)).unsqueeze(0)
        return (s_uv_star, s_uv), sim

    def ibvs(self):
        """One control-law step: updates ``self.v_c`` (EMA-smoothed) or leaves it untouched on failure.  With
        ``params.photometric_handover`` > 0 and the hand-over made (``photometric_active``), the step is the photometric law's alone:
        no forward runs."""
        if self.latest_image is None:
            return
        if self.photometric_active and self._photometric_step():
            return
        result = self.detect_features()
        if self._law_step(result is not None and result[0] is not None):
            self._watch_handover()

    def _law_step(self, have_features: bool) -> bool:
        if not have_features:
            return False
        if self.latest_image_depth is None and self.params.interaction != "desired" and self.params.law != "homography":
            return False                                  # reference: "Failed to get depth - skipping"; L(s*, Z*) reads none, and
                                                          # neither does the homography law
        # fewer than 4 matches: the reference's calculate_uv hands back all-zero feature arrays of num_pairs rows
        # (vitvs_v2.py:539-541), len() >= 4 passes the check at :604, e = 0 and the raw twist is exactly 0 — which is
        # what the kernel reports with status TOO_FEW; the EMA is updated with it, as in the reference
        self._smooth()
        return True

    def _smooth(self):
        """The raw twist through the EMA into ``v_c`` and the history."""
        self.v_c = ema_update(self.ema_velocities, self._raw_v, self.params.ema_alpha)
        self.velocity_vector_history.append(self.v_c)
        if len(self.velocity_vector_history) > self.max_velocity_vector_history:
            self.velocity_vector_history.pop(0)

    # -- the hand-over to the photometric law (params.photometric_handover > 0)
    def _watch_handover(self):
        """Behind a ViT update that reached the EMA: with status OK and max |raw v_c| / lambda_ — the law's own estimate of what is
        left, in metres / radians; exactly 0 under the same-image shortcut — below the threshold, the next ``ibvs()`` is the
        photometric law's."""
        p = self.params
        if not p.photometric_handover > 0 or self.last_status != _lib.STATUS_OK or p.lambda_ == 0:
            return
        left = float(np.max(np.abs(np.asarray(self._raw_v, np.float64)))) / abs(p.lambda_)
        if left < p.photometric_handover and self._photometric_inputs() is not None:
            self.photometric_active = True

    def _device_copy(self, cached, arr):
        """(host copy, device tensor) of ``arr``, uploaded again only when its content changed."""
        if cached is None or cached[0].shape != arr.shape or not np.array_equal(cached[0], arr):
            host = np.array(arr, copy=True, order="C")
            cached = (host, torch.from_numpy(host).to(self.engine.device))
        return cached

    def _photometric_inputs(self):
        """(current frame, goal frame on the device, depth image or None, scalar depth) at camera resolution, or None when the goal
        image is not at the camera's v_max x u_max (the intrinsics are that geometry's)."""
        p = self.params
        goal = self.goal_image
        cur = np.asarray(self.latest_image, dtype=np.uint8)
        if not _is_pil(goal):                                                 # an array may be rewritten in place: compared by content
            self._photo_goal = self._device_copy(self._photo_goal, np.asarray(goal, dtype=np.uint8))
        elif self._photo_goal is None or self._photo_goal_src is not goal:    # a PIL image: converted and uploaded once per object
            self._photo_goal, self._photo_goal_src = self._device_copy(None, _as_array(goal)), goal
        if cur.shape != (p.v_max, p.u_max, 3) or self._photo_goal[0].shape != cur.shape:
            return None
        depth = self.goal_depth if p.photometric_interaction == "desired" else self.latest_image_depth
        z = None
        if depth is not None and np.asarray(depth).dtype == np.uint16 and np.asarray(depth).shape[-2:] == (p.v_max, p.u_max) \
                and np.asarray(depth).size == p.v_max * p.u_max:
            if p.photometric_interaction == "desired":
                self._photo_goal_depth = self._device_copy(self._photo_goal_depth, np.asarray(depth).reshape(p.v_max, p.u_max))
                z = self._photo_goal_depth[1]
            else:
                z = np.asarray(depth).reshape(p.v_max, p.u_max)
        return cur, self._photo_goal[1], z, (0.0 if z is not None else p.homography_depth)

    def _photometric_step(self) -> bool:
        """One update by the photometric law alone.  False, with the hand-over cleared, when its status is not OK or its rejected
        share is above ``photometric_handback_rejected``: the caller runs the ViT update for this call."""
        p = self.params
        inputs = self._photometric_inputs()
        if inputs is None:
            self.photometric_active = False
            return False
        cur, goal, z, scalar = inputs
        lam = p.lambda_ if p.photometric_lambda is None else p.photometric_lambda
        robust = p.photometric_illumination or p.photometric_robust_iterations > 0
        tiles = tuple(p.photometric_tiles) != (1, 1)
        surface = p.photometric_surface is not None
        if surface:
            v, info = self.engine.photometric_surface_velocity(cur, goal, None if z is None else z[None], p.intrinsics(),
                                                               p.photometric_level, p.photometric_interaction, p.photometric_mu, lam,
                                                               scalar, tuple(p.photometric_surface), p.photometric_robust_iterations,
                                                               p.photometric_sigma_min)
        elif tiles:
            v, info = self.engine.photometric_tile_velocity(cur, goal, None if z is None else z[None], p.intrinsics(),
                                                            p.photometric_level, p.photometric_interaction, p.photometric_mu, lam, scalar,
                                                            tuple(p.photometric_tiles), p.photometric_robust_iterations,
                                                            p.photometric_sigma_min)
        elif robust:
            v, info = self.engine.photometric_robust_velocity(cur, goal, None if z is None else z[None], p.intrinsics(),
                                                              p.photometric_level, p.photometric_interaction, p.photometric_mu, lam, scalar,
                                                              p.photometric_illumination, p.photometric_robust_iterations,
                                                              p.photometric_sigma_min)
        else:
            v, info = self.engine.photometric_velocity(cur, goal, None if z is None else z[None], p.intrinsics(), p.photometric_level,
                                                       p.photometric_interaction, p.photometric_mu, lam, scalar)
        st = int(info["status"][0])
        self.last_photometric = dict(status=st, cost=float(info["cost"][0]), n=int(info["n"][0]))
        if surface:
            gains = info["node_gain"][0][info["node_live"][0]]
            self.last_photometric.update(sigma=float(info["sigma"][0]), rejected=float(info["rejected"][0]), dead=int(info["dead"][0]),
                                         gain_min=float(gains.min()) if gains.size else 0.0,
                                         gain_max=float(gains.max()) if gains.size else 0.0)
        elif tiles:
            gains = info["tile_gain"][0][info["tile_live"][0]]
            self.last_photometric.update(sigma=float(info["sigma"][0]), rejected=float(info["rejected"][0]),
                                         dead_tiles=int(info["dead_tiles"][0]),
                                         gain_min=float(gains.min()) if gains.size else 0.0,
                                         gain_max=float(gains.max()) if gains.size else 0.0)
        elif robust:
            self.last_photometric.update({k: float(info[k][0]) for k in ("gain", "bias", "sigma", "rejected")})
        # photometric_handback_rejected: a rejected share above it is a status that is not OK
        share = p.photometric_handback_rejected
        if st != _lib.STATUS_OK or (share > 0 and (surface or tiles or robust) and self.last_photometric["rejected"] > share):
            self.photometric_active = False
            return False
        self._raw_v, self.last_status = v[0].cpu().numpy(), st
        self.feature_failure_count = 0
        self._smooth()
        return True

    def publish_twist(self, v_c=None):
        return twist_from_velocity(self.v_c if v_c is None else v_c, self.params.max_velocity)

    # -- rotation compensation: 4 (or any number of) candidate views against the one goal image
    ROTATION_SEARCH_PAIRS = 48                            # vitvs_v2.py:1158

    def best_rotation(self, candidate_frames: Sequence, generator: Optional[torch.Generator] = None):
        """Index of the candidate current frame whose selected correspondences are most similar on average, and the
        scores (reference: find_and_set_best_pose — ``num_pairs`` raised to 48 for these calls, score =
        ``sim_selected_12.mean()``, the first best wins, failed views are skipped), evaluated as ONE batch of
        ``len(candidate_frames)`` pairs sharing the goal forward.  Returns ``(None, scores)`` if every view failed."""
        eng = self.engine
        n = len(candidate_frames)
        if eng.max_pairs < n:
            raise ValueError("engine.max_pairs is smaller than the number of candidates")
        k = self.ROTATION_SEARCH_PAIRS
        if eng.max_rows < k:
            raise ValueError(f"engine.max_rows must be >= {k} for the rotation search")
        dev = eng.device
        frames = self._path_frames(self.goal_image, *candidate_frames)
        des = torch.as_tensor(frames[0]).to(dev)[None]
        cur = torch.stack([torch.as_tensor(f).to(dev) for f in frames[1:]])
        z = np.zeros((n, self.params.v_max, self.params.u_max), np.uint16)
        mode, order = _engine_selection("order", n, eng.tokens, generator)
        _, st = eng.compute_velocity(cur, des, z, self.params.intrinsics(), mode=mode, selection=order, des_shared=True, num_pairs=k)
        det = eng.last_details(n)
        status = st.cpu().numpy()
        scores, best, best_mean = [], None, float("-inf")
        for b in range(n):
            m = int(det["info"][b, 3])
            if status[b] == _lib.STATUS_NO_CORRESPONDENCE or m == 0:
                scores.append(None)                       # "Feature detection failed for this rotation"
                continue
            mean = float(det["feat"][b, :m, 3].astype(np.float32).mean())
            scores.append(mean)
            if mean > best_mean:
                best_mean, best = mean, b
        return best, scores


# ------------------------------------------------------------------------------------------ several cameras, one GPU
class MultiController:
    """N cameras on ONE GPU (BASELINE.json configs[3], the 8-camera rig, when the rig has fewer GPUs than cameras).

    The reference runs one ``Controller`` per camera and process (vitvs_v2.py:702-819), each with its own goal image, EMA state,
    failure counter and history (:224, :325-343, :500-505).  Here every camera keeps exactly that state — ``self.cameras[i]`` IS a
    ``Controller`` and is fed through its own ``image_callback_*`` — while one round of updates for all of them goes to the GPU
    together:

      backend = ``Engine`` with ``max_pairs >= N``   ONE batched call per round: the N frame pairs run through the many-row
                                                     kernels as one launch chain (bench.py ``--pairs N``)
      backend = ``UpdatePipeline``                   one update per camera, ``depth`` of them in flight on separate handles and
                                                     streams (what bench.py measures ``value`` with); the cameras' inputs live in
                                                     device buffers of their own, so every (slot, camera) replays its captured graph

    Each camera's raw and smoothed ``v_c`` equal those of an independent ``Controller(Engine)`` fed the same frames and the same
    draw (tests/test_gpu_multi.py: bit for bit).  ``selection``: "order" (a fresh random visiting order per camera and round, drawn
    in camera order from ``generator`` / torch's global RNG, exactly the draws N ``Controller(selection="order")`` make when their
    ``ibvs()`` are called in camera order), "dense", "best" (the device's own deterministic choice per camera, ``SELECT_BEST``: no
    draw at all), or — per round, through ``ibvs(selection=[ids_0, ...])`` — explicit token ids.
    The reference's host-side sort + randperm draw ("reference") needs a host round trip per camera and stays with ``Controller``.
    """

    def __init__(self, backend, goal_images: Sequence, params: Optional[ServoParams] = None, selection: str = "order",
                 generator: Optional[torch.Generator] = None, goal_depth=None, rig: Optional[Sequence] = None):
        from .pipeline import UpdatePipeline
        self.pipe = backend if isinstance(backend, UpdatePipeline) else None
        # rig = [(R_i, t_i), ...]: the cameras are one rigid body, camera i at pose (R_i, t_i) in the rig frame.  After each
        # round's batched call the rig law (Engine.rig_velocity) gives the ONE twist of the rig over that round's live cameras:
        # ``rig_velocity_raw``, and ``v_rig`` smoothed by the cameras' EMA; the cameras' own state is exactly as without it.
        # With ``params.rig_robust_iterations`` = N > 0 that law is the robust rig law (N Tukey re-weightings of the stack) and
        # ``rig_weights`` [cameras, max_rows] holds the round's final weights (0 for a camera without an image, None before).
        # With ``params.law`` = "pose" (Engine backend, ``rig=`` and ``goal_depth=`` required) that law is the pose rig law
        # (Engine.pose_rig_velocity) with ``params.rig_pose_robust_iterations`` re-weightings, and ``rig_pose`` = (R, t)
        # is the current rig in the goal rig's frame; ``goal_depth`` is then one image for all cameras or [N, v, u], one per camera.
        self.rig_W = None
        self.rig = None
        self.rig_weights = None
        self.rig_pose = None
        self.rig_velocity_raw, self.v_rig, self.rig_status, self.rig_info = None, None, None, None
        self._rig_ema = [None] * 6
        if rig is not None:
            if self.pipe is not None:
                raise ValueError("rig= needs the Engine backend: a pipeline slot sees one camera, the rig law all of them in one handle")
            if len(rig) != len(goal_images):
                raise ValueError("rig= takes one (R, t) per camera")
            self.rig_W = np.stack([twist_matrix(R, t) for R, t in rig])
            self.rig = [(np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)) for R, t in rig]
        self.engines = list(backend.engines) if self.pipe is not None else [backend]
        self.engine = self.engines[0]
        self.law = (params or self.engine.params).law
        self._goal_depths, self._goal_depth_live = None, None
        if (params or self.engine.params).roll_search:
            raise ValueError("roll_search is servo.Controller's: a MultiController round is one batched call over the cameras, the roll "
                             "search one call of four turned copies per camera")
        # photometric_handover > 0: once a round's rig twist says less than that is left, the rounds are the photometric rig law's
        # alone (Engine.photometric_rig_velocity) on the live cameras' camera-resolution frames, until its status is
        # not OK.  ``goal_depth`` (one image, or one per camera) is then also the depth of interaction "desired".
        self.photometric_active = False
        self.last_photometric = None                      # dict(status, cost, n, cameras, gain, bias, sigma, rejected) of its last call;
                                                          # with photometric_handback_rejected: and rejected_share, the stack's
        self._photo_goal, self._photo_depth, self._photo_rows = None, None, None
        self._photo_goal_depth = None if goal_depth is None else np.asarray(goal_depth)
        if tuple((params or self.engine.params).photometric_tiles) != (1, 1):
            raise ValueError("photometric_tiles is servo.Controller's: the photometric rig law keeps one gain per camera, and tiles "
                             "inside a rig are not built")
        if (params or self.engine.params).photometric_surface is not None:
            raise ValueError("photometric_surface is servo.Controller's: the photometric rig law keeps one gain per camera, and a "
                             "lighting surface inside a rig is not built")
        if (params or self.engine.params).photometric_handover > 0:
            if self.pipe is not None:
                raise ValueError("photometric_handover needs the Engine backend: the photometric rig law reads all cameras in one handle, "
                                 "a pipeline slot sees one camera")
            if rig is None:
                raise ValueError("photometric_handover in a MultiController hands over to the photometric RIG law and needs "
                                 "rig=[(R_i, t_i), ...]: the hand-over watches the rig's one twist (one camera: servo.Controller)")
        if self.law == "homography":
            raise ValueError('law="homography" is servo.Controller\'s: the homography law has no rig form (one camera, one plane)')
        if self.law == "pose":
            # the cameras run the image-based law exactly as with law "ibvs"; the pose law of a MultiController is the RIG's
            if self.pipe is not None:
                raise ValueError('law="pose" needs the Engine backend: the pose rig law reads all cameras in one handle')
            if rig is None:
                raise ValueError('MultiController runs the image-based law per camera: law="pose" here is the pose rig law and needs '
                                 'rig=[(R_i, t_i), ...] (one camera: servo.Controller)')
            if goal_depth is None:
                raise ValueError('law="pose" needs goal_depth: the depth image(s) taken at the goal pose')
            if (params or self.engine.params).interaction == "desired":
                raise ValueError('law="pose" does not combine with interaction="desired" (its feature rows hold Z*, not Z)')
            gd = np.asarray(goal_depth)
            if gd.ndim == 3 and gd.shape[0] != len(goal_images):
                raise ValueError("goal_depth is one image for all cameras, or one per camera")
            self._goal_depths = gd if gd.ndim == 3 else None
            params = (params or self.engine.params).replace(law="ibvs")
        if selection not in ("order", "dense", "best"):
            raise ValueError('MultiController draws on the device: selection is "order", "dense" or "best" (explicit ids per round: ibvs(selection=...))')
        self.selection, self.generator = selection, generator
        n = len(goal_images)
        if self.pipe is None and self.engine.max_pairs < n:
            raise ValueError(f"engine.max_pairs ({self.engine.max_pairs}) is smaller than the number of cameras ({n})")
        if params is not None:
            for e in self.engines:                        # every pipeline slot evaluates the law of the params given
                e.apply_law_params(params)
        self.cameras = [Controller(self.engine, g, params, selection="order") for g in goal_images]
        self.params = self.cameras[0].params
        if self.law == "pose":
            self.params = self.params.replace(law="pose")
        # the goal depth of interaction "desired" / "mean": one image (uint16 [v_max, u_max]) that serves every camera, in every
        # engine or slot (one image pairs with a call of any number of pairs)
        if goal_depth is not None:
            if self.pipe is not None:
                self.pipe.set_goal_depth(np.asarray(goal_depth))
            else:
                self.engine.set_goal_depth(np.asarray(goal_depth))
        self._buffers = {}                                # pipeline mode: per-camera device inputs at stable addresses

    def __len__(self):
        return len(self.cameras)

    @property
    def v_c(self):
        """The cameras' smoothed twists (None until a camera's first successful update), like ``Controller.v_c``."""
        return [c.v_c for c in self.cameras]

    # -- inputs: camera i's ROS callbacks
    def image_callback_rgb(self, i: int, rgb_u8):
        self.cameras[i].image_callback_rgb(rgb_u8)

    def image_callback_depth(self, i: int, depth_u16):
        self.cameras[i].image_callback_depth(depth_u16)

    # -- one round
    def _frames_for(self, live):
        """(current frames, goal frames) of the live cameras as the engines take them: one geometry for all (the usual rig) goes in
        as it is and is resized inside the patch-row build (``Engine.set_frame_size``); anything else is resized per frame first.
        The geometries the fused resize refused are remembered in camera 0's set."""
        imgs = [self.cameras[i].latest_pil_image for i in live] + [self.cameras[i].goal_image for i in live]
        frames = _engine_frames(self.engines, imgs, self.cameras[0]._rejected_geometries)
        return frames[:len(live)], frames[len(live):]

    def _absorb_rig(self, v_r, live, weights: bool) -> bool:
        """A rig law's result of this round: with ``weights`` its final weights into ``rig_weights`` [cameras, max_rows] (0 for a
        camera that is not live), and with status OK the raw rig twist and its EMA.  True with status OK."""
        if weights:
            self.rig_weights = np.zeros((len(self.cameras), self.engine.max_rows))
            self.rig_weights[live] = self.rig_info["weights"].cpu().numpy()
        if self.rig_status != _lib.STATUS_OK:
            return False
        self.rig_velocity_raw = v_r.cpu().numpy()
        self.v_rig = ema_update(self._rig_ema, self.rig_velocity_raw, self.params.ema_alpha)
        return True

    # -- the hand-over to the photometric rig law (params.photometric_handover > 0)
    def _watch_handover(self, live):
        """Behind a round whose rig law ran: with rig status OK and max |raw rig twist| / lambda_ below the threshold, the next
        rounds are the photometric rig law's."""
        p = self.params
        if not p.photometric_handover > 0 or self.rig_status != _lib.STATUS_OK or p.lambda_ == 0 or self.rig_velocity_raw is None:
            return
        left = float(np.max(np.abs(np.asarray(self.rig_velocity_raw, np.float64)))) / abs(p.lambda_)
        if left < p.photometric_handover and self._photometric_inputs(live) is not None:
            self.photometric_active = True

    @staticmethod
    def _photometric_rows(z, n, shape, level):
        """The rows of each of ``n`` cameras at pooled ``level``: the pooled pixels inside the one-pixel border whose block holds a
        depth sample (``z`` uint16 [n, v, u]; None: every one)."""
        h, w = shape[0] >> level, shape[1] >> level
        if z is None:
            return np.full(n, (h - 2) * (w - 2), np.int64)
        s = 1 << level
        filled = (np.asarray(z)[:, :h * s, :w * s].reshape(n, h, s, w, s) != 0).any(axis=(2, 4))
        return filled[:, 1:-1, 1:-1].sum(axis=(1, 2)).astype(np.int64)

    def _photometric_inputs(self, live):
        """(current frames, goal frames on the device, depth images or None, scalar depth, rows per camera) of the live cameras at
        camera resolution, or None when a frame or a goal image is not at the cameras' v_max x u_max."""
        p, cam0 = self.params, self.cameras[0]
        shape = (p.v_max, p.u_max)
        cur = [np.asarray(self.cameras[i].latest_image, dtype=np.uint8) for i in live]
        goals = [_as_array(self.cameras[i].goal_image) for i in live]
        if any(a.shape != shape + (3,) for a in cur + goals):
            return None
        self._photo_goal = cam0._device_copy(self._photo_goal, np.stack(goals).astype(np.uint8, copy=False))
        z, rows = None, None
        if p.photometric_interaction == "desired":
            gd = self._photo_goal_depth
            if gd is not None and gd.dtype == np.uint16 and gd.shape[-2:] == shape and gd.ndim in (2, 3) \
                    and (gd.ndim == 2 or gd.shape[0] == len(self.cameras)):
                stack = np.broadcast_to(gd, (len(live),) + shape) if gd.ndim == 2 else gd[live]
                before = self._photo_depth
                self._photo_depth = cam0._device_copy(before, stack)
                if self._photo_depth is not before or self._photo_rows is None:
                    self._photo_rows = self._photometric_rows(self._photo_depth[0], len(live), shape, p.photometric_level)
                z, rows = self._photo_depth[1], self._photo_rows
        else:
            depths = [self.cameras[i].latest_image_depth for i in live]
            if all(d is not None and np.asarray(d).dtype == np.uint16 and np.asarray(d).size == shape[0] * shape[1] for d in depths):
                z = np.stack([np.asarray(d).reshape(shape) for d in depths])
                rows = self._photometric_rows(z, len(live), shape, p.photometric_level)
        if z is None:
            rows = self._photometric_rows(None, len(live), shape, p.photometric_level)
        return np.stack(cur), self._photo_goal[1], z, (0.0 if z is not None else p.homography_depth), rows

    def _photometric_round(self, live) -> bool:
        """One round by the photometric rig law alone.  False, with the hand-over cleared, when its status is not OK or the share
        of rows at weight 0 is above ``photometric_handback_rejected``: the caller runs the batched ViT round for this call."""
        p = self.params
        inputs = self._photometric_inputs(live)
        if inputs is None:
            self.photometric_active = False
            return False
        cur, goal, z, scalar, rows = inputs
        lam = p.lambda_ if p.photometric_lambda is None else p.photometric_lambda
        v, info = self.engine.photometric_rig_velocity(cur, goal, z, p.intrinsics(), self.rig_W[live], None, p.photometric_level,
                                                       p.photometric_interaction, p.photometric_mu, lam, scalar,
                                                       p.photometric_illumination, p.photometric_robust_iterations,
                                                       p.photometric_sigma_min)
        st = int(info["status"])
        with np.errstate(divide="ignore", invalid="ignore"):
            rejected = np.where(rows > 0, 1.0 - info["weight"] / np.maximum(rows, 1), 0.0)
        self.last_photometric = dict(status=st, cost=float(info["cost"]), n=int(info["n"]), cameras=list(live),
                                     gain=info["gain"].tolist(), bias=info["bias"].tolist(), sigma=float(info["sigma"].max()),
                                     rejected=rejected.tolist())
        # photometric_handback_rejected: a share of the stack's rows at weight 0 above it is a status that is not OK
        share = p.photometric_handback_rejected
        if share > 0:
            self.last_photometric["rejected_share"] = float(info["zero_weight"]) / max(int(info["n"]), 1)
        if st != _lib.STATUS_OK or (share > 0 and self.last_photometric["rejected_share"] > share):
            self.photometric_active = False
            return False
        self.rig_status, self.rig_info = st, info
        self.rig_velocity_raw = v.cpu().numpy()
        self.v_rig = ema_update(self._rig_ema, self.rig_velocity_raw, p.ema_alpha)
        return True

    def ibvs(self, selection=None, want_features: bool = False):
        """One control-law step for every camera that has an image: each camera's ``v_c`` is updated (EMA) or left untouched on
        failure, exactly as its own ``Controller.ibvs()`` would.  Returns the per-camera ``detect_features`` results
        (``((s_uv_star, s_uv), sim)`` or ``(None, None)``; ``None`` for cameras without an image) when ``want_features``.
        With ``params.photometric_handover`` > 0 and the hand-over made (``photometric_active``), the round is the photometric rig
        law's alone: no forward runs, the cameras' own state stays, and only ``v_rig`` moves."""
        live = [i for i, c in enumerate(self.cameras) if c.latest_image is not None]
        results = [None] * len(self.cameras)
        if not live:
            return results if want_features else None
        if self.photometric_active and self._photometric_round(live):
            return results if want_features else None
        p, eng = self.params, self.engine
        cur, des = self._frames_for(live)
        zeros = np.zeros((p.v_max, p.u_max), np.uint16)
        depth = [self.cameras[i].latest_image_depth if self.cameras[i].latest_image_depth is not None else zeros for i in live]
        k = self.cameras[0].num_pairs
        if selection is not None:
            mode, sel = _lib.SELECT_EXPLICIT, [np.asarray(selection[i]) for i in live]
        else:                                             # "order": one fresh order per camera, drawn in camera order
            mode, sel = _engine_selection(self.selection, len(live), eng.tokens, self.generator)
        if self.pipe is None:
            if self._goal_depths is not None and self._goal_depth_live != live:
                # one goal depth per camera: the engine pairs image j with pair j of the call, so a round of other live
                # cameras needs theirs (set-up, only when the live set changed)
                eng.set_goal_depth(np.ascontiguousarray(self._goal_depths[live]))
                self._goal_depth_live = list(live)
            stack = lambda xs: torch.stack([torch.as_tensor(x).to(eng.device) for x in xs])   # noqa: E731
            v, st = eng.compute_velocity(stack(cur), stack(des), np.stack(depth), p.intrinsics(), mode=mode, selection=sel, num_pairs=k)
            if self.law == "pose":                        # the pose rig law in place of the image-based rig law
                v_r, self.rig_status, self.rig_info = eng.pose_rig_velocity([self.rig[i] for i in live], p.intrinsics(), st,
                                                                            p.rig_pose_robust_iterations)
                if self._absorb_rig(v_r, live, weights=self.rig_status == _lib.STATUS_OK):
                    self.rig_pose = (self.rig_info["R"].cpu().numpy(), self.rig_info["t"].cpu().numpy())
            elif self.rig_W is not None:                  # (before the host reads: the law is one more launch behind the call)
                N = p.rig_robust_iterations               # > 0: Tukey IRLS over the stack, one median over all live cameras' residuals
                v_r, self.rig_status, self.rig_info = eng.rig_velocity(self.rig_W[live], st, N, K=p.intrinsics() if N else None)
                self._absorb_rig(v_r, live, weights=N > 0)
            if self.rig_W is not None:
                self._watch_handover(live)
            v, st = v.cpu().numpy(), st.cpu().numpy()
            det = eng.last_features(len(live)) if want_features else None
            failure = None
            for j, i in enumerate(live):
                # a camera's 10th consecutive failure raises (vitvs_v2.py:500-505) — after EVERY camera of the round has been
                # absorbed: N independent Controllers would each have taken their own step
                try:
                    ok = self.cameras[i]._absorb(v[j], int(st[j]))
                except RuntimeError as exc:
                    failure, ok = failure or exc, False
                if want_features:
                    results[i] = self.cameras[i]._features(det, j) if ok else (None, None)
                self.cameras[i]._law_step(ok)
            if failure is not None:
                raise failure
            return results if want_features else None
        # pipeline: `depth` cameras in flight at a time; a slot's outputs are read before the slot is used again
        pipe, dev = self.pipe, eng.device
        pending = []
        failures = []

        def collect(upto):
            while len(pending) > upto:
                i, t = pending.pop(0)
                v, st = pipe.result(t)
                try:
                    ok = self.cameras[i]._absorb(v.cpu().numpy()[0], int(st[0]))
                except RuntimeError as exc:               # raised once the round is complete and nothing is in flight (below)
                    failures.append(exc)
                    ok = False
                if want_features:
                    results[i] = self.cameras[i]._features(pipe.engines[t % pipe.depth].last_features(1), 0) if ok else (None, None)
                self.cameras[i]._law_step(ok)

        for j, i in enumerate(live):
            buf = self._buffers.setdefault(i, {})

            def stable(name, value, dtype=None):
                t_ = torch.as_tensor(value)
                t_ = t_ if dtype is None else t_.to(dtype)
                b_ = buf.get(name)
                if b_ is None or b_.shape != t_.shape or b_.dtype != t_.dtype:
                    b_ = torch.empty(t_.shape, dtype=t_.dtype, device=dev)
                    buf[name] = b_
                b_.copy_(t_, non_blocking=True)
                return b_
            c_ = stable("cur", cur[j])[None]
            d_ = stable("des", des[j])[None]
            z_ = stable("Z", depth[j])[None]
            k_ = stable("K", torch.tensor([p.intrinsics()], dtype=torch.float64))
            s_, n_ = None, None
            if mode == _lib.SELECT_ORDER:
                s_ = stable("order", sel[j])[None]
            elif mode == _lib.SELECT_EXPLICIT:
                ids = torch.zeros(k, dtype=torch.int32)
                got = torch.as_tensor(sel[j], dtype=torch.int32).flatten()[:k]
                ids[:got.numel()] = got
                s_ = stable("ids", ids)[None]
                n_ = stable("n_ids", torch.tensor([got.numel()], dtype=torch.int32))
            collect(pipe.depth - 1)
            pending.append((i, pipe.submit(c_, d_, z_, k_, mode, s_, n_, False, k)))
        collect(0)
        if failures:
            pipe.synchronize()                            # no slot still reads the cameras' input buffers when the caller sees it
            raise failures[0]
        return results if want_features else None

    def detect_features(self):
        """Every camera's ``Controller.detect_features()`` result for this round (and the law step, as ``ibvs`` does it)."""
        return self.ibvs(want_features=True)

    def publish_twist(self, i: int, v_c=None):
        return self.cameras[i].publish_twist(v_c)
