"""Model and servo configuration for the ViT-VS hot path.

The model names are the ones the reference's ``ViTExtractor`` accepts
(reference: catkin_ws/ibvs/src/dinov2_extractor.py:28-29, 57-83); the servo
defaults are the reference's config.yaml values
(reference: catkin_ws/ibvs/config/config.yaml:1-17, 38).
"""
from __future__ import annotations

import dataclasses
import math
from dataclasses import dataclass
from typing import Optional

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
HALF_MEAN = (0.5, 0.5, 0.5)
HALF_STD = (0.5, 0.5, 0.5)


@dataclass(frozen=True)
class ViTConfig:
    """Geometry of one extractor model at one input size.

    ``layer`` is the block whose output is the descriptor (reference:
    vitvs_v2.py:484, dinov2_extractor.py:226-229); blocks after it are never run.
    """
    model_type: str
    img_size: int          # S: side of the (square) ViT input
    patch: int             # p
    stride: int            # patch-embed stride (== patch unless the extractor's stride hack is used)
    dim: int               # D
    depth: int             # blocks in the checkpoint
    heads: int             # H (head dim is always 64 for this family)
    layerscale: bool       # DINOv2 layout (ls1/ls2 gammas)
    native_grid: int       # side of the grid pos_embed is stored at
    layer: int = 11
    mlp_ratio: int = 4
    ln_eps: float = 1e-6
    registers: int = 0     # R: register tokens (DINOv2 "_reg" checkpoints), rows 1 .. R of the sequence, no position embedding

    @property
    def grid(self) -> int:
        # reference: dinov2_extractor.py:262 (1 + (H - p) // stride)
        return 1 + (self.img_size - self.patch) // self.stride

    @property
    def tokens(self) -> int:  # T, patch tokens
        return self.grid * self.grid

    @property
    def prefix(self) -> int:  # P: rows in front of the patch tokens (cls + registers)
        return 1 + self.registers

    @property
    def seq(self) -> int:  # N = T + cls + registers
        return self.tokens + self.prefix

    @property
    def head_dim(self) -> int:
        return self.dim // self.heads

    @property
    def hidden(self) -> int:
        return self.dim * self.mlp_ratio

    @property
    def blocks_run(self) -> int:
        return self.layer + 1

    @property
    def mean(self):
        # reference: dinov2_extractor.py:49-50 (substring test on the model name)
        return IMAGENET_MEAN if "dino" in self.model_type else HALF_MEAN

    @property
    def std(self):
        return IMAGENET_STD if "dino" in self.model_type else HALF_STD

    @property
    def patch_k(self) -> int:
        return 3 * self.patch * self.patch

    def flops_per_image(self) -> float:
        """Algorithmic FLOPs of one forward through block ``layer``."""
        n, d, h = self.seq, self.dim, self.hidden
        per_block = 2 * n * d * 3 * d + 2 * 2 * n * n * d + 2 * n * d * d + 2 * 2 * n * d * h
        return 2.0 * self.tokens * self.patch_k * d + self.blocks_run * per_block

    def flops_per_pair(self, binned: bool = False) -> float:
        gram = 2.0 * self.tokens * self.tokens * self.dim * (9 if binned else 1)
        return 2 * self.flops_per_image() + gram

    def weight_elems(self) -> int:
        d, h = self.dim, self.hidden
        per_block = 3 * d * d + d * d + 2 * d * h
        return self.patch_k * d + self.blocks_run * per_block


_FAMILY = {
    # name: (patch, dim, depth, heads, layerscale, native image side[, register tokens])
    "dino_vits16": (16, 384, 12, 6, False, 224),
    "dino_vits8": (8, 384, 12, 6, False, 224),
    "dino_vitb16": (16, 768, 12, 12, False, 224),
    "dino_vitb8": (8, 768, 12, 12, False, 224),
    "vit_small_patch16_224": (16, 384, 12, 6, False, 224),
    "vit_small_patch8_224": (8, 384, 12, 6, False, 224),
    "vit_base_patch16_224": (16, 768, 12, 12, False, 224),
    "vit_base_patch8_224": (8, 768, 12, 12, False, 224),
    "dinov2_vits14": (14, 384, 12, 6, True, 518),
    "dinov2_vitb14": (14, 768, 12, 12, True, 518),
    "dinov2_vitl14": (14, 1024, 24, 16, True, 518),
    # DINOv2 with registers (Darcet et al., "Vision Transformers Need Registers"): the same networks plus 4 learned tokens
    # between the class token and the patches, published beside the plain checkpoints under these names
    "dinov2_vits14_reg": (14, 384, 12, 6, True, 518, 4),
    "dinov2_vitb14_reg": (14, 768, 12, 12, True, 518, 4),
    "dinov2_vitl14_reg": (14, 1024, 24, 16, True, 518, 4),
}


def vit_config(model_type: str, img_size: int, stride: int | None = None, layer: int = 11) -> ViTConfig:
    if model_type not in _FAMILY:
        raise ValueError(f"unknown model_type {model_type!r}; known: {sorted(_FAMILY)}")
    patch, dim, depth, heads, ls, native, *reg = _FAMILY[model_type]
    stride = patch if stride is None else int(stride)
    if (patch // stride) * stride != patch:
        # reference: dinov2_extractor.py:137-138
        raise ValueError(f"stride {stride} should divide patch_size {patch}")
    if not 0 <= layer < depth:
        raise ValueError(f"layer {layer} outside 0..{depth - 1}")
    if img_size < patch:
        raise ValueError("image smaller than one patch")
    if (img_size - patch) % stride != 0:
        # the reference floors (dinov2_extractor.py:262, 1 + (H - p) // stride) and silently ignores the right / bottom
        # remainder; the device path needs the covered extent to be exact, so ask for the size that is actually used
        used = patch + ((img_size - patch) // stride) * stride
        raise ValueError(f"img_size {img_size} leaves a remainder for patch {patch} / stride {stride}: "
                         f"resize or crop to {used} (the extent the reference's floor would use)")
    return ViTConfig(model_type=model_type, img_size=int(img_size), patch=patch, stride=stride, dim=dim,
                     depth=depth, heads=heads, layerscale=ls, native_grid=native // patch, layer=layer,
                     registers=reg[0] if reg else 0)


# The five BASELINE.json configs + the reference's shipped default, by short key.
BASELINE_CONFIGS = {
    "vits16_224": ("dino_vits16", 224),       # configs[0]
    "vitb16_224": ("vit_base_patch16_224", 224),  # configs[1] and [3]
    "vitb8_448": ("dino_vitb8", 448),         # configs[2]
    "vitl14_518": ("dinov2_vitl14", 518),     # configs[4]
    "vits14_308": ("dinov2_vits14", 308),     # reference default (vitvs_v2.py:250, config.yaml:14)
}


def baseline_config(key: str) -> ViTConfig:
    name, size = BASELINE_CONFIGS[key]
    return vit_config(name, size)


LAWS = ("ibvs", "pose", "homography")            # ServoParams.law: the image-based law of the reference, the pose law,
                                                 # or the homography law of a planar target, which needs no depth
PHOTOMETRIC_INTERACTIONS = ("current", "desired")  # ServoParams.photometric_interaction: the photometric law has no mean form
INTERACTIONS = ("current", "desired", "mean")    # values 0 / 1 / 2 of option "interaction" (include/vitvs.h)


@dataclass
class ServoParams:
    """Camera + control-law parameters (reference: config.yaml:1-17,38; vitvs_v2.py:278-283)."""
    u_max: int = 640
    v_max: int = 480
    f_x: float = 502.3016357421875
    f_y: float = 502.3016357421875
    lambda_: float = 0.03
    num_pairs: int = 24
    dino_input_size: int = 308
    use_feature_binning: bool = True
    ema_alpha: float = 0.8
    max_velocity: float = 1.0
    robust_iterations: int = 0     # Tukey re-weightings of the control law (option "robust_law", 1 .. 16); 0 = the reference's
                                   # plain least squares.  Not in the reference's config.yaml: an extension, off by default
    subpatch: bool = False         # sub-patch refinement of the matches (option "subpatch"); False = the reference's patch centres.
                                   # Not in the reference's config.yaml either: an extension, off by default
    interaction: str = "current"   # the interaction matrix the law inverts (option "interaction"): "current" L(s, Z), the reference's;
                                   # "desired" L(s*, Z*); "mean" of the two.  The last two need a goal depth (Engine.set_goal_depth)

    select_cells: int = 4          # image cells per side of selection "best" (option "select_cells", 1 .. 16): the best matches are
                                   # taken round-robin over a select_cells x select_cells grid; 1 = the most similar ones wherever
                                   # they lie.  Not in the reference's config.yaml: it belongs to an extension

    rig_robust_iterations: int = 0  # Tukey re-weightings of the RIG law (MultiController(rig=...): one median over all cameras'
                                    # residuals, vitvs_rig_robust_velocity_dev; 1 .. 16); 0 = the plain rig law

    law: str = "ibvs"              # the twist a servo.Controller executes: "ibvs", the image-based law above (the reference's),
                                   # "pose": the pose law on the matched 3-D points (Engine.pose_velocity), which needs a goal depth, or
                                   # "homography": the homography law of a planar target (Engine.homography_velocity): RGB only
    pose_robust_iterations: int = 0  # Tukey re-weightings of the pose law (0 .. 16); 0 = the plain alignment
    pose_consensus: int = 0        # three-point hypotheses of the pose law's consensus start (0 .. 4096): the law starts
                                   # from the rows that agree with the best of them instead of from all rows; 0 = no such start.
                                   # 256 fills one round of the kernel's workgroup.  Past one half of wrong matches run it with
                                   # pose_robust_iterations = 0: the re-weightings' scale is a median over all rows
    pose_consensus_seed: int = 0   # of the hypotheses' draw (0 .. 2^32 - 1); fixed across updates: same frames, same twist
    rig_pose_robust_iterations: int = 0  # Tukey re-weightings of the pose RIG law (MultiController(rig=..., law "pose"): one median
                                         # over all cameras' 3-D residuals, vitvs_pose_rig_velocity_dev; 0 .. 16); 0 = the plain one

    homography_robust_iterations: int = 0  # Tukey re-weightings of the homography law (0 .. 16); 0 = the plain DLT
    homography_depth: float = 1.0  # the homography law's depth scale in metres (> 0): a rough guess of the distance to the target,
                                   # which scales its translational gain and nothing else
    homography_consensus: int = 0  # four-point hypotheses of the homography law's consensus start (0 .. 4096): the law
                                   # starts from the rows that agree with the best of them instead of from all rows; 0 = no such
                                   # start.  256 fills one round of the kernel's workgroup
    homography_consensus_seed: int = 0  # of the hypotheses' draw (0 .. 2^32 - 1); fixed across updates: same frames, same twist

    roll_search: bool = False      # a servo.Controller runs every update through the roll search (Engine.roll_velocity): the
                                   # current frame is matched as its four quarter-turned copies and the law runs on the best one's
                                   # matches, so the servo starts from any in-plane rotation.  Four or five forwards per update
                                   # instead of two; needs an engine with max_pairs >= 4; not with subpatch or selection "reference"

    photometric_handover: float = 0.0  # > 0: a servo.Controller hands the robot to the photometric law (Engine.photometric_velocity,
                                       # DESIGN.md 5k) once an update's raw twist says less than this is left, max |v_c| / lambda_ in
                                       # metres / radians; from then on no forward runs.  0 = off, nothing changes.  The photometric
                                       # law's domain is small: hand over inside the ViT law's dead zone, not before.  A
                                       # servo.MultiController(rig=...) hands over to the photometric RIG law on
                                       # max |rig twist| / lambda_
    photometric_level: int = 2         # its pyramid level, 0 .. 3: luminance pooled over 2^level x 2^level pixels
    photometric_mu: float = 0.01       # its Levenberg-Marquardt damping (>= 0; 0 = Gauss-Newton)
    photometric_lambda: Optional[float] = None  # its gain; None: lambda_
    photometric_interaction: str = "desired"    # "desired": gradients of the goal image, depth = the goal depth; "current": of the
                                                # current frame, depth = the latest depth image
    photometric_illumination: bool = False      # the hand-over runs the robust photometric law (Engine.photometric_robust_velocity,
                                                # DESIGN.md 5l) and estimates a lighting gain and bias with the twist
    photometric_robust_iterations: int = 0      # 0 .. 4 Tukey re-weightings of its rows (> 0: the robust law); both off: the plain law
    photometric_sigma_min: float = 1.0          # > 0, grey levels: the floor of the robust law's residual scale
    photometric_tiles: tuple = (1, 1)           # (tiles_y, tiles_x), each 1 .. 8: a lighting gain / bias per tile of that grid
                                                # (Engine.photometric_tile_velocity); needs photometric_illumination.
                                                # (1, 1) = off: the hand-over calls exactly what it calls without this field
    photometric_handback_rejected: float = 0.0  # a share in (0, 1]: a robust, tile or rig photometric call that leaves more than
                                                # this share of its rows at weight 0 hands back to the ViT update, as a status
                                                # that is not OK does; needs photometric_robust_iterations > 0.  0 = off
    photometric_surface: Optional[tuple] = None # (cells_y, cells_x), each 1 .. 8: a SMOOTH lighting model, a bilinear spline of gains
                                                # and biases on the nodes of that grid (Engine.photometric_surface_velocity, DESIGN.md
                                                # 5o); needs photometric_illumination, and excludes photometric_tiles.  None = off:
                                                # the hand-over calls exactly what it calls without this field

    def __post_init__(self):
        if not isinstance(self.photometric_illumination, bool):
            raise ValueError(f"photometric_illumination is a flag, got {self.photometric_illumination!r}")
        if isinstance(self.photometric_robust_iterations, bool) or not isinstance(self.photometric_robust_iterations, int) \
                or not 0 <= int(self.photometric_robust_iterations) <= 4:
            raise ValueError(f"photometric_robust_iterations is 0 .. 4, got {self.photometric_robust_iterations!r}")
        if isinstance(self.photometric_sigma_min, bool) or not isinstance(self.photometric_sigma_min, (int, float)) \
                or not (math.isfinite(float(self.photometric_sigma_min)) and float(self.photometric_sigma_min) > 0.0):
            raise ValueError(f"photometric_sigma_min is finite and > 0 grey levels, got {self.photometric_sigma_min!r}")
        t = self.photometric_tiles
        if isinstance(t, list):
            t = tuple(t)                                                          # a YAML sequence
            object.__setattr__(self, "photometric_tiles", t)
        if not (isinstance(t, tuple) and len(t) == 2 and all(isinstance(g, int) and not isinstance(g, bool) and 1 <= g <= 8 for g in t)):
            raise ValueError(f"photometric_tiles is (tiles_y, tiles_x), each 1 .. 8, got {self.photometric_tiles!r}")
        if t != (1, 1) and not self.photometric_illumination:
            raise ValueError("photometric_tiles other than (1, 1) needs photometric_illumination=True: the tiles are the grid of the "
                             "lighting model, and a grid without a lighting model means nothing")
        sf = self.photometric_surface
        if isinstance(sf, list):
            sf = tuple(sf)                                                        # a YAML sequence
            object.__setattr__(self, "photometric_surface", sf)
        if sf is not None:
            if not (isinstance(sf, tuple) and len(sf) == 2
                    and all(isinstance(g, int) and not isinstance(g, bool) and 1 <= g <= 8 for g in sf)):
                raise ValueError(f"photometric_surface is None (off) or (cells_y, cells_x), each 1 .. 8, got {self.photometric_surface!r}")
            if not self.photometric_illumination:
                raise ValueError("photometric_surface needs photometric_illumination=True: the cells are the grid of the lighting "
                                 "model, and a grid without a lighting model means nothing")
            if t != (1, 1):
                raise ValueError("photometric_surface and photometric_tiles exclude each other: the hand-over calls ONE lighting model, "
                                 "the surface for smooth fields or the tiles for edges; both together are not built")
        hb = self.photometric_handback_rejected
        if isinstance(hb, bool) or not isinstance(hb, (int, float)) or not (math.isfinite(float(hb)) and 0.0 <= float(hb) <= 1.0):
            raise ValueError(f"photometric_handback_rejected is 0 (off) or a share in (0, 1], got {hb!r}")
        if hb > 0 and self.photometric_robust_iterations == 0:
            raise ValueError("photometric_handback_rejected needs photometric_robust_iterations > 0: without a re-weighting no row "
                             "is ever rejected")
        if not (math.isfinite(float(self.photometric_handover)) and float(self.photometric_handover) >= 0.0):
            raise ValueError(f"photometric_handover is a finite threshold >= 0 (0 = off), got {self.photometric_handover!r}")
        if isinstance(self.photometric_level, bool) or int(self.photometric_level) != self.photometric_level \
                or not 0 <= int(self.photometric_level) <= 3:
            raise ValueError(f"photometric_level is 0 .. 3, got {self.photometric_level!r}")
        if not (math.isfinite(float(self.photometric_mu)) and float(self.photometric_mu) >= 0.0):
            raise ValueError(f"photometric_mu is finite and >= 0, got {self.photometric_mu!r}")
        if self.photometric_lambda is not None and not math.isfinite(float(self.photometric_lambda)):
            raise ValueError(f"photometric_lambda is a finite gain or None, got {self.photometric_lambda!r}")
        if self.photometric_interaction not in PHOTOMETRIC_INTERACTIONS:
            raise ValueError(f"photometric_interaction is one of {PHOTOMETRIC_INTERACTIONS}, got {self.photometric_interaction!r}")
        if self.photometric_handover > 0 and self.roll_search:
            raise ValueError("photometric_handover does not combine with roll_search: the hand-over watches the plain update's twist")
        if self.roll_search and self.subpatch:
            raise ValueError("roll_search does not combine with subpatch: the sub-patch offsets of a turned copy would have to be "
                             "turned too")
        if self.interaction not in INTERACTIONS:
            raise ValueError(f"interaction is one of {INTERACTIONS}, got {self.interaction!r}")
        if not 1 <= int(self.select_cells) <= 16:
            raise ValueError(f"select_cells is 1 .. 16, got {self.select_cells!r}")
        if self.law not in LAWS:
            raise ValueError(f"law is one of {LAWS}, got {self.law!r}")
        if not 0 <= int(self.pose_robust_iterations) <= 16:
            raise ValueError(f"pose_robust_iterations is 0 .. 16, got {self.pose_robust_iterations!r}")
        if not 0 <= int(self.pose_consensus) <= 4096:
            raise ValueError(f"pose_consensus is 0 .. 4096, got {self.pose_consensus!r}")
        if not 0 <= int(self.pose_consensus_seed) <= 0xFFFFFFFF:
            raise ValueError(f"pose_consensus_seed is 0 .. 2^32 - 1, got {self.pose_consensus_seed!r}")
        if not 0 <= int(self.homography_robust_iterations) <= 16:
            raise ValueError(f"homography_robust_iterations is 0 .. 16, got {self.homography_robust_iterations!r}")
        if not (float(self.homography_depth) > 0.0 and math.isfinite(float(self.homography_depth))):
            raise ValueError(f"homography_depth is a positive, finite length in metres, got {self.homography_depth!r}")
        if not 0 <= int(self.homography_consensus) <= 4096:
            raise ValueError(f"homography_consensus is 0 .. 4096, got {self.homography_consensus!r}")
        if not 0 <= int(self.homography_consensus_seed) <= 0xFFFFFFFF:
            raise ValueError(f"homography_consensus_seed is 0 .. 2^32 - 1, got {self.homography_consensus_seed!r}")
        if not 0 <= int(self.rig_robust_iterations) <= 16:
            raise ValueError(f"rig_robust_iterations is 0 .. 16, got {self.rig_robust_iterations!r}")
        if not 0 <= int(self.rig_pose_robust_iterations) <= 16:
            raise ValueError(f"rig_pose_robust_iterations is 0 .. 16, got {self.rig_pose_robust_iterations!r}")

    @property
    def c_x(self) -> float:
        return self.u_max / 2

    @property
    def c_y(self) -> float:
        return self.v_max / 2

    def intrinsics(self):
        return (self.f_x, self.f_y, self.c_x, self.c_y)

    def replace(self, **kw) -> "ServoParams":
        return dataclasses.replace(self, **kw)


def grid_side(tokens: int) -> int:
    # reference: vitvs_v2.py:75 (int(np.sqrt(T)); square grids only)
    return int(math.sqrt(tokens))


# ------------------------------------------------------------------------------------------------------------------
# The reference's configuration file (catkin_ws/ibvs/config/config.yaml, read by Controller.load_parameters,
# vitvs_v2.py:272-323): the data format on the caller's side of the path.
_REQUIRED_KEYS = (   # load_parameters indexes these with config[...]: a missing one is a KeyError there and here
    "u_max", "v_max", "f_x", "f_y", "lambda_", "min_error", "max_error", "num_pairs", "thresh_filter_keypoints",
    "dino_input_size", "use_feature_binning", "num_samples", "num_circles", "circle_radius_aug",
    "velocity_convergence_threshold", "velocity_threshold_translation", "velocity_threshold_rotation",
    "error_threshold_ratio", "error_threshold_absolute_translation", "error_threshold_absolute_rotation",
    "min_iterations", "max_iterations", "image_path")


@dataclass
class ReferenceConfig:
    """What a ``config.yaml`` of the reference says, split by who reads it here."""
    servo: ServoParams                      # the path: camera model, gain, pairs, input size, binning, EMA, clip
    max_iterations: int                     # ServoLoop(max_iterations=...)                       (vitvs_v2.py:412)
    max_velocity_vector_history: int        # Controller.max_velocity_vector_history              (vitvs_v2.py:627)
    image_path: str                         # goal image, relative to the reference's script directory (:323)
    extras: dict                            # loaded by the reference, never read on the path (sampling, thresholds ...)

    def apply(self, controller=None, loop=None):
        """Copy the run-loop settings onto a ``servo.Controller`` / ``loop.ServoLoop`` built from ``self.servo``."""
        if controller is not None:
            controller.max_velocity_vector_history = self.max_velocity_vector_history
        if loop is not None:
            loop.max_iterations = self.max_iterations
        return self


def load_reference_config(source) -> ReferenceConfig:
    """``source``: path of a YAML file in the reference's schema, or the mapping ``yaml.safe_load`` returned.

    Same required keys as ``Controller.load_parameters`` (a missing one raises ``KeyError`` naming it) and the same
    defaults for the optional ones: ``max_velocity`` 1.0, ``ema_alpha`` 0.1 (NOT the 0.8 the shipped file sets),
    ``max_velocity_vector_history`` 200, ``background_thresh`` 0.5 (vitvs_v2.py:287, 296, 316, 319).  ``robust_iterations`` (this
    project's robust control law, no key of the reference's file) is taken when the mapping carries it, else 0; ``subpatch`` (the
    sub-patch refinement of the matches) likewise, else False; ``interaction`` (which interaction matrix the law inverts) likewise,
    else "current"; ``law`` ("ibvs" / "pose" / "homography"), ``pose_robust_iterations`` and ``rig_pose_robust_iterations`` likewise,
    else "ibvs", 0 and 0; ``homography_robust_iterations`` and ``homography_depth`` likewise, else 0 and 1.0; ``homography_consensus`` and
    ``homography_consensus_seed`` likewise, else 0 and 0; ``pose_consensus`` and ``pose_consensus_seed`` likewise, else 0 and 0;
    ``select_cells`` (the cell grid of selection "best") likewise, else 4;
    ``roll_search`` (the roll search in front of every update) likewise, else False; ``photometric_handover``, ``photometric_level``,
    ``photometric_mu``, ``photometric_lambda`` and ``photometric_interaction`` (the hand-over to the photometric law) likewise, else
    0.0 (off), 2, 0.01, None and "desired"; ``photometric_illumination``, ``photometric_robust_iterations`` and
    ``photometric_sigma_min`` (its robust form) likewise, else False, 0 and 1.0; ``photometric_tiles`` (its tile form, a sequence of
    two) and ``photometric_handback_rejected`` likewise, else (1, 1) and 0.0; ``photometric_surface`` (its surface form, a sequence of
    two) likewise, else None."""
    if isinstance(source, dict):
        cfg = dict(source)
    else:
        import yaml
        with open(source, "r") as fh:
            cfg = yaml.safe_load(fh)
        if not isinstance(cfg, dict):
            raise ValueError(f"{source}: not a mapping")
    for key in _REQUIRED_KEYS:
        if key not in cfg:
            raise KeyError(key)
    servo = ServoParams(u_max=int(cfg["u_max"]), v_max=int(cfg["v_max"]), f_x=float(cfg["f_x"]), f_y=float(cfg["f_y"]),
                        lambda_=float(cfg["lambda_"]), num_pairs=int(cfg["num_pairs"]),
                        dino_input_size=int(cfg["dino_input_size"]), use_feature_binning=bool(cfg["use_feature_binning"]),
                        ema_alpha=float(cfg.get("ema_alpha", 0.1)), max_velocity=float(cfg.get("max_velocity", 1.0)),
                        robust_iterations=int(cfg.get("robust_iterations", 0)), subpatch=bool(cfg.get("subpatch", False)),
                        interaction=str(cfg.get("interaction", "current")),
                        rig_robust_iterations=int(cfg.get("rig_robust_iterations", 0)), law=str(cfg.get("law", "ibvs")),
                        pose_robust_iterations=int(cfg.get("pose_robust_iterations", 0)),
                        pose_consensus=int(cfg.get("pose_consensus", 0)),
                        pose_consensus_seed=int(cfg.get("pose_consensus_seed", 0)),
                        rig_pose_robust_iterations=int(cfg.get("rig_pose_robust_iterations", 0)),
                        homography_robust_iterations=int(cfg.get("homography_robust_iterations", 0)),
                        homography_depth=float(cfg.get("homography_depth", 1.0)),
                        homography_consensus=int(cfg.get("homography_consensus", 0)),
                        homography_consensus_seed=int(cfg.get("homography_consensus_seed", 0)),
                        select_cells=int(cfg.get("select_cells", 4)), roll_search=bool(cfg.get("roll_search", False)),
                        photometric_handover=float(cfg.get("photometric_handover", 0.0)),
                        photometric_level=cfg.get("photometric_level", 2),
                        photometric_mu=float(cfg.get("photometric_mu", 0.01)),
                        photometric_lambda=(None if cfg.get("photometric_lambda") is None else float(cfg["photometric_lambda"])),
                        photometric_interaction=str(cfg.get("photometric_interaction", "desired")),
                        photometric_illumination=cfg.get("photometric_illumination", False),
                        photometric_robust_iterations=cfg.get("photometric_robust_iterations", 0),
                        photometric_sigma_min=cfg.get("photometric_sigma_min", 1.0),
                        photometric_tiles=cfg.get("photometric_tiles", (1, 1)),
                        photometric_handback_rejected=cfg.get("photometric_handback_rejected", 0.0),
                        photometric_surface=cfg.get("photometric_surface", None))
    used = {"roll_search","u_max", "v_max", "f_x", "f_y", "lambda_", "num_pairs", "dino_input_size", "use_feature_binning", "ema_alpha",
            "max_velocity", "max_iterations", "max_velocity_vector_history", "image_path", "robust_iterations",
            "subpatch", "interaction", "rig_robust_iterations", "law", "pose_robust_iterations",
            "rig_pose_robust_iterations", "homography_robust_iterations", "homography_depth",
            "homography_consensus", "homography_consensus_seed", "select_cells", "pose_consensus", "pose_consensus_seed",
            "photometric_handover", "photometric_level", "photometric_mu", "photometric_lambda", "photometric_interaction",
            "photometric_illumination", "photometric_robust_iterations", "photometric_sigma_min", "photometric_tiles",
            "photometric_handback_rejected", "photometric_surface"}
    extras = {k: v for k, v in cfg.items() if k not in used}
    extras.setdefault("background_thresh", 0.5)
    return ReferenceConfig(servo=servo, max_iterations=int(cfg["max_iterations"]),
                           max_velocity_vector_history=int(cfg.get("max_velocity_vector_history", 200)),
                           image_path=str(cfg["image_path"]), extras=extras)
