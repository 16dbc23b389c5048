"""What the tiny-handle tests of the control laws share (tests/test_gpu_servo_cover.py, test_gpu_robust_law.py,
test_gpu_interaction.py, test_gpu_refine.py, test_gpu_select*.py, test_gpu_pose*.py, test_gpu_homography*.py, test_gpu_rig*.py,
test_gpu_law_host_calls.py): the weight-less configuration, the random tables, depth images and intrinsics the cases are made
of, the oracle's law, servo.hip's pivot rule restated, and the cache of tiny handles.

Every helper draws from the generator it is given in a fixed order: the cases of the tests are defined by their seeds.

Handles live per test module: a module makes its own ``ENGINES = TinyEngines()`` and imports ``close_engines``, which closes
that module's handles at its teardown.  There is no cache across modules."""
import dataclasses

import numpy as np
import pytest
import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib, config, synth
from vitvs_amd.engine import Engine
from oracle import servo_ref as sr
import rig_ref as rg
import robust_ref as rr
import solve_ref as sv

N_CAMERAS = 3           # the rig tests' cameras
LAW_OPTIONS = ("robust_law", "subpatch", "interaction")     # what a follow-on law's tests switch off on every fetch


def tiny_cfg(img):
    base = config.vit_config("dino_vits16", img)
    return dataclasses.replace(base, dim=128, depth=2, heads=2, layer=1, native_grid=base.grid)


class TinyEngines:
    """One module's tiny handles (no weights: the law alone) for g x g grids of 16-pixel patches, made on first use."""

    def __init__(self):
        self.engines = {}

    def fetch(self, g, max_rows, max_pairs=1, lam=None, reset=()):
        """(Engine, params) for the key; the options named in `reset` are set to 0 on every fetch."""
        key = (g, max_rows, max_pairs, lam)
        if key not in self.engines:
            img = 16 * g
            params = config.ServoParams(dino_input_size=img) if lam is None else config.ServoParams(dino_input_size=img, lambda_=lam)
            self.engines[key] = (Engine(tiny_cfg(img), params, precision="fp32", max_pairs=max_pairs, max_rows=max_rows), params)
        eng, params = self.engines[key]
        for option in reset:
            eng.set_option(option, 0)
        return eng, params

    def close(self):
        for eng, _ in self.engines.values():
            eng.close()
        self.engines.clear()


@pytest.fixture(scope="module", autouse=True)
def close_engines(request):
    """Closes the importing module's ``ENGINES`` when its last test has run."""
    yield
    request.module.ENGINES.close()


def tables(rng, t, n_boost):
    """Arg-max tables of a random similarity matrix with `n_boost` planted mutual nearest neighbours."""
    S = rng.uniform(0.2, 0.8, size=(t, t)).astype(np.float32)
    S[rng.permutation(t)[:n_boost], rng.permutation(t)[:n_boost]] = rng.uniform(0.85, 0.95, size=n_boost).astype(np.float32)
    sim1, nn1, _, nn2 = sr.nearest_neighbours(torch.from_numpy(S))
    nn1, nn2 = nn1.numpy().astype(np.int64), nn2.numpy().astype(np.int64)
    mutual = np.nonzero(nn2[nn1] == np.arange(t))[0]
    assert 0 < len(mutual) < t
    return nn1, nn2, sim1.numpy(), mutual


def depth(rng):
    depth = synth.depth_pattern().copy()
    depth.reshape(-1)[rng.integers(0, depth.size, size=depth.size // 7)] = 0     # holes: the 100 m sentinel
    return depth


def goal_depth(rng, holes=True):
    """Another depth image with holes: the goal pose's (a transposed-and-flipped pattern, so Z* differs from Z nearly everywhere)."""
    d = np.ascontiguousarray(synth.depth_pattern()[::-1, ::-1]).copy()
    d = (d.astype(np.int64) + 137).clip(1, 65535).astype(np.uint16)
    if holes:
        d.reshape(-1)[rng.integers(0, d.size, size=d.size // 7)] = 0
    return d


def goal_depth_of(seed):
    """goal_depth with a generator and a level of its own per seed (one goal image per camera of a rig)."""
    rng = np.random.default_rng(seed)
    d = np.ascontiguousarray(synth.depth_pattern()[::-1, ::-1]).copy()
    d = (d.astype(np.int64) + 137 + 11 * seed).clip(1, 65535).astype(np.uint16)
    d.reshape(-1)[rng.integers(0, d.size, size=d.size // 7)] = 0
    return d


def intrinsics(rng, params):
    return (float(rng.uniform(300, 700)), float(rng.uniform(300, 700)), params.u_max / 2 + float(rng.uniform(-20, 20)),
            params.v_max / 2 + float(rng.uniform(-20, 20)))


def oracle(g, img, params, nn1, ids, rows, depth, K):
    ids = np.asarray(ids, np.int64)
    p1 = torch.from_numpy(np.stack([ids // g, ids % g], 1))
    p2 = torch.from_numpy(np.stack([nn1[ids] // g, nn1[ids] % g], 1))
    s_star, s_ = sr.calculate_uv(sr.patch_centres(p1, img, g), sr.patch_centres(p2, img, g), rows, params.u_max, params.v_max, img)
    return np.asarray(s_star), np.asarray(s_), sr.velocity(s_star, s_, depth, K[0], K[1], K[2], K[3], params.lambda_)


def ldlt_passes(L):
    """servo.hip's pivot test on the normal equations of L (rows x 6), restated in fp64 (tests/solve_ref.py, which owns the
    threshold)."""
    return sv.ldlt_passes(L)


def planted_case(engines, g, seed, num_pairs, share=0.125):
    """(eng, params, scenario): rr.planted_scenario with random intrinsics and holes, for the module's 130-row handle with every
    follow-on option off."""
    eng, params = engines.fetch(g, 130, reset=LAW_OPTIONS)
    rng = np.random.default_rng(seed)
    return eng, params, rr.planted_scenario(rng, num_pairs, share, params, K=intrinsics(rng, params), g=g, holes=True)


def s_min(params, img, K):
    return rr.sigma_min(16, params.u_max, params.v_max, img, K[0], K[1])


def pitches(params, stride, img):
    return stride * params.u_max / img, stride * params.v_max / img


def host(info):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in info.items()}


def same_values(a, b):
    """Two dicts of arrays with the same keys and equal values, NaNs in the same places."""
    return sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


def goal_table(zg, g, img, params):
    """The handle's goal-depth table restated: zg at every token's patch centre (0 where that lies outside the image: the law
    reads it as 100 m, like a hole), entry T at pixel (0, 0)."""
    uv = rr.token_pixels(np.arange(g * g), g, img, params.u_max, params.v_max)
    inside = (uv[:, 0] < params.u_max) & (uv[:, 1] < params.v_max)
    at = np.where(inside[:, None], uv, 0)
    return np.concatenate([np.where(inside, zg[at[:, 1], at[:, 0]], 0), zg[0:1, 0]]).astype(np.uint16)


def servo_law(eng, sc, num_pairs=None, ids=None, select=_lib.SELECT_EXPLICIT, offsets=None, depth=True):
    """servo_from_nn on a scenario's tables (its own ids and pair count unless others are given; without the depth image where
    depth is False): (v_c on the host, status)."""
    ids = sc["ids"] if ids is None else ids
    k = len(sc["ids"]) if num_pairs is None else num_pairs
    v, st = eng.servo_from_nn(sc["nn_1"], sc["nn_2"], sc["sim_1"], sc["depth"] if depth else None, sc["K"], mode=select,
                              selection=[ids] if select == _lib.SELECT_EXPLICIT else ids, num_pairs=k, offsets=offsets)
    return v.cpu().numpy(), int(st)


def snapshot(eng, v):
    det = eng.last_details(1)
    return dict(det, v_c=np.array(v, copy=True))


# ----------------------------------------------------------------------------- the rig tests' scenario dict `s`
def order(cfg, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randperm(cfg.tokens, generator=g) for _ in range(n)]).to(torch.int32)


def rig_velocity(s, eng=None, r=0, n=N_CAMERAS, seed=11):
    eng = eng or s["eng"]
    return eng.compute_velocity(s["curs"][r][:n], s["des"][:n], s["depth"][:n], s["params"].intrinsics(), mode=_lib.SELECT_ORDER,
                                selection=order(s["cfg"], n, seed))


def extrinsics(seed=3, n=N_CAMERAS):
    rng = np.random.default_rng(seed)
    return [rg.random_extrinsic(rng, 0.3, 0.2) for _ in range(n)]
