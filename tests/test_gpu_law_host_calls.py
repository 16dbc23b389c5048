"""The five follow-on laws' host-pointer C entry points (vitvs_{rig,rig_robust,pose,homography,pose_rig}_velocity) called straight
through the library, where the Python wrappers never go: a handle of max_pairs = 3 and max_rows = 8 serving a call of n = 2 pairs
(capacity != count: a field of the handle's device-side block placed at the count, not the capacity, lands on its neighbour), every
optional output passed and then every optional output NULL, caller arrays sized at max_pairs whose rows past the call's must stay
untouched.  Host and device form are the same launch on the same inputs: every comparison is exact.  ViT-S/16 224², synthetic
weights, fp32."""
import ctypes as C

import numpy as np
import pytest
import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib, config, synth, weights
from vitvs_amd.engine import Engine

import pose_rig_ref as rr
import rig_ref as rg
import law_support as ls

pytestmark = pytest.mark.gpu

KEY = "vits16_224"
P, R, N = 3, 8, 2                       # max_pairs, max_rows, the call's pairs
SENTINEL = {np.float64: -777.25, np.int32: -777}
F, I = np.float64, np.int32

# law -> (inputs in the entry point's order, the scalars between inputs and outputs, outputs (name, shape of a row, type, one row
# per pair?) in the entry point's order: the first two are mandatory, the rest optional)
LAWS = {
    "rig": (("cVr", "status"), (),
            (("v", (6,), F, False), ("law_status", (1,), I, False), ("info", (8,), I, False), ("normal", (28,), F, False))),
    "rig_robust": (("cVr", "status", "K"), (4,),
                   (("v", (6,), F, False), ("law_status", (1,), I, False), ("info", (8,), I, False), ("normal", (28,), F, False),
                    ("weights", (R,), F, True), ("sigma", (1,), F, False))),
    "pose": (("K", "status"), (4,),
             (("v", (6,), F, True), ("law_status", (), I, True), ("pose", (12,), F, True), ("info", (8,), I, True),
              ("weights", (R,), F, True), ("sigma", (), F, True))),
    "homography": (("K", "status"), (0.7, 4),
                   (("v", (6,), F, True), ("law_status", (), I, True), ("H", (9,), F, True), ("info", (8,), I, True),
                    ("weights", (R,), F, True), ("sigma", (), F, True))),
    "pose_rig": (("rTc", "K", "status"), (4,),
                 (("v", (6,), F, False), ("law_status", (1,), I, False), ("pose", (12,), F, False), ("info", (8,), I, False),
                  ("moments", (18,), F, False), ("weights", (R,), F, True), ("sigma", (1,), F, False))),
}


@pytest.fixture(scope="module")
def call():
    """One velocity call of N pairs on a handle for P, and the laws' inputs in caller arrays of P rows (rows N .. P - 1 are the
    sentinel: nothing may read them either)."""
    cfg = config.baseline_config(KEY)
    params = config.ServoParams(dino_input_size=cfg.img_size, use_feature_binning=False, num_pairs=R)
    des, cur = synth.frame_pair(cfg.img_size, synth.ACCEPTED_FRAME_SEEDS[KEY])
    curs = np.stack([np.roll(cur, shift=2 * c - 2, axis=1).copy() for c in range(N)])
    depth = np.stack([np.roll(synth.depth_pattern(), 7 * c, axis=1) for c in range(N)])
    eng = Engine(cfg, params, precision="fp32", max_pairs=P, max_rows=R).load_state_dict(weights.synthetic_state_dict(cfg, 0))
    eng.set_goal_depth(np.stack([ls.goal_depth_of(s) for s in range(N)]))
    g = torch.Generator().manual_seed(11)
    order = torch.stack([torch.randperm(cfg.tokens, generator=g) for _ in range(N)]).to(torch.int32)
    _, st = eng.compute_velocity(curs, np.stack([des] * N), depth, params.intrinsics(), mode=_lib.SELECT_ORDER, selection=order)
    torch.cuda.synchronize()
    rng = np.random.default_rng(5)
    inputs = dict(cVr=np.full((P, 36), SENTINEL[F]), K=np.full((P, 4), SENTINEL[F]), rTc=np.full((P, 12), SENTINEL[F]),
                  status=np.full(P, SENTINEL[I], I))
    inputs["cVr"][:N] = np.stack([rg.twist_matrix(*rg.random_extrinsic(rng)).reshape(36) for _ in range(N)])
    inputs["K"][:N] = params.intrinsics()
    inputs["rTc"][:N] = rr.rtc_rows(rr.seeded_rig(rng, N))
    inputs["status"][:N] = st.cpu().numpy()
    print("velocity statuses", inputs["status"][:N])
    yield dict(eng=eng, inputs=inputs)
    eng.close()


def _outputs(spec):
    """caller arrays at the capacity, pre-filled with the sentinel"""
    return {name: np.full(((P,) if per_pair else ()) + row, SENTINEL[t], t) for name, row, t, per_pair in spec}


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("law", list(LAWS))
def test_host_form_is_the_device_form_at_a_count_below_the_capacity(call, law):
    eng, lib = call["eng"], call["eng"].lib
    names, scalars, spec = LAWS[law]
    ins = [call["inputs"][name] for name in names]

    # the device form, every optional output asked for, on tensors that hold the call's rows only
    dev_in = [torch.from_numpy(np.ascontiguousarray(a[:N])).to(eng.device) for a in ins]
    dev_out = {name: torch.from_numpy(a).to(eng.device) for name, a in _outputs(spec).items()}
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rc = getattr(lib, f"vitvs_{law}_velocity_dev")(eng.handle, N, *map(p, dev_in), *scalars, *map(p, dev_out.values()),
                                                    C.c_void_p(torch.cuda.current_stream(eng.device).cuda_stream))
    assert rc == 0, _lib.last_error(eng.handle)
    torch.cuda.synchronize()
    ref = {name: t.cpu().numpy() for name, t in dev_out.items()}
    print(law, "law status", ref["law_status"].reshape(-1)[:N], "v", ref["v"].reshape(-1, 6)[:N])
    assert ref["v"].reshape(-1, 6)[:N].any(), "choose other inputs: the law returned no twist, equal outputs would say little"

    # the host-pointer form: every optional output, then none of them
    q = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    host = getattr(lib, f"vitvs_{law}_velocity")
    full, bare = _outputs(spec), _outputs(spec)
    assert host(eng.handle, N, *map(q, ins), *scalars, *map(q, full.values())) == 0, _lib.last_error(eng.handle)
    mandatory = [name for name, *_ in spec[:2]]
    optional = [None] * (len(spec) - 2)
    assert host(eng.handle, N, *map(q, ins), *scalars, *(q(bare[name]) for name in mandatory), *optional) == 0, \
        _lib.last_error(eng.handle)

    for name, row, t, per_pair in spec:
        rows = N if per_pair else None                            # what the call writes: the first N rows, or the whole array
        assert _same(full[name][:rows], ref[name][:rows]), (law, name, "host form != device form")
        if name in mandatory:
            assert _same(bare[name][:rows], ref[name][:rows]), (law, name, "without optional outputs != device form")
        if per_pair:
            for got in (full[name], bare[name] if name in mandatory else full[name], ref[name]):
                assert (got[N:] == SENTINEL[t]).all(), (law, name, "rows past the call's pairs were written")
    for name, a in zip(names, ins):
        assert (a[N:] == SENTINEL[a.dtype.type]).all(), (law, name)
