"""Handle to the HIP hot path (libvitvs_hip.so) for one extractor configuration on one GPU.

PyTorch is used here only as plumbing: device buffers (``tensor.data_ptr()``), the current HIP
stream, and host-side weight preparation.  All arithmetic of the path runs in the HIP kernels
behind the C ABI (include/vitvs.h); nothing here falls back to torch ops or to the CPU oracle.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from .config import INTERACTIONS, ServoParams, ViTConfig
from .weights import check_state_dict, resample_pos_embed


class VitvsError(RuntimeError):
    pass


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream_ptr(device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class _Staging:
    """What a call's host-pointer form (``_HostStaging``: numpy arrays) and its device form (``_DeviceStaging``: tensors on the
    engine's device, torch's current stream) make their C calls of.  The checks and layouts are written once, here, on what numpy
    and torch share; a subclass says how an argument is read (``array``), where the call reads it (``put``), what an output is
    (``f64``, ``i32``), how it comes back (``read``), an array's pointer (``ptr``) and the call's trailing arguments (``stream``)."""

    def frames(self, a, n, shape):
        """uint8 frames ``[n, h, w, 3]``, ``[h, w, 3]`` for one.  ``n`` None: any number of them; ``shape`` = (h, w), None: any one geometry."""
        a = self.array(a)
        a = a[None] if a.ndim == 3 else a
        if a.dtype != self.xp.uint8 or a.ndim != 4 or a.shape[3] != 3 or (n is not None and a.shape[0] != n) \
                or (shape is not None and tuple(a.shape[1:3]) != tuple(shape)):
            h, w = shape or "HW"
            raise VitvsError(f"frames must be uint8 [{'n' if n is None else n},{h},{w},3], all of one shape, "
                             f"got {a.dtype} {tuple(a.shape)}")
        return self.put(a)

    def depth(self, Z, n, hw):
        """``Z``: the sensor's uint16 millimetre image of every pair, ``[n, h, w]`` (``[h, w]`` for one; ``n`` None: as many as it
        holds), or None."""
        if Z is None:
            return None
        z, hw = self.array(Z), tuple(hw)
        if n is None and z.ndim in (2, 3):
            n = 1 if z.ndim == 2 else int(z.shape[0])
        if z.dtype != self.xp.uint16 or tuple(z.shape[-2:]) != hw or n is None or math.prod(z.shape) != n * hw[0] * hw[1]:
            raise VitvsError(f"depth must be the sensor's uint16 millimetre image(s) [v_max, u_max] of the call's geometry, "
                             f"[{n or 'n'},{hw[0]},{hw[1]}], got {z.dtype} {tuple(z.shape)}")
        return self.put(z.reshape((n,) + hw))

    def intrinsics(self, K, n, who="pair", error=VitvsError):
        """``K`` as float64 ``[n, 4]``: one (fx, fy, cx, cy) per ``who``, or one for all."""
        k = self.array(K, "float64").reshape(-1, 4)
        if k.shape[0] == 1 and n > 1:
            k = self.xp.broadcast_to(k, (n, 4))
        if k.shape[0] != n:
            raise error(f"K is one (fx, fy, cx, cy) for all, or one per {who}")
        return self.put(k)

    def selection(self, mode, selection, n, tokens, k):
        """The selection as the int32 arrays the C ABI takes: (ids [n, k], counts [n]) for EXPLICIT — ``selection`` one id list per
        pair, or the one pair's ids —, (visiting order [n, tokens], None) for ORDER, (None, None) for DENSE and BEST."""
        if mode in (_lib.SELECT_DENSE, _lib.SELECT_BEST) or (selection is None and mode not in (_lib.SELECT_ORDER, _lib.SELECT_EXPLICIT)):
            return None, None                               # nothing comes from the caller (an unknown mode is the library's to refuse)
        if selection is None:
            raise VitvsError("this selection mode needs a selection array")
        if mode != _lib.SELECT_EXPLICIT:
            return self.put(self.array(selection, "int32").reshape(n, tokens)), None
        rows = selection if isinstance(selection, (list, tuple)) else [selection]
        if len(rows) != n:
            raise VitvsError("one id list per pair expected")
        sel, cnt = np.zeros((n, k), np.int32), np.zeros(n, np.int32)
        for b, ids in enumerate(rows):
            ids = np.asarray(ids.cpu() if torch.is_tensor(ids) else ids, np.int32).reshape(-1)[:k]
            sel[b, :ids.size] = ids
            cnt[b] = ids.size
        return self.put(self.array(sel)), self.put(self.array(cnt))

    def status(self, status):
        """The velocity call's statuses as a law's call reads them: contiguous int32 [n] (a device tensor stays on the device)."""
        return self.put(self.array(status, "int32").reshape(-1))


class _HostStaging(_Staging):
    """numpy in, numpy out, one synchronous C call: needs neither a handle nor a device, so one instance serves every engine."""
    xp, stream = np, ()

    def array(self, a, dtype=None):
        return np.asarray(a.cpu() if torch.is_tensor(a) else a, dtype)

    put = staticmethod(np.ascontiguousarray)                # (no copy of what is contiguous already)
    read = staticmethod(lambda a: a)

    def f64(self, *shape):
        return np.zeros(shape)

    def i32(self, *shape):
        return np.zeros(shape, np.int32)

    def ptr(self, a):
        return None if a is None else a.ctypes.data_as(C.c_void_p)


class _DeviceStaging(_Staging):
    """Tensors on ``device``, the call enqueued on torch's current stream; nothing here synchronises but ``read``."""
    xp, ptr = torch, staticmethod(_ptr)

    def __init__(self, device):
        self.device = device

    def array(self, a, dtype=None):
        return torch.as_tensor(a, dtype=dtype and getattr(torch, dtype))

    def put(self, a):
        return a.to(self.device).contiguous()

    def read(self, a):
        return a.cpu().numpy()

    def f64(self, *shape):
        return torch.empty(shape, dtype=torch.float64, device=self.device)

    def i32(self, *shape):
        return torch.empty(shape, dtype=torch.int32, device=self.device)

    @property
    def stream(self):
        return (_stream_ptr(self.device),)


_HOST = _HostStaging()


class Engine:
    """One ``vitvs_handle``: device weights + workspaces for up to ``max_pairs`` frame pairs."""

    def __init__(self, cfg: ViTConfig, params: ServoParams = None, *, precision: str = "fp32", max_pairs: int = 1,
                 max_rows: Optional[int] = None, binned: Optional[bool] = None, device=None):
        if not torch.cuda.is_available():
            raise VitvsError("no HIP device: the ViT-VS hot path has no CPU fallback")
        self.lib = _lib.load()
        self.cfg = cfg
        given = params or ServoParams(dino_input_size=cfg.img_size)
        self.params = given.replace(robust_iterations=0, subpatch=False, interaction="current", select_cells=4)   # a fresh handle's law: apply_law_params
        # "f16x2": split-f16 (include/vitvs.h VITVS_F16X2) — fp32-class results on the f16 matrix cores, the parity mode at servo rate
        self.precision = {"fp32": _lib.F32, "f32": _lib.F32, "bf16": _lib.BF16, "fp16": _lib.F16, "f16": _lib.F16,
                          "f16x2": _lib.F16X2, "split-f16": _lib.F16X2}[precision]
        self.precision_name = {_lib.F32: "fp32", _lib.BF16: "bf16", _lib.F16: "fp16", _lib.F16X2: "f16x2"}[self.precision]
        self.binned = self.params.use_feature_binning if binned is None else bool(binned)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.max_pairs = int(max_pairs)
        # capacity in feature pairs per frame pair: the reference's rotation search raises num_pairs to 48 for its calls
        # (vitvs_v2.py:1151-1189), so that is the default floor
        self.max_rows = int(max_rows) if max_rows is not None else max(int(self.params.num_pairs), 48)
        c = _lib.VitvsConfig()
        c.abi_version = _lib.ABI_VERSION
        c.img_size, c.patch, c.stride, c.dim = cfg.img_size, cfg.patch, cfg.stride, cfg.dim
        c.heads, c.blocks, c.layerscale = cfg.heads, cfg.blocks_run, int(cfg.layerscale)
        for i in range(3):
            c.mean[i] = cfg.mean[i]
            c.std[i] = cfg.std[i]
        c.ln_eps = cfg.ln_eps
        c.precision = self.precision
        c.binned = int(self.binned)
        c.num_pairs = self.params.num_pairs
        c.u_max, c.v_max = self.params.u_max, self.params.v_max
        c.lambda_ = self.params.lambda_
        c.max_pairs, c.max_rows = self.max_pairs, self.max_rows
        self._c = c
        self.handle = C.c_void_p()
        with torch.cuda.device(self.device):
            if cfg.registers:
                rc = self.lib.vitvs_create_ex(C.byref(c), cfg.registers, C.byref(self.handle))
            else:
                rc = self.lib.vitvs_create(C.byref(c), C.byref(self.handle))
        if rc != 0:
            raise VitvsError(f"vitvs_create failed ({rc}): {_lib.last_error(None)}")
        self.frame_size = (cfg.img_size, cfg.img_size)   # geometry of the frames the calls take (set_frame_size)
        self._last_host_pairs = 1                         # pairs of the last host-pointer velocity call (reselect_host)
        self.tokens = self.lib.vitvs_tokens(self.handle)
        self.desc_dim = self.lib.vitvs_desc_dim(self.handle)
        assert self.tokens == cfg.tokens and self.lib.vitvs_register_tokens(self.handle) == cfg.registers
        self.apply_law_params(given)

    # ------------------------------------------------------------------ lifetime
    def close(self):
        if getattr(self, "handle", None) is not None and self.handle.value:
            self.lib.vitvs_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str):
        if rc < 0:
            raise VitvsError(f"{what} failed ({rc}): {_lib.last_error(self.handle)}")
        return rc

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> "Engine":
        """Upload a DINO / timm / DINOv2 state dict (fp32).  ``pos_embed`` is resampled to this
        handle's token grid on the host first (reference: dinov2_extractor.py:94-118)."""
        check_state_dict(self.cfg, sd)
        for name, t in sd.items():
            if name == "pos_embed":
                t = resample_pos_embed(t, self.cfg.grid)
            elif name.startswith("blocks."):
                if int(name.split(".")[1]) >= self.cfg.blocks_run:
                    continue
            elif name not in ("patch_embed.proj.weight", "patch_embed.proj.bias", "cls_token", "register_tokens"):
                continue
            a = np.ascontiguousarray(t.detach().to(torch.float32).cpu().numpy())
            rc = self.lib.vitvs_set_tensor(self.handle, name.encode(), _HOST.ptr(a), a.size)
            self._check(rc, f"vitvs_set_tensor({name})")
        self._check(self.lib.vitvs_weights_ready(self.handle), "vitvs_weights_ready")
        return self

    def share_weights(self, owner: "Engine") -> "Engine":
        """Borrow ``owner``'s device weights instead of uploading a copy (``vitvs_share_weights``): same network, input
        geometry and precision; ``owner`` must stay alive as long as this engine."""
        self._check(self.lib.vitvs_share_weights(self.handle, owner.handle), "vitvs_share_weights")
        self._weights_owner = owner                      # keeps the owner (and its device memory) alive
        return self

    # ------------------------------------------------------------------ helpers
    def _stage(self, host: bool) -> _Staging:
        """The staging of a call's host-pointer or device form; the device one is made on an engine's first device call, so that an
        engine without a device can still check arguments."""
        if host:
            return _HOST
        if "_device_staging" not in self.__dict__:
            self._device_staging = _DeviceStaging(self.__dict__.get("device"))
        return self._device_staging

    def _frames(self, frames) -> torch.Tensor:
        return self._stage(False).frames(frames, None, self.frame_size)

    def set_frame_size(self, height: Optional[int] = None, width: Optional[int] = None) -> "Engine":
        """Declare the geometry of the frames handed to this engine from now on: camera frames uint8 [height, width, 3]
        instead of [S, S, 3].  The reference's ``image.resize((S, S))`` (PIL bicubic, vitvs_v2.py:474-475) then happens
        inside the launch that builds the patch rows (bit-identical to PIL, no resized image in memory).  No arguments:
        back to frames at S x S."""
        s = self.cfg.img_size
        h, w = (0, 0) if height is None or (height, width) == (s, s) else (int(height), int(width))
        rc = self.lib.vitvs_set_frame_size(self.handle, h, w)
        self._check(rc, "vitvs_set_frame_size")
        self.frame_size = (h, w) if h else (s, s)
        return self

    # ------------------------------------------------------------------ seams
    def forward_tokens(self, frames) -> torch.Tensor:
        """Residual stream after block ``layer``: float32 [n, 1+R+T, D] (the hooked tensor,
        reference: dinov2_extractor.py:198-199; rows cls, the R register tokens, the patches)."""
        f = self._frames(frames)
        n = f.shape[0]
        out = torch.empty((n, self.cfg.seq, self.cfg.dim), dtype=torch.float32, device=self.device)
        rc = self.lib.vitvs_forward_tokens_dev(self.handle, n, _ptr(f), _ptr(out), _stream_ptr(self.device))
        self._check(rc, "vitvs_forward_tokens_dev")
        return out

    def resize_frames(self, frames) -> torch.Tensor:
        """Camera frames uint8 [n,h,w,3] (or [h,w,3]) -> uint8 [n,S,S,3] on the device, bit-identical to
        ``PIL.Image.resize((S, S))`` (the reference's resize in front of the path, vitvs_v2.py:474-475)."""
        f = torch.as_tensor(np.ascontiguousarray(frames)) if not torch.is_tensor(frames) else frames
        if f.dim() == 3:
            f = f[None]
        if f.dtype != torch.uint8 or f.dim() != 4 or f.shape[-1] != 3:
            raise ValueError("frames must be uint8 [n,h,w,3]")
        f = f.to(self.device).contiguous()
        n, h, w, _ = f.shape
        s = self.cfg.img_size
        out = torch.empty((n, s, s, 3), dtype=torch.uint8, device=self.device)
        rc = self.lib.vitvs_resize_frames_dev(self.handle, n, _ptr(f), h, w, _ptr(out), _stream_ptr(self.device))
        self._check(rc, "vitvs_resize_frames_dev")
        return out

    FACETS = ("query", "key", "value", "token")

    def extract_descriptors(self, frames, facet: str = "token", bin: Optional[bool] = None,
                            include_cls: bool = False) -> torch.Tensor:
        """``ViTExtractor.extract_descriptors(batch, layer, facet, bin, include_cls)`` (dinov2_extractor.py:313-337):
        [n,1,T,D], [n,1,T,9D] with ``bin`` (3x3 log-bin of that facet), [n,1,1+T,D] with ``include_cls``.  facet 'token' (the
        servo path's choice) or 'query' / 'key' / 'value' (descriptor index d*H + h like the reference).  ``bin=None``: the
        engine's ``use_feature_binning`` for the token facet, False for the others.  ``bin`` with ``include_cls`` raises the
        reference's AssertionError; an unknown facet its TypeError-like message."""
        if facet not in self.FACETS:
            raise TypeError(f"{facet} is not a supported facet.")                # the reference's message
        binned = (self.binned if facet == "token" else False) if bin is None else bool(bin)
        if binned and include_cls:
            raise AssertionError("bin = True and include_cls = True are not supported together, set one of them False.")
        f = self._frames(frames)
        n = f.shape[0]
        if facet == "token" and not include_cls and binned == self.binned:      # the velocity path's own descriptors
            out = torch.empty((n, 1, self.tokens, self.desc_dim), dtype=torch.float32, device=self.device)
            rc = self.lib.vitvs_extract_descriptors_dev(self.handle, n, _ptr(f), _ptr(out), _stream_ptr(self.device))
            self._check(rc, "vitvs_extract_descriptors_dev")
            return out
        rows = self.tokens + (1 if include_cls else 0)
        out = torch.empty((n, 1, rows, self.cfg.dim * (9 if binned else 1)), dtype=torch.float32, device=self.device)
        rc = self.lib.vitvs_extract_descriptors_ex_dev(self.handle, n, _ptr(f), self.FACETS.index(facet), int(binned),
                                                       int(include_cls), _ptr(out), _stream_ptr(self.device))
        self._check(rc, "vitvs_extract_descriptors_ex_dev")
        return out

    def extract_saliency_maps(self, frames, head_idxs=(0, 2, 4, 5)) -> torch.Tensor:
        """``ViTExtractor.extract_saliency_maps(batch)`` (dinov2_extractor.py:339-353): the class token's attention over the
        patch tokens in block ``layer`` (the reference hooks block 11), averaged over ``head_idxs`` and min-max normalised per
        image: float32 [n, T] in [0, 1].  Like the reference, only for ``dino_vits8`` (its assertion, same message)."""
        assert self.cfg.model_type == "dino_vits8", "saliency maps are supported only for dino_vits model_type."
        f = self._frames(frames)
        n = f.shape[0]
        heads = (C.c_int32 * len(head_idxs))(*[int(i) for i in head_idxs])
        out = torch.empty((n, self.tokens), dtype=torch.float32, device=self.device)
        rc = self.lib.vitvs_extract_saliency_dev(self.handle, n, _ptr(f), len(head_idxs), heads, _ptr(out),
                                                 _stream_ptr(self.device))
        self._check(rc, "vitvs_extract_saliency_dev")
        return out

    def correspond(self, desc1: torch.Tensor, desc2: torch.Tensor, want_matrix: bool = False):
        """Similarity + argmax stage of find_correspondences_batch on [T,D] descriptors."""
        d1 = desc1.to(self.device, torch.float32).contiguous()
        d2 = desc2.to(self.device, torch.float32).contiguous()
        t, d = d1.shape
        pad = (-d) % 32
        if pad:  # zero columns leave cosine similarities unchanged
            d1 = torch.nn.functional.pad(d1, (0, pad))
            d2 = torch.nn.functional.pad(d2, (0, pad))
        nn1 = torch.empty(t, dtype=torch.int32, device=self.device)
        nn2 = torch.empty(t, dtype=torch.int32, device=self.device)
        sim1 = torch.empty(t, dtype=torch.float32, device=self.device)
        smat = torch.empty((t, t), dtype=torch.float32, device=self.device) if want_matrix else None
        rc = self.lib.vitvs_correspond_dev(self.handle, t, d + pad, _ptr(d1), _ptr(d2), _ptr(nn1), _ptr(nn2),
                                           _ptr(sim1), _ptr(smat), _stream_ptr(self.device))
        self._check(rc, "vitvs_correspond_dev")
        return (nn1, nn2, sim1, smat) if want_matrix else (nn1, nn2, sim1)

    def refine(self, desc1: torch.Tensor, desc2: torch.Tensor, nn_1) -> torch.Tensor:
        """``vitvs_refine_dev``: the sub-patch offsets (option ``subpatch``) of every token's match on [T, D] descriptors and a
        given ``nn_1`` [T]: float32 [T, 2] = (dr, dc) in patch pitches, on the device."""
        d1 = desc1.to(self.device, torch.float32).contiguous()
        d2 = desc2.to(self.device, torch.float32).contiguous()
        t, d = d1.shape
        pad = (-d) % 32
        if pad:  # zero columns leave cosine similarities unchanged
            d1 = torch.nn.functional.pad(d1, (0, pad))
            d2 = torch.nn.functional.pad(d2, (0, pad))
        nn1 = torch.as_tensor(nn_1).to(self.device, torch.int32).contiguous()
        off = torch.empty((t, 2), dtype=torch.float32, device=self.device)
        rc = self.lib.vitvs_refine_dev(self.handle, t, d + pad, _ptr(d1), _ptr(d2), _ptr(nn1), _ptr(off), _stream_ptr(self.device))
        self._check(rc, "vitvs_refine_dev")
        return off

    def _num_pairs(self, num_pairs) -> int:
        k = int(self.params.num_pairs if num_pairs is None else num_pairs)
        if not 1 <= k <= self.max_rows:
            raise VitvsError(f"num_pairs {k} outside 1..max_rows ({self.max_rows})")
        return k

    def _selection_args(self, mode, selection, n_pairs, tokens, num_pairs=None):
        """The device form's selection tensors, for callers that lay out a ``compute_velocity_dev`` call themselves."""
        k = self._num_pairs(num_pairs) if mode == _lib.SELECT_EXPLICIT else 0
        return self._stage(False).selection(mode, selection, n_pairs, tokens, k)

    def _selection_arrays_host(self, mode, selection, n, k):
        """The same as numpy arrays, for a host-pointer call."""
        return _HOST.selection(mode, selection, n, self.tokens, k)

    def servo_from_nn(self, nn_1, nn_2, sim_1, depth, K, mode=_lib.SELECT_DENSE, selection=None, num_pairs=None, offsets=None):
        """Control law on given nearest-neighbour tables (one pair); ``num_pairs`` as in ``compute_velocity``.  ``offsets``
        float32 [T, 2]: the sub-patch offsets (dr, dc) of every token's match (``vitvs_servo_from_nn_ex_dev``); None: patch centres."""
        nn1 = torch.as_tensor(nn_1).to(self.device, torch.int32).contiguous()
        nn2 = torch.as_tensor(nn_2).to(self.device, torch.int32).contiguous()
        s1 = torch.as_tensor(sim_1).to(self.device, torch.float32).contiguous()
        t = nn1.numel()
        stage = self._stage(False)
        z = stage.depth(depth, 1, (self.params.v_max, self.params.u_max))
        kk = stage.intrinsics(K, 1)
        k = self._num_pairs(num_pairs)
        sel, cnt = stage.selection(mode, selection, 1, t, k)
        v = torch.zeros((1, 6), dtype=torch.float64, device=self.device)
        st = torch.zeros(1, dtype=torch.int32, device=self.device)
        n_sel = int(cnt[0].item()) if cnt is not None else 0
        if offsets is None:
            rc = self.lib.vitvs_servo_from_nn_dev(self.handle, t, _ptr(nn1), _ptr(nn2), _ptr(s1), _ptr(z), _ptr(kk), mode,
                                                  _ptr(sel), n_sel, k, _ptr(v), _ptr(st), _stream_ptr(self.device))
        else:
            off = torch.as_tensor(offsets).to(self.device, torch.float32).contiguous()
            if tuple(off.shape) != (t, 2):
                raise VitvsError("offsets must be [T, 2]")
            rc = self.lib.vitvs_servo_from_nn_ex_dev(self.handle, t, _ptr(nn1), _ptr(nn2), _ptr(s1), _ptr(z), _ptr(kk), mode,
                                                     _ptr(sel), n_sel, k, _ptr(off), _ptr(v), _ptr(st), _stream_ptr(self.device))
        self._check(rc, "vitvs_servo_from_nn_dev")
        self._last_tokens = t
        return v[0], st[0]

    # ------------------------------------------------------------------ the hot path
    def set_goal(self, I_des) -> "Engine":
        """Forward the goal frame(s) once and keep their descriptors in the handle (``vitvs_set_goal_dev``): later
        ``compute_velocity(..., I_des=None, ...)`` calls forward only the current frames.  One frame per pair of the later
        calls, or one frame for ``des_shared`` calls.  The reference recomputes the goal every update
        (vitvs_v2.py:482-487); the cache is for servo loops whose goal image does not change, and any call that forwards
        other frames through the engine drops it.  Enqueued on torch's current stream, no synchronisation: a later call on
        that stream runs behind it, a host-pointer call (``compute_velocity_host``, ``reselect_host``) orders itself behind it
        whatever the stream; only a ``_dev`` call on ANOTHER stream is the caller's to order (include/vitvs.h)."""
        des = self._frames(I_des)
        self._check(self.lib.vitvs_set_goal_dev(self.handle, int(des.shape[0]), _ptr(des), _stream_ptr(self.device)), "vitvs_set_goal_dev")
        return self

    def set_goal_depth(self, Z) -> "Engine":
        """The depth image(s) taken at the goal pose, uint16 millimetres [v_max, u_max] or [n, v_max, u_max] (``vitvs_set_goal_depth_dev``
        on the current stream for a device tensor, else ``vitvs_set_goal_depth``): what ``interaction`` "desired" and "mean" read
        Z* from.  One image per pair of the later calls, or one image for all of them.  ``None`` clears it."""
        if Z is None:
            self._check(self.lib.vitvs_set_goal_depth(self.handle, 0, None), "vitvs_set_goal_depth")
            return self
        dev = torch.is_tensor(Z) and Z.is_cuda
        stage = self._stage(not dev)
        z = stage.depth(Z, None, (self.params.v_max, self.params.u_max))
        entry = getattr(self.lib, "vitvs_set_goal_depth_dev" if dev else "vitvs_set_goal_depth")
        rc = entry(self.handle, int(z.shape[0]), stage.ptr(z), *stage.stream)
        if dev:
            z.record_stream(torch.cuda.current_stream(self.device))
        self._check(rc, "vitvs_set_goal_depth")
        return self

    def compute_velocity_dev(self, I_cur: torch.Tensor, I_des: Optional[torch.Tensor], Z: Optional[torch.Tensor],
                             K: torch.Tensor, mode: int = _lib.SELECT_DENSE, selection: Optional[torch.Tensor] = None,
                             n_selected: Optional[torch.Tensor] = None, des_shared: bool = False,
                             out_v: Optional[torch.Tensor] = None, out_status: Optional[torch.Tensor] = None,
                             num_pairs: int = 0):
        """Device-resident call: every argument is a CUDA tensor already laid out as the C ABI
        wants it; work is enqueued on the current stream and nothing synchronises.  ``num_pairs`` = feature pairs of the
        law for this call (0: the engine's default)."""
        n = I_cur.shape[0]
        v = out_v if out_v is not None else torch.empty((n, 6), dtype=torch.float64, device=self.device)
        st = out_status if out_status is not None else torch.empty(n, dtype=torch.int32, device=self.device)
        rc = self.lib.vitvs_compute_velocity_dev(self.handle, n, _ptr(I_cur), _ptr(I_des), int(des_shared), _ptr(Z),
                                                 _ptr(K), mode, _ptr(selection), _ptr(n_selected), int(num_pairs), _ptr(v),
                                                 _ptr(st), _stream_ptr(self.device))
        self._check(rc, "vitvs_compute_velocity_dev")
        self._last_tokens = self.tokens
        return v, st

    def compute_velocity(self, I_cur, I_des, Z, K, mode: int = _lib.SELECT_DENSE, selection=None,
                         des_shared: bool = False, num_pairs: Optional[int] = None):
        """Convenience form: numpy / CPU inputs are moved to the device, then the device path runs.  ``num_pairs``:
        the reference's ``Controller.num_pairs`` for this call (default: the engine's parameters)."""
        return self._velocity(False, I_cur, I_des, Z, K, mode, selection, des_shared, num_pairs)

    def _velocity(self, host, I_cur, I_des, Z, K, mode, selection, des_shared, num_pairs):
        """``compute_velocity`` (``vitvs_compute_velocity_dev``) and ``compute_velocity_host`` (``vitvs_compute_velocity``)."""
        stage = self._stage(host)
        cur = stage.frames(I_cur, None, self.frame_size)
        n = int(cur.shape[0])
        # I_des None: the goal cached by set_goal(); else one frame per pair, or one frame when des_shared
        des = None if I_des is None else stage.frames(I_des, 1 if des_shared else n, self.frame_size)
        z = stage.depth(Z, n, (self.params.v_max, self.params.u_max))
        kk = stage.intrinsics(K, n)
        k = self._num_pairs(num_pairs)
        sel, cnt = stage.selection(mode, selection, n, self.tokens, k)
        v, st, p = stage.f64(n, 6), stage.i32(n), stage.ptr
        entry = "vitvs_compute_velocity" + ("" if host else "_dev")
        rc = getattr(self.lib, entry)(self.handle, n, p(cur), p(des), int(des_shared), p(z), p(kk), mode, p(sel), p(cnt), k, p(v), p(st),
                                      *stage.stream)
        self._check(rc, entry)
        self._last_tokens = self.tokens
        if host:
            self._last_host_pairs = n
        return v, st

    def compute_velocity_host(self, I_cur, I_des, Z, K, mode: int = _lib.SELECT_DENSE, selection=None, n_selected=None,
                              des_shared: bool = False, num_pairs: Optional[int] = None):
        """The host-pointer entry point (``vitvs_compute_velocity``): numpy arrays in — uint8 frames [n, H, W, 3] in the
        engine's current frame geometry, uint16 depth [n, v_max, u_max] (or None), intrinsics [n, 4] or [4], an int32
        selection laid out for ``mode`` — numpy ``(v_c [n, 6] float64, status [n] int32)`` out, ONE synchronous C call: what
        the reference's ``detect_features`` + ``ibvs`` do per update with the arrays its callbacks hold
        (vitvs_v2.py:464-523, 588-632).  No torch tensor is created on this path."""
        return self._velocity(True, I_cur, I_des, Z, K, mode, selection, des_shared, num_pairs)

    def reselect_host(self, mode: int, selection=None, num_pairs: Optional[int] = None):
        """``vitvs_reselect``: the control law again, for another selection, on what the last ``compute_velocity_host`` left in
        the handle (arg-max keys, depth image, intrinsics) — the second half of the reference's update when the draw happens on
        the host between the correspondence and the law (vitvs_v2.py:127-141).  numpy ``(v_c [n, 6], status [n])``."""
        n = self._last_host_pairs
        k = self._num_pairs(num_pairs)
        sel, cnt = _HOST.selection(mode, selection, n, self.tokens, k)
        v, st, p = _HOST.f64(n, 6), _HOST.i32(n), _HOST.ptr
        self._check(self.lib.vitvs_reselect(self.handle, mode, p(sel), p(cnt), k, p(v), p(st)), "vitvs_reselect")
        return v, st

    # ------------------------------------------------------------------ the roll search
    def quarter_turns(self, frames) -> torch.Tensor:
        """``vitvs_quarter_turns_dev``: uint8 frames [n, S, S, 3] (or [S, S, 3]) -> uint8 [n, 4, S, S, 3] on the device, copy k =
        ``numpy.rot90(frame, k)``.  One launch on the current stream."""
        f = self._stage(False).frames(frames, None, (self.cfg.img_size,) * 2)   # at the extractor's input size, whatever set_frame_size says
        out = torch.empty((f.shape[0], 4) + tuple(f.shape[1:]), dtype=torch.uint8, device=self.device)
        rc = self.lib.vitvs_quarter_turns_dev(self.handle, int(f.shape[0]), _ptr(f), _ptr(out), _stream_ptr(self.device))
        self._check(rc, "vitvs_quarter_turns_dev")
        return out

    @staticmethod
    def _roll_info(roll_info, scores) -> dict:
        return dict(roll=int(roll_info[0]), scores=np.array(scores, np.float64), n_mutual=np.array(roll_info[1:5], np.int32),
                    same_image=bool(roll_info[5]))

    def roll_velocity(self, I_cur, I_des, Z, K, mode: int = _lib.SELECT_DENSE, selection=None, num_pairs: Optional[int] = None):
        """``vitvs_roll_velocity_dev``: one servo update of ONE frame pair from any in-plane rotation.  The current
        frame [S, S, 3] is matched against the goal (``I_des`` [S, S, 3], or None: the one goal image cached by ``set_goal``) as its
        four quarter-turned copies in one batch, the best copy wins, its matches are carried back into the unturned frame and the
        law runs on them with ``Z``, ``K`` and the selection as ``compute_velocity`` takes them for one pair.  Needs ``max_pairs >= 4``,
        frames at S x S and ``subpatch`` off.  Returns ``(v_c float64 [6] device tensor, status int32 device scalar, info)``, ``info``
        = dict(``roll``: the winner k (the current frame turned by k quarter turns matched best; -1: no valid candidate),
        ``scores`` float64 [4] (NaN: not valid), ``n_mutual`` int32 [4], ``same_image``: the winner fell under the same-image
        shortcut).  Afterwards ``last_details(1)``, ``pose_velocity`` and ``homography_velocity`` see a one-pair call.  Reading
        ``info`` synchronises; the first call allocates: make it outside a stream capture."""
        return self._roll(False, I_cur, I_des, Z, K, mode, selection, num_pairs)

    def _roll(self, host, I_cur, I_des, Z, K, mode, selection, num_pairs):
        """``roll_velocity`` (``vitvs_roll_velocity_dev``) and ``roll_velocity_host`` (``vitvs_roll_velocity``): one pair."""
        stage, square = self._stage(host), (self.cfg.img_size,) * 2
        cur = stage.frames(I_cur, 1, square)
        des = None if I_des is None else stage.frames(I_des, 1, square)
        z = stage.depth(Z, 1, (self.params.v_max, self.params.u_max))
        kk = stage.intrinsics(K, 1)
        k = self._num_pairs(num_pairs)
        sel, cnt = stage.selection(mode, selection, 1, self.tokens, k)
        v, st, rinfo, scores, p = stage.f64(1, 6), stage.i32(1), stage.i32(8), stage.f64(4), stage.ptr
        entry = "vitvs_roll_velocity" + ("" if host else "_dev")
        rc = getattr(self.lib, entry)(self.handle, p(cur), p(des), p(z), p(kk), mode, p(sel), p(cnt), k, p(v), p(st), p(rinfo), p(scores),
                                      *stage.stream)
        self._check(rc, entry)
        self._last_tokens = self.tokens
        return v[0], st[0], self._roll_info(stage.read(rinfo), stage.read(scores))

    def roll_velocity_host(self, I_cur, I_des, Z, K, mode: int = _lib.SELECT_DENSE, selection=None, num_pairs: Optional[int] = None):
        """``vitvs_roll_velocity``, the host-pointer form of ``roll_velocity``: numpy arrays in, ``(v_c float64 [6], status int,
        info)`` out, one synchronous C call, ordered behind whatever ``_dev`` work the engine still has pending."""
        v, st, info = self._roll(True, I_cur, I_des, Z, K, mode, selection, num_pairs)
        return v, int(st), info

    # ------------------------------------------------------------------ the photometric law
    _PHOTOMETRIC_INTERACTIONS = {"current": 0, "desired": 1, 0: 0, 1: 1}

    def _photometric_scalars(self, level, interaction, mu, lambda_, depth_scale):
        if interaction not in self._PHOTOMETRIC_INTERACTIONS:
            raise VitvsError(f'the photometric law inverts the "current" or the "desired" interaction matrix, got {interaction!r}')
        lam = self.params.lambda_ if lambda_ is None else float(lambda_)
        return int(level), self._PHOTOMETRIC_INTERACTIONS[interaction], float(mu), lam, float(depth_scale)

    @staticmethod
    def _photometric_info(status, normal, pinfo) -> dict:
        n = pinfo[:, 0]
        with np.errstate(divide="ignore", invalid="ignore"):
            cost = np.where(n > 0, normal[:, 27] / np.maximum(n, 1), 0.0)
        return dict(status=status, normal=normal, n=n.copy(), cost=cost, pooled=pinfo[:, 1:3].copy(), bands=pinfo[:, 3].copy(),
                    holes=pinfo[:, 4].copy(), pivot_failed=pinfo[:, 5].astype(bool))

    def photometric_velocity(self, I_cur, I_des, Z, K, level: int = 2, interaction="desired", mu: float = 0.01,
                             lambda_: Optional[float] = None, depth_scale: float = 0.0):
        """``vitvs_photometric_velocity_dev``: the photometric law of ``n`` frame pairs, uint8 ``[n, H, W, 3]`` (or
        ``[H, W, 3]``) at any one geometry up to 4096 x 4096 — camera resolution, not the extractor's input.  ``Z``: uint16
        millimetres ``[n, H, W]`` — the depth of the image the gradients are taken of, the goal's for ``interaction`` "desired", the
        current one for "current" — or None: ``depth_scale`` metres everywhere (RGB only).  ``K``: (fx, fy, cx, cy) at that geometry,
        one for all or ``[n, 4]``.  ``lambda_`` None: the engine's ``params.lambda_``.  No forward runs and no velocity call is needed
        or disturbed.  Two launches on the current stream.  Returns ``(v float64 [n, 6] device tensor, info)``, ``info`` =
        dict(``status`` int32 [n], ``normal`` float64 [n, 28], ``n`` rows, ``cost`` = sum e^2 / n, ``pooled`` [n, 2], ``bands``,
        ``holes``, ``pivot_failed``) as numpy arrays.  Reading ``info`` synchronises; the engine's first call allocates: make it
        outside a stream capture."""
        return self._photometric(False, I_cur, I_des, Z, K, level, interaction, mu, lambda_, depth_scale)

    def _photometric(self, host, I_cur, I_des, Z, K, level, interaction, mu, lambda_, depth_scale):
        """``photometric_velocity`` (``vitvs_photometric_velocity_dev``) and ``photometric_velocity_host`` (``vitvs_photometric_velocity``)."""
        stage = self._stage(host)
        cur = stage.frames(I_cur, None, None)
        n, hh, ww = (int(x) for x in cur.shape[:3])
        des = stage.frames(I_des, n, (hh, ww))
        z = stage.depth(Z, n, (hh, ww))
        kk = stage.intrinsics(K, n)
        level, inter, mu, lam, ds = self._photometric_scalars(level, interaction, mu, lambda_, depth_scale)
        v, st, normal, pinfo, p = stage.f64(n, 6), stage.i32(n), stage.f64(n, 28), stage.i32(n, 8), stage.ptr
        entry = "vitvs_photometric_velocity" + ("" if host else "_dev")
        rc = getattr(self.lib, entry)(self.handle, n, p(cur), p(des), hh, ww, p(z), ds, p(kk), level, inter, mu, lam, p(v), p(st), p(normal),
                                      p(pinfo), *stage.stream)
        self._check(rc, entry)
        return v, self._photometric_info(stage.read(st), stage.read(normal), stage.read(pinfo))

    def photometric_velocity_host(self, I_cur, I_des, Z, K, level: int = 2, interaction="desired", mu: float = 0.01,
                                  lambda_: Optional[float] = None, depth_scale: float = 0.0):
        """``vitvs_photometric_velocity``, the host-pointer form of ``photometric_velocity``: numpy arrays in, ``(v float64 [n, 6],
        info)`` out, one synchronous C call, ordered behind whatever ``_dev`` work the engine still has pending.  Frames of at most
        ``params.v_max`` x ``params.u_max`` pixels."""
        return self._photometric(True, I_cur, I_des, Z, K, level, interaction, mu, lambda_, depth_scale)

    # ------------------------------------------------------------------ the robust photometric law
    @staticmethod
    def _photometric_robust_scalars(illumination, robust_iterations, sigma_min):
        if illumination not in (False, True, 0, 1):
            raise VitvsError(f"illumination is a flag, got {illumination!r}")
        if isinstance(robust_iterations, bool) or int(robust_iterations) != robust_iterations or not 0 <= int(robust_iterations) <= 4:
            raise VitvsError(f"robust_iterations is 0 .. 4, got {robust_iterations!r}")
        if not (math.isfinite(float(sigma_min)) and float(sigma_min) > 0.0):
            raise VitvsError(f"sigma_min is finite and > 0 grey levels, got {sigma_min!r}")
        return int(bool(illumination)), int(robust_iterations), float(sigma_min)

    def photometric_robust_velocity(self, I_cur, I_des, Z, K, level: int = 2, interaction="desired", mu: float = 0.01,
                                    lambda_: Optional[float] = None, depth_scale: float = 0.0, illumination=True,
                                    robust_iterations: int = 4, sigma_min: float = 1.0):
        """``vitvs_photometric_robust_velocity_dev``: the photometric law under a lighting model and Tukey weights.
        The arguments of ``photometric_velocity``, and ``illumination`` (estimate the gain and bias ``I_cur ~ (1 + gamma) I_des +
        beta`` with the twist), ``robust_iterations`` 0 .. 4 re-weightings and ``sigma_min`` > 0, the floor of the residual scale in
        grey levels.  3 ``robust_iterations`` + 2 launches on the current stream.  Returns ``(v float64 [n, 6] device tensor,
        info)``: ``photometric_velocity``'s ``info`` with ``normal`` float64 [n, 45] (``cost`` = sum w e^2 / sum w), and ``gamma``, ``gain``
        (1 + gamma), ``bias``, ``sigma`` (the last scale; 0 without a re-weighting), ``weight`` (the final sum of the weights),
        ``rejected`` (the share of rows at weight 0) and ``reweightings``.  With ``illumination`` off and ``robust_iterations`` 0
        the twist is ``photometric_velocity``'s bit for bit.  Reading ``info`` synchronises; the engine's first call allocates:
        make it outside a stream capture."""
        return self._photometric_robust(False, I_cur, I_des, Z, K, level, interaction, mu, lambda_, depth_scale, illumination,
                                        robust_iterations, sigma_min)

    def _photometric_robust(self, host, I_cur, I_des, Z, K, level, interaction, mu, lambda_, depth_scale, illumination,
                            robust_iterations, sigma_min):
        """``photometric_robust_velocity`` (``vitvs_photometric_robust_velocity_dev``) and ``photometric_robust_velocity_host``
        (``vitvs_photometric_robust_velocity``)."""
        stage = self._stage(host)
        cur = stage.frames(I_cur, None, None)
        n, hh, ww = (int(x) for x in cur.shape[:3])
        des = stage.frames(I_des, n, (hh, ww))
        z = stage.depth(Z, n, (hh, ww))
        kk = stage.intrinsics(K, n)
        illum, iters, smin = self._photometric_robust_scalars(illumination, robust_iterations, sigma_min)
        level, inter, mu, lam, ds = self._photometric_scalars(level, interaction, mu, lambda_, depth_scale)
        v, st, robust, normal, pinfo, p = stage.f64(n, 6), stage.i32(n), stage.f64(n, 4), stage.f64(n, 45), stage.i32(n, 8), stage.ptr
        entry = "vitvs_photometric_robust_velocity" + ("" if host else "_dev")
        rc = getattr(self.lib, entry)(self.handle, n, p(cur), p(des), hh, ww, p(z), ds, p(kk), level, inter, mu, lam, illum, iters, smin,
                                      p(v), p(st), p(robust), p(normal), p(pinfo), *stage.stream)
        self._check(rc, entry)
        return v, self._photometric_robust_info(stage.read(st), stage.read(normal), stage.read(pinfo), stage.read(robust))

    @staticmethod
    def _photometric_robust_info(status, normal, pinfo, robust) -> dict:
        n, weight = pinfo[:, 0], robust[:, 3]
        with np.errstate(divide="ignore", invalid="ignore"):
            cost = np.where(weight > 0, normal[:, 27] / np.where(weight > 0, weight, 1.0), 0.0)
            rejected = np.where(n > 0, pinfo[:, 6] / np.maximum(n, 1), 0.0)
        return dict(status=status, normal=normal, n=n.copy(), cost=cost, pooled=pinfo[:, 1:3].copy(), bands=pinfo[:, 3].copy(),
                    holes=pinfo[:, 4].copy(), pivot_failed=pinfo[:, 5].astype(bool), zero_weight=pinfo[:, 6].copy(),
                    reweightings=pinfo[:, 7].copy(), gamma=robust[:, 0].copy(), gain=1.0 + robust[:, 0], bias=robust[:, 1].copy(), sigma=robust[:, 2].copy(),
                    weight=weight.copy(), rejected=rejected)

    def photometric_robust_velocity_host(self, I_cur, I_des, Z, K, level: int = 2, interaction="desired", mu: float = 0.01,
                                         lambda_: Optional[float] = None, depth_scale: float = 0.0, illumination=True,
                                         robust_iterations: int = 4, sigma_min: float = 1.0):
        """``vitvs_photometric_robust_velocity``, the host-pointer form of ``photometric_robust_velocity``: numpy arrays in, ``(v
        float64 [n, 6], info)`` out, one synchronous C call.  Frames of at most ``params.v_max`` x ``params.u_max`` pixels."""
        return self._photometric_robust(True, I_cur, I_des, Z, K, level, interaction, mu, lambda_, depth_scale, illumination,
                                        robust_iterations, sigma_min)

    # ------------------------------------------------------------------ the tile photometric law
    @staticmethod
    def _photometric_tile_grid(tiles):
        try:
            gy, gx = tiles
        except (TypeError, ValueError):
            raise VitvsError(f"tiles is (tiles_y, tiles_x), got {tiles!r}") from None
        for g in (gy, gx):
            if isinstance(g, bool) or not isinstance(g, (int, np.integer)) or not 1 <= int(g) <= 8:
                raise VitvsError(f"tiles is (tiles_y, tiles_x), each 1 .. 8, got {tiles!r}")
        return int(gy), int(gx)

    def photometric_tile_velocity(self, I_cur, I_des, Z, K, level: int = 2, interaction="desired", mu: float = 0.01,
                                  lambda_: Optional[float] = None, depth_scale: float = 0.0, tiles=(4, 4), robust_iterations: int = 4,
                                  sigma_min: float = 1.0):
        """``vitvs_photometric_tile_velocity_dev``: the robust photometric law with a LOCAL lighting model: one gain
        and bias per tile of a ``tiles`` = (tiles_y, tiles_x) grid (each 1 .. 8, at most the pooled side) over the pooled image, for
        cast shadows, lighting edges and regional exposure.  The lighting model is always on; the other arguments are
        ``photometric_robust_velocity``'s.  A tile whose rows cannot tell gain from bias (flat, empty, all rejected) is dead in that
        pass and adds nothing.  3 ``robust_iterations`` + 2 launches on the current stream.  Returns ``(v float64 [n, 6] device
        tensor, info)``: ``photometric_robust_velocity``'s ``info`` without ``gamma`` / ``gain`` / ``bias``, with ``normal`` float64
        [n, T, 45] per tile, ``weight`` the live tiles' final sum of weights, and ``tile_gain`` (1 + gamma_k; 1 for a dead tile),
        ``tile_bias``, ``tile_weight``, ``tile_live`` (bool), each [n, tiles_y, tiles_x], ``live_tiles`` and ``dead_tiles``.
        A smooth lighting field is not what tiles fit: they only slow that failure.  Reading ``info`` synchronises; the engine's
        first call allocates: make it outside a stream capture."""
        return self._photometric_tile(False, I_cur, I_des, Z, K, level, interaction, mu, lambda_, depth_scale, tiles, robust_iterations,
                                      sigma_min)

    def photometric_tile_velocity_host(self, I_cur, I_des, Z, K, level: int = 2, interaction="desired", mu: float = 0.01,
                                       lambda_: Optional[float] = None, depth_scale: float = 0.0, tiles=(4, 4),
                                       robust_iterations: int = 4, sigma_min: float = 1.0):
        """``vitvs_photometric_tile_velocity``, the host-pointer form of ``photometric_tile_velocity``: numpy arrays in, ``(v float64
        [n, 6], info)`` out, one synchronous C call.  Frames of at most ``params.v_max`` x ``params.u_max`` pixels."""
        return self._photometric_tile(True, I_cur, I_des, Z, K, level, interaction, mu, lambda_, depth_scale, tiles, robust_iterations,
                                      sigma_min)

    def _photometric_tile(self, host, I_cur, I_des, Z, K, level, interaction, mu, lambda_, depth_scale, tiles, robust_iterations,
                          sigma_min):
        stage = self._stage(host)
        cur = stage.frames(I_cur, None, None)
        n, hh, ww = (int(x) for x in cur.shape[:3])
        des = stage.frames(I_des, n, (hh, ww))
        z = stage.depth(Z, n, (hh, ww))
        kk = stage.intrinsics(K, n)
        gy, gx = self._photometric_tile_grid(tiles)
        _, iters, smin = self._photometric_robust_scalars(True, robust_iterations, sigma_min)
        level, inter, mu, lam, ds = self._photometric_scalars(level, interaction, mu, lambda_, depth_scale)
        T = gy * gx
        v, st, robust, ptiles, normal, pinfo, p = (stage.f64(n, 6), stage.i32(n), stage.f64(n, 4), stage.f64(n, T, 4),
                                                   stage.f64(n, T, 45), stage.i32(n, 8), stage.ptr)
        entry = "vitvs_photometric_tile_velocity" + ("" if host else "_dev")
        rc = getattr(self.lib, entry)(self.handle, n, p(cur), p(des), hh, ww, p(z), ds, p(kk), level, inter, mu, lam, gy, gx, iters, smin,
                                      p(v), p(st), p(robust), p(ptiles), p(normal), p(pinfo), *stage.stream)
        self._check(rc, entry)
        return v, self._photometric_tile_info(stage.read(st), stage.read(normal), stage.read(pinfo), stage.read(robust),
                                              stage.read(ptiles), gy, gx)

    @staticmethod
    def _photometric_tile_info(status, normal, pinfo, robust, ptiles, gy, gx) -> dict:
        n, weight = pinfo[:, 0], robust[:, 3]
        t = ptiles.reshape(-1, gy, gx, 4)
        live = t[..., 3] != 0
        c = (normal[:, :, 27] * live.reshape(live.shape[0], -1)).sum(axis=1)      # sum w e^2 over the live tiles
        with np.errstate(divide="ignore", invalid="ignore"):
            cost = np.where(weight > 0, c / np.where(weight > 0, weight, 1.0), 0.0)
            rejected = np.where(n > 0, pinfo[:, 6] / np.maximum(n, 1), 0.0)
        return dict(status=status, normal=normal, n=n.copy(), cost=cost, pooled=pinfo[:, 1:3].copy(), bands=pinfo[:, 3].copy(),
                    holes=pinfo[:, 4].copy(), pivot_failed=pinfo[:, 5].astype(bool), zero_weight=pinfo[:, 6].copy(),
                    reweightings=pinfo[:, 7].copy(), sigma=robust[:, 2].copy(), weight=weight.copy(), rejected=rejected,
                    tile_gain=1.0 + t[..., 0], tile_bias=t[..., 1].copy(), tile_weight=t[..., 2].copy(), tile_live=live,
                    live_tiles=robust[:, 0].astype(np.int64), dead_tiles=robust[:, 1].astype(np.int64))

    # ------------------------------------------------------------------ the surface photometric law
    @staticmethod
    def _photometric_surface_grid(cells):
        try:
            gy, gx = cells
        except (TypeError, ValueError):
            raise VitvsError(f"cells is (cells_y, cells_x), got {cells!r}") from None
        for g in (gy, gx):
            if isinstance(g, bool) or not isinstance(g, (int, np.integer)) or not 1 <= int(g) <= 8:
                raise VitvsError(f"cells is (cells_y, cells_x), each 1 .. 8, got {cells!r}")
        return int(gy), int(gx)

    def photometric_surface_velocity(self, I_cur, I_des, Z, K, level: int = 2, interaction="desired", mu: float = 0.01,
                                     lambda_: Optional[float] = None, depth_scale: float = 0.0, cells=(4, 4), robust_iterations: int = 4,
                                     sigma_min: float = 1.0):
        """``vitvs_photometric_surface_velocity_dev``: the robust photometric law with a SMOOTH lighting model: a
        bilinear spline of gains and biases on the (cells_y + 1) x (cells_x + 1) nodes of a ``cells`` = (cells_y, cells_x) grid (each
        1 .. 8, at most the pooled side) over the pooled image, for a lamp beside the target, vignetting or a window at one side of
        the room.  The lighting model is always on; the other arguments are ``photometric_robust_velocity``'s.  A node unknown the
        rows cannot tell from the ones before it (a flat or empty neighbourhood) is dead in that pass and takes the value 0.
        3 ``robust_iterations`` + 2 launches on the current stream.  Returns ``(v float64 [n, 6] device tensor, info)``:
        ``photometric_robust_velocity``'s ``info`` without ``gamma`` / ``gain`` / ``bias``, with ``normal`` float64 [n, cells, 120]
        per cell, ``weight`` the final sum of weights, ``node_gain`` (1 + gamma_a; 1 for a dead unknown), ``node_bias``, each
        [n, cells_y + 1, cells_x + 1], ``node_live`` (bool, the same shape: gamma_a is live) and ``node_bias_live`` (beta_a is),
        ``live`` and ``dead`` (unknowns).  An edge in the lighting is the tile law's case, not this one's.  Reading ``info`` synchronises; the engine's
        first call allocates: make it outside a stream capture."""
        return self._photometric_surface(False, I_cur, I_des, Z, K, level, interaction, mu, lambda_, depth_scale, cells,
                                         robust_iterations, sigma_min)

    def photometric_surface_velocity_host(self, I_cur, I_des, Z, K, level: int = 2, interaction="desired", mu: float = 0.01,
                                          lambda_: Optional[float] = None, depth_scale: float = 0.0, cells=(4, 4),
                                          robust_iterations: int = 4, sigma_min: float = 1.0):
        """``vitvs_photometric_surface_velocity``, the host-pointer form of ``photometric_surface_velocity``: numpy arrays in,
        ``(v float64 [n, 6], info)`` out, one synchronous C call.  Frames of at most ``params.v_max`` x ``params.u_max`` pixels."""
        return self._photometric_surface(True, I_cur, I_des, Z, K, level, interaction, mu, lambda_, depth_scale, cells,
                                         robust_iterations, sigma_min)

    def _photometric_surface(self, host, I_cur, I_des, Z, K, level, interaction, mu, lambda_, depth_scale, cells, robust_iterations,
                             sigma_min):
        stage = self._stage(host)
        cur = stage.frames(I_cur, None, None)
        n, hh, ww = (int(x) for x in cur.shape[:3])
        des = stage.frames(I_des, n, (hh, ww))
        z = stage.depth(Z, n, (hh, ww))
        kk = stage.intrinsics(K, n)
        gy, gx = self._photometric_surface_grid(cells)
        _, iters, smin = self._photometric_robust_scalars(True, robust_iterations, sigma_min)
        level, inter, mu, lam, ds = self._photometric_scalars(level, interaction, mu, lambda_, depth_scale)
        T, Q = gy * gx, (gy + 1) * (gx + 1)
        v, st, robust, pnodes, sums, pinfo, p = (stage.f64(n, 6), stage.i32(n), stage.f64(n, 4), stage.f64(n, Q, 4),
                                                 stage.f64(n, T, 120), stage.i32(n, 8), stage.ptr)
        entry = "vitvs_photometric_surface_velocity" + ("" if host else "_dev")
        rc = getattr(self.lib, entry)(self.handle, n, p(cur), p(des), hh, ww, p(z), ds, p(kk), level, inter, mu, lam, gy, gx, iters, smin,
                                      p(v), p(st), p(robust), p(pnodes), p(sums), p(pinfo), *stage.stream)
        self._check(rc, entry)
        return v, self._photometric_surface_info(stage.read(st), stage.read(sums), stage.read(pinfo), stage.read(robust),
                                                 stage.read(pnodes), gy, gx)

    @staticmethod
    def _photometric_surface_info(status, normal, pinfo, robust, pnodes, gy, gx) -> dict:
        n, weight = pinfo[:, 0], robust[:, 3]
        q = pnodes.reshape(-1, gy + 1, gx + 1, 4)
        c = normal[:, :, 27].sum(axis=1)                                            # sum w e^2 over the cells
        with np.errstate(divide="ignore", invalid="ignore"):
            cost = np.where(weight > 0, c / np.where(weight > 0, weight, 1.0), 0.0)
            rejected = np.where(n > 0, pinfo[:, 6] / np.maximum(n, 1), 0.0)
        return dict(status=status, normal=normal, n=n.copy(), cost=cost, pooled=pinfo[:, 1:3].copy(), bands=pinfo[:, 3].copy(),
                    holes=pinfo[:, 4].copy(), pivot_failed=pinfo[:, 5].astype(bool), zero_weight=pinfo[:, 6].copy(),
                    reweightings=pinfo[:, 7].copy(), sigma=robust[:, 2].copy(), weight=weight.copy(), rejected=rejected,
                    node_gain=1.0 + q[..., 0], node_bias=q[..., 1].copy(), node_live=q[..., 2] != 0, node_bias_live=q[..., 3] != 0,
                    live=robust[:, 0].astype(np.int64), dead=robust[:, 1].astype(np.int64))

    # ------------------------------------------------------------------ the photometric rig law
    def photometric_rig_velocity(self, I_cur, I_des, Z, K, cVr, live=None, level: int = 2, interaction="desired", mu: float = 0.01,
                                 lambda_: Optional[float] = None, depth_scale: float = 0.0, illumination=True,
                                 robust_iterations: int = 4, sigma_min: float = 1.0):
        """``vitvs_photometric_rig_velocity_dev``: the robust photometric law of the ``n`` cameras of one rigid rig as ONE system
        (DESIGN.md 5m).  The arguments of ``photometric_robust_velocity`` with a camera in the place of a pair, ``cVr`` float64
        ``[n, 6, 6]`` (``servo.twist_matrix`` per camera) and ``live`` (one flag per camera, None: all; a camera at 0 leaves no
        trace).  Every camera has its own gain and bias; the re-weighting takes one median over all cameras' residuals.  4
        ``robust_iterations`` + 2 launches on the current stream.  Returns ``(v_rig float64 [6] device tensor, info)``: ``status``
        (int), ``n`` (rows of the stack), ``cost`` (sum w e^2 / sum w of the stack), ``live``, ``zero_weight``, ``reweightings``,
        ``holes``, ``pivot_failed``, ``pooled``, ``rig_normal`` float64 [28], and per camera ``normal`` float64 [n, 45], ``gamma``,
        ``gain``, ``bias``, ``sigma`` and ``weight`` (the camera's final sum of weights; against its rows it tells the share set
        aside).  Reading ``info`` synchronises; the engine's first call allocates: make it outside a stream capture."""
        return self._photometric_rig(False, I_cur, I_des, Z, K, cVr, live, level, interaction, mu, lambda_, depth_scale, illumination,
                                     robust_iterations, sigma_min)

    def photometric_rig_velocity_host(self, I_cur, I_des, Z, K, cVr, live=None, level: int = 2, interaction="desired",
                                      mu: float = 0.01, lambda_: Optional[float] = None, depth_scale: float = 0.0, illumination=True,
                                      robust_iterations: int = 4, sigma_min: float = 1.0):
        """``vitvs_photometric_rig_velocity``, the host-pointer form of ``photometric_rig_velocity``: numpy arrays in, ``(v_rig
        float64 [6], info)`` out, one synchronous C call.  Frames of at most ``params.v_max`` x ``params.u_max`` pixels."""
        return self._photometric_rig(True, I_cur, I_des, Z, K, cVr, live, level, interaction, mu, lambda_, depth_scale, illumination,
                                     robust_iterations, sigma_min)

    def _photometric_rig(self, host, I_cur, I_des, Z, K, cVr, live, level, interaction, mu, lambda_, depth_scale, illumination,
                         robust_iterations, sigma_min):
        stage = self._stage(host)
        cur = stage.frames(I_cur, None, None)
        n, hh, ww = (int(x) for x in cur.shape[:3])
        des = stage.frames(I_des, n, (hh, ww))
        z = stage.depth(Z, n, (hh, ww))
        kk = stage.intrinsics(K, n, "camera")
        W = stage.array(cVr, "float64")
        if tuple(W.shape) != (n, 6, 6):
            raise VitvsError(f"cVr is one 6 x 6 twist transform per camera, [{n},6,6], got {tuple(W.shape)}")
        W = stage.put(W)
        alive = None
        if live is not None:
            alive = stage.array(np.asarray(live.cpu() if torch.is_tensor(live) else live).astype(bool).astype(np.int32), "int32")
            if tuple(alive.shape) != (n,):
                raise VitvsError(f"live is one flag per camera, [{n}], got {tuple(alive.shape)}")
            alive = stage.put(alive)
        illum, iters, smin = self._photometric_robust_scalars(illumination, robust_iterations, sigma_min)
        level, inter, mu, lam, ds = self._photometric_scalars(level, interaction, mu, lambda_, depth_scale)
        v, st, robust, normal, rig_normal, rinfo, p = (stage.f64(6), stage.i32(1), stage.f64(n, 4), stage.f64(n, 45), stage.f64(28),
                                                       stage.i32(8), stage.ptr)
        entry = "vitvs_photometric_rig_velocity" + ("" if host else "_dev")
        rc = getattr(self.lib, entry)(self.handle, n, p(cur), p(des), hh, ww, p(z), ds, p(kk), p(W), p(alive), level, inter, mu, lam, illum,
                                      iters, smin, p(v), p(st), p(robust), p(normal), p(rig_normal), p(rinfo), *stage.stream)
        self._check(rc, entry)
        return v, self._photometric_rig_info(stage.read(st), stage.read(normal), stage.read(rig_normal), stage.read(rinfo),
                                             stage.read(robust))

    @staticmethod
    def _photometric_rig_info(status, normal, rig_normal, rinfo, robust) -> dict:
        weight = robust[:, 3]
        total = float(weight.sum())
        # (a camera's own rows are not an output: the caller that knows its depth images counts them, servo.MultiController does)
        return dict(status=int(status[0]), n=int(rinfo[1]), cost=float(rig_normal[27] / total) if total > 0 else 0.0, live=int(rinfo[0]),
                    zero_weight=int(rinfo[2]), reweightings=int(rinfo[3]), holes=int(rinfo[4]), pivot_failed=bool(rinfo[5]),
                    pooled=(int(rinfo[6]), int(rinfo[7])), rig_normal=rig_normal, normal=normal, gamma=robust[:, 0].copy(),
                    gain=1.0 + robust[:, 0], bias=robust[:, 1].copy(), sigma=robust[:, 2].copy(), weight=weight.copy())

    def last_tables(self, n_pairs: int = 1) -> dict:
        """``nn_1``, ``nn_2`` (int32) and ``sim_1`` (float32) [n, T] of the last servo call; after ``compute_velocity_host`` they
        come from host memory (the handle's pinned block), no device call."""
        t = getattr(self, "_last_tokens", self.tokens)
        nn1 = np.empty((n_pairs, t), np.int32)
        nn2 = np.empty((n_pairs, t), np.int32)
        sim1 = np.empty((n_pairs, t), np.float32)
        p = _HOST.ptr
        rc = self.lib.vitvs_last_details(self.handle, n_pairs, p(nn1), p(nn2), p(sim1), None, None, None, None, None)
        self._check(rc, "vitvs_last_details")
        return dict(nn_1=nn1, nn_2=nn2, sim_1=sim1)

    def last_features(self, n_pairs: int = 1) -> dict:
        """``info``, ``s_uv`` and ``feat`` of the last servo call — what ``detect_features`` returns is made of
        (vitvs_v2.py:511-553) — without the arg-max tables and ``L_e`` that ``last_details`` also fetches.  After
        ``compute_velocity_host`` they are already in host memory (the handle's pinned block): no device call at all."""
        r = self.max_rows
        info = np.empty((n_pairs, 8), np.int32)
        suv = np.empty((n_pairs, r, 4), np.int32)
        feat = np.empty((n_pairs, r, 4), np.float64)
        p = _HOST.ptr
        rc = self.lib.vitvs_last_details(self.handle, n_pairs, None, None, None, p(info), None, p(suv), p(feat), None)
        self._check(rc, "vitvs_last_details")
        return dict(info=info, s_uv=suv, feat=feat)

    # ------------------------------------------------------------------ the follow-on laws
    @staticmethod
    def _robust_iterations(robust_iterations) -> int:
        N = int(robust_iterations)
        if not 0 <= N <= 16:
            raise ValueError(f"robust_iterations is 0 .. 16, got {robust_iterations!r}")
        return N

    @staticmethod
    def _law_info(fields, counters, per_pair, **arrays):
        """A law's ``info``: ``arrays`` as given, then the counters ``fields`` names: column i of ``counters`` [n, 8] for a law per
        pair, the int ``counters[i]`` for a rig's."""
        info = dict(arrays)
        info.update({name: counters[:, i] if per_pair else int(counters[i]) for i, name in enumerate(fields)})
        return info

    @staticmethod
    def _rig_robust_arguments(n, robust_iterations, K, stage=_HOST):
        """The checks of the robust rig law's extra arguments (no handle needed): float64 [n, 4] intrinsics, or None for N = 0."""
        if Engine._robust_iterations(robust_iterations) == 0:
            return None
        if K is None:
            raise ValueError("robust_iterations > 0 needs K: the cameras' intrinsics (fx, fy, cx, cy), one row per camera or one for all")
        return stage.intrinsics(K, n, "camera", ValueError)

    def rig_velocity(self, cVr, status, robust_iterations: int = 0, K=None):
        """``vitvs_rig_velocity_dev``: the ONE twist of a rigid rig whose cameras were the pairs of the last velocity call, from
        what that call left in the handle.  ``cVr``: float64 [n, 6, 6], camera i's twist transform from the rig frame
        (``servo.twist_matrix``); ``status``: the int32 [n] the velocity call returned (a device tensor stays on the device).
        Returns ``(v_rig float64 tensor [6] on the device, rig_status int, info)`` with ``info`` = dict(cameras, rows, sweeps
        (-1: LDL^T), worst_status, normal float64 [28] device tensor: G upper triangle, g, rows).  Reading the status synchronises.

        ``robust_iterations`` = N > 0: ``vitvs_rig_robust_velocity_dev``, Tukey IRLS over the stacked system with one median over
        all cameras' residuals (valid with option ``robust_law`` on or off); ``K`` (required then) the cameras' intrinsics, [n, 4]
        or one (fx, fy, cx, cy) for all.  ``info`` gains ``reweighted``, ``zero_weights``, ``sigma`` (float) and ``weights``
        (float64 [n, max_rows] device tensor, 0 on padded and unused pairs and on cameras that did not contribute)."""
        v, o, normal, weights, sigma = self._rig(False, cVr, status, robust_iterations, K)
        info = dict(cameras=int(o[1]), rows=int(o[2]), sweeps=int(o[3]), worst_status=int(o[5]), normal=normal)
        if weights is not None:
            info.update(reweighted=int(o[6]), zero_weights=int(o[7]), sigma=float(sigma.cpu()[0]), weights=weights)
        return v, int(o[0]), info

    def _rig(self, host, cVr, status, robust_iterations, K):
        """``rig_velocity`` (``vitvs_rig_velocity_dev``, ``vitvs_rig_robust_velocity_dev``) and ``rig_velocity_host``: ``(v_rig [6],
        rig_status | rig_info [8] on the host, normal [28], weights [n, max_rows] and sigma [1] or None without re-weightings)``."""
        stage = self._stage(host)
        w = stage.array(cVr, "float64").reshape(-1, 36)
        n = int(w.shape[0])
        k = self._rig_robust_arguments(n, robust_iterations, K, stage)   # (before anything touches the device)
        w, st = stage.put(w), stage.status(status)
        if st.shape[0] != n:
            raise VitvsError("one status per camera expected")
        v, normal, p = stage.f64(6), stage.f64(28), stage.ptr
        out = stage.i32(9)                                               # rig_status | rig_info [8]
        weights, sigma, entry = None, None, "vitvs_rig_velocity" + ("" if host else "_dev")
        if k is None:
            rc = getattr(self.lib, entry)(self.handle, n, p(w), p(st), p(v), p(out), p(out[1:]), p(normal), *stage.stream)
        else:
            weights, sigma, entry = stage.f64(n, self.max_rows), stage.f64(1), entry.replace("rig_", "rig_robust_")
            rc = getattr(self.lib, entry)(self.handle, n, p(w), p(st), p(k), int(robust_iterations), p(v), p(out), p(out[1:]), p(normal),
                                          p(weights), p(sigma), *stage.stream)
        self._check(rc, entry)
        return v, stage.read(out), normal, weights, sigma

    def rig_velocity_host(self, cVr, status, robust_iterations: int = 0, K=None):
        """``vitvs_rig_velocity``, the host-pointer form: numpy in, ``(v_rig float64 [6], rig_status, info [8] int32, normal [28])``
        out; with ``robust_iterations`` > 0 (``vitvs_rig_robust_velocity``, ``K`` as ``rig_velocity`` takes it) two more:
        ``weights`` float64 [n, max_rows] and ``sigma``."""
        v, o, normal, weights, sigma = self._rig(True, cVr, status, robust_iterations, K)
        plain = (v, int(o[0]), o[1:], normal)
        return plain if weights is None else plain + (weights, float(sigma[0]))

    def _pair_law(self, entry, host, K, status, scalars, cols):
        """A law per pair of the last velocity call through ``entry`` (host-pointer form) or ``entry + "_dev"``: numpy or device
        tensors ``(v [n, 6], law status [n], the law's own output [n, cols], counters [n, 8], weights [n, max_rows], sigma [n])``."""
        stage = self._stage(host)
        f64, i32, p = stage.f64, stage.i32, stage.ptr
        st = stage.status(status)
        n = int(st.shape[0])
        kk = stage.intrinsics(K, n, "pair", ValueError if host else VitvsError)
        entry += "" if host else "_dev"
        v, own, weights, sigma, lst, counters = f64(n, 6), f64(n, cols), f64(n, self.max_rows), f64(n), i32(n), i32(n, 8)
        rc = getattr(self.lib, entry)(self.handle, n, p(kk), p(st), *scalars, p(v), p(lst), p(own), p(counters), p(weights), p(sigma),
                                      *stage.stream)
        self._check(rc, entry)
        return v, lst, own, counters, weights, sigma

    POSE_INFO_FIELDS = ("usable", "sweeps", "reweighted", "zero_weights", "degenerate", "holes")

    @staticmethod
    def _consensus_arguments(consensus, seed):
        """The checks of a consensus start's arguments (no handle needed)."""
        M, s = int(consensus), int(seed)
        if not 0 <= M <= 4096:
            raise ValueError(f"consensus is 0 .. 4096 hypotheses, got {consensus!r}")
        if not 0 <= s <= 0xFFFFFFFF:
            raise ValueError(f"seed is 0 .. 2^32 - 1, got {seed!r}")
        return M, s

    def _pose_law(self, host, K, status, robust_iterations, consensus=0, seed=0):
        N = self._robust_iterations(robust_iterations)
        M, s = self._consensus_arguments(consensus, seed)
        if M:
            v, pst, pose, pinfo, weights, sigma = self._pair_law("vitvs_pose_consensus_velocity", host, K, status, (N, M, s), 12)
        else:
            v, pst, pose, pinfo, weights, sigma = self._pair_law("vitvs_pose_velocity", host, K, status, (N,), 12)
        return v, self._law_info(self.POSE_INFO_FIELDS, pinfo, True, status=pst, R=pose[:, :9].reshape(len(pst), 3, 3), t=pose[:, 9:],
                                 weights=weights, sigma=sigma, winner=pinfo[:, 6], start_weights=pinfo[:, 7])

    def pose_velocity(self, K, status, robust_iterations: int = 0, consensus: int = 0, seed: int = 0):
        """``vitvs_pose_velocity_dev``: the pose law of every pair of the last velocity call, from what that call left
        in the handle and the goal depth (``set_goal_depth``): one rigid alignment (R, t) of the matched 3-D points per pair,
        X_goal = R X_cam + t, and ``v_pose = -lambda (R^T t, theta u)``.  ``K``: the intrinsics of that call, [n, 4] or one (fx, fy, cx,
        cy) for all; ``status``: the int32 [n] it returned (a device tensor stays on the device); ``robust_iterations``: Tukey
        re-weightings, 0 .. 16.  Returns ``(v_pose float64 [n, 6] device tensor, info)``, ``info`` = dict of device tensors: ``status``
        int32 [n], ``R`` [n, 3, 3], ``t`` [n, 3], ``usable`` / ``sweeps`` / ``reweighted`` / ``zero_weights`` / ``degenerate`` /
        ``holes`` int32 [n], ``weights`` float64 [n, max_rows], ``sigma`` float64 [n].  ``consensus`` > 0
        (``vitvs_pose_consensus_velocity_dev``): that many three-point hypotheses (0 .. 4096) drawn from ``seed`` are scored in front
        of the alignment and the law starts from the rows that agree with the best one; ``info`` then also says which won (``winner``
        int32 [n], j + 1, 0 without a consensus start) and how many rows started at weight 1 (``start_weights`` int32 [n]), and
        ``zero_weights`` counts the rows it left out.  With more than half of the matches wrong use ``robust_iterations`` = 0 behind
        it: the re-weightings' scale is a median over all rows.  One launch on the current stream either way; nothing synchronises
        after the first call (which allocates: make it outside a stream capture)."""
        return self._pose_law(False, K, status, robust_iterations, consensus, seed)

    def pose_velocity_host(self, K, status, robust_iterations: int = 0, consensus: int = 0, seed: int = 0):
        """``vitvs_pose_velocity`` (``vitvs_pose_consensus_velocity`` with ``consensus`` > 0), the host-pointer form: numpy in,
        ``(v_pose float64 [n, 6], info)`` out, ``info`` as ``pose_velocity``'s with numpy arrays.  Synchronous."""
        return self._pose_law(True, K, status, robust_iterations, consensus, seed)

    HOMOGRAPHY_INFO_FIELDS = ("usable", "sweeps", "reweighted", "zero_weights", "degenerate", "behind")

    @staticmethod
    def _homography_arguments(depth_scale, robust_iterations, consensus=0, seed=0):
        """The checks of the homography law's arguments (no handle needed)."""
        N = Engine._robust_iterations(robust_iterations)
        z = float(depth_scale)
        if not (z > 0.0 and math.isfinite(z)):
            raise ValueError(f"depth_scale is a positive, finite length in metres, got {depth_scale!r}")
        M, s = Engine._consensus_arguments(consensus, seed)
        return z, N, M, s

    def _homography_law(self, host, K, status, depth_scale, robust_iterations, consensus=0, seed=0):
        z, N, M, s = self._homography_arguments(depth_scale, robust_iterations, consensus, seed)
        if M:
            v, hst, H, hinfo, weights, sigma = self._pair_law("vitvs_homography_consensus_velocity", host, K, status, (z, N, M, s), 9)
        else:
            v, hst, H, hinfo, weights, sigma = self._pair_law("vitvs_homography_velocity", host, K, status, (z, N), 9)
        return v, self._law_info(self.HOMOGRAPHY_INFO_FIELDS, hinfo, True, status=hst, H=H.reshape(len(hst), 3, 3), weights=weights,
                                 sigma=sigma, winner=hinfo[:, 6], start_weights=hinfo[:, 7])

    def homography_velocity(self, K, status, depth_scale: float = 1.0, robust_iterations: int = 0, consensus: int = 0, seed: int = 0):
        """``vitvs_homography_velocity_dev``: the homography law of every pair of the last velocity call, from the
        matched image points that call left in the handle and nothing else: no depth image, no goal depth.  Per pair the 3 x 3
        homography ``H`` of a planar target, m* ~ H m, and ``v_h = -lambda (depth_scale (H - I) m_c, (H21 - H12, H02 - H20, H10 -
        H01))``.  ``K``: the intrinsics of that call, [n, 4] or one (fx, fy, cx, cy) for all; ``status``: the int32 [n] it returned
        (a device tensor stays on the device; NO_DEPTH does not stop this law); ``depth_scale``: a rough guess of the distance to the
        target in metres, which scales the translational gain only; ``robust_iterations``: Tukey re-weightings, 0 .. 16.  Returns
        ``(v_h float64 [n, 6] device tensor, info)``, ``info`` = dict of device tensors: ``status`` int32 [n], ``H`` [n, 3, 3],
        ``usable`` / ``sweeps`` / ``reweighted`` / ``zero_weights`` / ``degenerate`` / ``behind`` int32 [n], ``weights`` float64
        [n, max_rows], ``sigma`` float64 [n].  ``consensus`` > 0 (``vitvs_homography_consensus_velocity_dev``): that many four-point
        hypotheses (0 .. 4096) drawn from ``seed`` are scored in front of the solve and the law starts from the rows that agree with
        the best one; ``info`` then also says which won (``winner`` int32 [n], j + 1, 0 without a consensus start) and how many rows
        started at weight 1 (``start_weights`` int32 [n]), and ``zero_weights`` counts the rows it left out.  One launch on the
        current stream either way; nothing synchronises after the first call (which allocates: make it outside a stream capture)."""
        return self._homography_law(False, K, status, depth_scale, robust_iterations, consensus, seed)

    def homography_velocity_host(self, K, status, depth_scale: float = 1.0, robust_iterations: int = 0, consensus: int = 0,
                                 seed: int = 0):
        """``vitvs_homography_velocity`` (``vitvs_homography_consensus_velocity`` with ``consensus`` > 0), the host-pointer form:
        numpy in, ``(v_h float64 [n, 6], info)`` out, ``info`` as ``homography_velocity``'s with numpy arrays.  Synchronous."""
        return self._homography_law(True, K, status, depth_scale, robust_iterations, consensus, seed)

    POSE_RIG_INFO_FIELDS = ("cameras", "usable", "sweeps", "reweighted", "zero_weights", "degenerate", "holes", "worst_status")

    @staticmethod
    def _pose_rig_arguments(rig, status, robust_iterations):
        """The checks of the pose rig law's arguments (no handle needed): float64 rTc [n, 12] and N."""
        N = Engine._robust_iterations(robust_iterations)
        n = len(rig)
        if n < 1:
            raise ValueError("rig is a sequence of (R_i, t_i), one per camera of the last velocity call")
        rtc = np.zeros((n, 12))
        for i, (R, t) in enumerate(rig):
            R, t = np.asarray(R, np.float64), np.asarray(t, np.float64)
            if R.size != 9 or t.size != 3:
                raise ValueError("rig is a sequence of (R_i [3, 3], t_i [3])")
            rtc[i, :9], rtc[i, 9:] = R.reshape(9), t.reshape(3)
        if int(status.numel() if torch.is_tensor(status) else np.asarray(status).size) != n:
            raise ValueError("one status per camera of the rig expected")
        return rtc, N

    def _pose_rig_law(self, host, rig, K, status, robust_iterations):
        stage = self._stage(host)
        f64, p = stage.f64, stage.ptr
        rtc, N = self._pose_rig_arguments(rig, status, robust_iterations)            # (before anything touches the device)
        n, entry = int(rtc.shape[0]), "vitvs_pose_rig_velocity" + ("" if host else "_dev")
        k = stage.intrinsics(K, n, "camera", ValueError)
        rtc, st = stage.put(stage.array(rtc)), stage.status(status)
        v, pose, moments, weights, sigma = f64(6), f64(12), f64(18), f64(n, self.max_rows), f64(1)
        out = stage.i32(9)                                               # rig_status | rig_info [8]
        rc = getattr(self.lib, entry)(self.handle, n, p(rtc), p(k), p(st), N, p(v), p(out), p(pose), p(out[1:]), p(moments),
                                      p(weights), p(sigma), *stage.stream)
        self._check(rc, entry)
        o = stage.read(out)
        return v, int(o[0]), self._law_info(self.POSE_RIG_INFO_FIELDS, o[1:], False, R=pose[:9].reshape(3, 3), t=pose[9:],
                                            moments=moments, weights=weights, sigma=float(sigma[0]) if host else sigma)

    def pose_rig_velocity(self, rig, K, status, robust_iterations: int = 0):
        """``vitvs_pose_rig_velocity_dev``: the pose rig law of a rigid rig whose cameras were the pairs of the last
        velocity call: ONE rigid alignment (R, t) of the matched 3-D points of all cameras in the rig frame, and ``v_rig = -lambda
        (R^T t, theta u)`` in the rig's own frame.  ``rig``: a sequence of (R_i, t_i), camera i's pose in the rig frame (what
        ``MultiController(rig=...)`` takes); ``K``: the intrinsics of that call, [n, 4] or one (fx, fy, cx, cy) for all; ``status``:
        the int32 [n] it returned (a device tensor stays on the device); ``robust_iterations``: Tukey re-weightings with one median
        over all cameras' residuals, 0 .. 16.  Returns ``(v_rig float64 [6] device tensor, rig_status int, info)``, ``info`` = dict
        (cameras, usable, sweeps, reweighted, zero_weights, degenerate, holes, worst_status as ints; R [3, 3], t [3], moments [18],
        weights [n, max_rows], sigma [1] as device tensors).  One launch on the current stream; reading the status synchronises.
        The first call allocates: make it outside a stream capture."""
        return self._pose_rig_law(False, rig, K, status, robust_iterations)

    def pose_rig_velocity_host(self, rig, K, status, robust_iterations: int = 0):
        """``vitvs_pose_rig_velocity``, the host-pointer form: numpy in, ``(v_rig float64 [6], rig_status, info)`` out, ``info`` as
        ``pose_rig_velocity``'s with numpy arrays (``sigma`` a float).  Synchronous."""
        return self._pose_rig_law(True, rig, K, status, robust_iterations)

    # ------------------------------------------------------------------ options
    def set_option(self, name: str, value: int) -> "Engine":
        """Per-handle options of include/vitvs.h: ``graph_replay`` (0 / 1), ``in_flight`` (updates run beside this handle's),
        ``robust_law`` (0: the plain control law; 1 .. 16: Tukey re-weightings), ``subpatch`` (0: patch centres; 1: matches
        refined by their sub-patch offsets), ``interaction`` (0: L(s, Z); 1: L(s*, Z*); 2: their mean), ``select_cells`` (1 .. 16:
        image cells per side of ``SELECT_BEST``)."""
        self._check(self.lib.vitvs_set_option(self.handle, name.encode(), int(value)), f"vitvs_set_option({name})")
        return self

    def apply_law_params(self, params: ServoParams) -> "Engine":
        """The control law of ``params`` (``robust_iterations``, ``subpatch``, ``interaction``, and ``select_cells`` of the selection
        in front of it): sets the options that differ from this engine's and keeps ``self.params`` in step."""
        for field, option, value in (("robust_iterations", "robust_law", params.robust_iterations),
                                     ("subpatch", "subpatch", int(params.subpatch)),
                                     ("interaction", "interaction", INTERACTIONS.index(params.interaction)),
                                     ("select_cells", "select_cells", int(params.select_cells))):
            if getattr(params, field) != getattr(self.params, field):
                self.set_option(option, value)
                self.params = self.params.replace(**{field: getattr(params, field)})
        return self

    # ------------------------------------------------------------------ measurement hooks
    def timing_enable(self, on: bool = True):
        self._check(self.lib.vitvs_timing_enable(self.handle, int(on)), "vitvs_timing_enable")

    def timing_collect(self) -> dict:
        """{kernel class: (total ms between its HIP event pairs, launches)} since the last collect."""
        n = self.lib.vitvs_timing_classes()
        ms = (C.c_double * n)()
        cnt = (C.c_int32 * n)()
        self._check(self.lib.vitvs_timing_collect(self.handle, n, ms, cnt), "vitvs_timing_collect")
        return {self.lib.vitvs_timing_class_name(i).decode(): (float(ms[i]), int(cnt[i])) for i in range(n)}

    def last_details(self, n_pairs: int = 1) -> dict:
        """Host copies of what the last servo call left on the device (synchronises)."""
        t, r = getattr(self, "_last_tokens", self.tokens), self.max_rows
        nn1 = np.empty((n_pairs, t), np.int32)
        nn2 = np.empty((n_pairs, t), np.int32)
        sim1 = np.empty((n_pairs, t), np.float32)
        info = np.empty((n_pairs, 8), np.int32)
        sel = np.empty((n_pairs, r), np.int32)
        suv = np.empty((n_pairs, r, 4), np.int32)
        feat = np.empty((n_pairs, r, 4), np.float64)
        L = np.empty((n_pairs, 7, 2 * r), np.float64)
        p = _HOST.ptr
        rc = self.lib.vitvs_last_details(self.handle, n_pairs, p(nn1), p(nn2), p(sim1), p(info), p(sel), p(suv),
                                         p(feat), p(L))
        self._check(rc, "vitvs_last_details")
        return dict(nn_1=nn1, nn_2=nn2, sim_1=sim1, info=info, selected=sel, s_uv=suv, feat=feat, L=L,
                    weights=self.last_weights(n_pairs), offsets=self.last_offsets(n_pairs), Z_goal=self.last_goal_depth(n_pairs))

    def last_goal_depth(self, n_pairs: int = 1) -> np.ndarray:
        """``vitvs_last_goal_depth``: float64 [n, max_rows], Z* in metres of every feature row in the last law evaluation (all 0
        with ``interaction`` "current", and on unused rows).  Synchronises."""
        z = np.empty((n_pairs, self.max_rows), np.float64)
        self._check(self.lib.vitvs_last_goal_depth(self.handle, n_pairs, _HOST.ptr(z)), "vitvs_last_goal_depth")
        return z

    def last_order(self, n_pairs: int = 1) -> np.ndarray:
        """``vitvs_last_order``: int32 [n, T], the visiting order the last law evaluation ran on when its mode was ``SELECT_BEST``
        (an error after any other mode).  Synchronises."""
        order = np.empty((n_pairs, getattr(self, "_last_tokens", self.tokens)), np.int32)
        self._check(self.lib.vitvs_last_order(self.handle, n_pairs, _HOST.ptr(order)), "vitvs_last_order")
        return order

    def last_offsets(self, n_pairs: int = 1) -> np.ndarray:
        """``vitvs_last_offsets``: float32 [n, max_rows, 2], the sub-patch offsets (dr, dc) of every feature row's match in the
        last law evaluation (all 0 with ``subpatch`` off, on zero-padded and unused rows).  Synchronises."""
        off = np.empty((n_pairs, self.max_rows, 2), np.float32)
        self._check(self.lib.vitvs_last_offsets(self.handle, n_pairs, _HOST.ptr(off)), "vitvs_last_offsets")
        return off

    def last_weights(self, n_pairs: int = 1) -> np.ndarray:
        """``vitvs_last_weights``: float64 [n, max_rows], the weight of every feature pair in the last law evaluation's final
        solve (all 1 on live pairs with ``robust_law`` off; 0 on zero-padded and unused rows).  Synchronises."""
        w = np.empty((n_pairs, self.max_rows), np.float64)
        self._check(self.lib.vitvs_last_weights(self.handle, n_pairs, _HOST.ptr(w)), "vitvs_last_weights")
        return w
