"""Host side of the MI355X render path: drives libcoponerf_hip.so kernel by kernel.

Mirrors the body of the reference's CoPoNeRF.forward (/root/reference models/CoPoNeRF.py:208-576):
pose algebra (4x4, on the host) -> K1 ray projection -> K1b per-sample geometry -> K2 gathers ->
K3 per-sample GEMMs -> K4 two rounds of joint-softmax attention -> K5 light-field decoder -> masking.
PyTorch is used for device memory, the current HIP stream and a handful of O(B) 4x4 operations only.
"""
from __future__ import annotations

import ctypes
import math
import os
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _hip, render_f32
from ._hip import call

V = 2  # context views; the kernels are specialised for stereo pairs like the reference's released model


def _ptr(t: Optional[torch.Tensor]) -> int:
    return 0 if t is None else t.data_ptr()


def _stream() -> int:
    return _hip.stream_handle()


def _flat_on_device(mats: Sequence[Optional[torch.Tensor]]) -> Optional[torch.Tensor]:
    """The live tensors of `mats` as ONE float32 device vector (None when all of them are on the host already)."""
    live = [m for m in mats if m is not None]
    if not live or all(m.device.type == "cpu" for m in live):
        return None
    dev = next(m.device for m in live if m.device.type != "cpu")
    return torch.cat([m.detach().float().to(dev).reshape(-1) for m in live])


def _split_host(mats: Sequence[Optional[torch.Tensor]], flat: torch.Tensor) -> List[Optional[torch.Tensor]]:
    out, off = [], 0
    for m in mats:
        if m is None:
            out.append(None)
            continue
        out.append(flat[off:off + m.numel()].view(m.shape).clone())
        off += m.numel()
    return out


def _to_host(*mats: Optional[torch.Tensor]) -> List[Optional[torch.Tensor]]:
    """float32 CPU copies of a few small device tensors with ONE device->host transfer (each .cpu() is a host sync)."""
    flat = _flat_on_device(mats)
    if flat is None:
        return [None if m is None else m.detach().float() for m in mats]
    return _split_host(mats, flat.cpu())


# ----------------------------------------------------------------------------------------------
# (a1) pose algebra on the host — O(B) 4x4 matrices, float32, LAPACK: deterministic and identical to
# what the CPU oracle computes, so everything downstream can be compared bit for bit.
# ----------------------------------------------------------------------------------------------
def _upload(host: Dict[str, torch.Tensor], dev) -> Dict[str, torch.Tensor]:
    """Small CPU float32 tensors -> device views of ONE pinned staging buffer, one asynchronous H2D copy."""
    total = sum(t.numel() for t in host.values())
    stage = torch.empty(total, dtype=torch.float32, pin_memory=(dev.type == "cuda"))
    off = 0
    for t in host.values():
        stage[off:off + t.numel()] = t.reshape(-1)
        off += t.numel()
    flat = stage.to(dev, non_blocking=True)
    out, off = {"_flat": flat}, 0
    for k, t in host.items():
        out[k] = flat[off:off + t.numel()].view(t.shape)
        off += t.numel()
    return out


def host_pose_products(ctx_c2w: torch.Tensor, qry_c2w: torch.Tensor, qry_K: torch.Tensor) -> Dict[str, torch.Tensor]:
    """O(B) 4x4 / 3x3 inverses the outputs need (CoPoNeRF.py:568-574 gt_rel_pose*, utils.py:140-170 and
    geometry.py:395-406 for the auxiliary reprojections), on the HOST next to the rest of the pose algebra: a GPU
    `torch.inverse` checks its LAPACK status on the host, i.e. every one of them is a full stream synchronisation at the
    END of a render pass (5 per call in round 1: the host could not run ahead of the GPU at all)."""
    return {"gt_rel_pose": torch.inverse(ctx_c2w[:, 0]) @ ctx_c2w[:, 1],
            "gt_rel_pose_flip": torch.inverse(torch.inverse(ctx_c2w[:, -1]) @ ctx_c2w[:, 0]),
            "inv_Kq": torch.inverse(qry_K[:, 0, :3, :3]), "inv_qc2w": torch.inverse(qry_c2w[:, 0])}


def build_ray_constants(prods: Dict[str, torch.Tensor], ctx_K: torch.Tensor, Tq: torch.Tensor) -> torch.Tensor:
    """(B, RAYC_STRIDE) float32 block of cpn_ray_outputs (include/coponerf_hip.h): what the per-ray auxiliary outputs
    need of the O(B) pose algebra (CoPoNeRF.py:508-521)."""
    B = ctx_K.shape[0]
    c = torch.zeros(B, _hip.RAYC_STRIDE, dtype=torch.float32)
    c[:, 0:4] = prods["inv_qc2w"][:, 2, :]
    c[:, 4:13] = prods["inv_Kq"].reshape(B, 9)
    c[:, 13:22] = ctx_K[:, 0, :3, :3].reshape(B, 9)
    c[:, 22:31] = ctx_K[:, 1, :3, :3].reshape(B, 9)
    c[:, 31:47] = Tq[:, 0].reshape(B, 16)
    c[:, 47:63] = Tq[:, 1].reshape(B, 16)
    return c


def _uv_rows(uv: torch.Tensor, B: int, R: int) -> Tuple[torch.Tensor, int]:
    """Query pixels (B,1,R,2) -> (float32 tensor whose storage the kernels read, batch stride in floats).  A ray chunk of
    a larger array (torch.chunk(uv_full, 18, dim=2), /root/reference test.py:177) is read in place through its stride."""
    u = uv.detach()
    if u.dtype != torch.float32:
        u = u.float()
    u = u.view(B, R, 2) if u.dim() == 4 and u.shape[1] == 1 and u.stride(3) == 1 and u.stride(2) == 2 else u.reshape(B, R, 2).contiguous()
    if u.stride(2) != 1 or u.stride(1) != 2 or (B > 1 and u.stride(0) < 2 * R):
        u = u.contiguous()
    return u, (u.stride(0) if B > 1 else 2 * R)


def _rigid_inverse(m: torch.Tensor) -> torch.Tensor:
    out = torch.zeros_like(m)
    rt = m[..., :3, :3].transpose(-1, -2)
    out[..., :3, :3] = rt
    out[..., :3, 3] = (-(rt @ m[..., :3, 3:]))[..., 0]
    out[..., 3, 3] = 1
    return out


def build_camera_block(ctx_c2w: torch.Tensor, ctx_K: torch.Tensor, qry_c2w: torch.Tensor, qry_K: torch.Tensor,
                       rel_pose: Optional[torch.Tensor], val: bool, H: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """CPU tensors in, (cam (B*V, CAM_STRIDE) float32 CPU, Tq (B,V,4,4) CPU) out.

    CoPoNeRF.py:239-244 (query pose in each context frame), :325-332 (context-to-context poses),
    :259-261 (normalised intrinsics: rows 0,1 divided by H)."""
    B = ctx_c2w.shape[0]
    inv_ctx = torch.inverse(ctx_c2w)
    M = inv_ctx @ ctx_c2w
    if val:
        q0 = inv_ctx[:, 0].unsqueeze(1) @ qry_c2w
        q1 = _rigid_inverse(rel_pose).unsqueeze(1) @ q0
        Tq = torch.cat((q0, q1), dim=1)
        A1 = torch.cat((torch.inverse(ctx_c2w[:, 0:1]) @ ctx_c2w[:, 0].unsqueeze(1), rel_pose.unsqueeze(1)), dim=1)
        A2 = torch.cat((_rigid_inverse(rel_pose).unsqueeze(1),
                        torch.inverse(ctx_c2w[:, 1:2]) @ ctx_c2w[:, -1].unsqueeze(1)), dim=1)
    else:
        Tq = inv_ctx @ qry_c2w
        A1 = torch.inverse(ctx_c2w[:, 0:1]) @ ctx_c2w
        A2 = torch.inverse(ctx_c2w[:, 1:2]) @ ctx_c2w
    Kn = ctx_K[:, :, :3, :3].clone()
    Kn[:, :, :2, :] = Kn[:, :, :2, :] / H
    cam = torch.zeros(B, V, _hip.CAM_STRIDE, dtype=torch.float32)
    cam[:, :, _hip.CAM_TQ:_hip.CAM_TQ + 16] = Tq.reshape(B, V, 16)
    cam[:, :, _hip.CAM_M:_hip.CAM_M + 16] = M.reshape(B, V, 16)
    # own-frame / other-frame transforms of each view's points: view 0 -> (A1[0], A2[0]), view 1 -> (A2[1], A1[1])
    cam[:, 0, _hip.CAM_AOWN:_hip.CAM_AOWN + 16] = A1[:, 0].reshape(B, 16)
    cam[:, 0, _hip.CAM_AOTH:_hip.CAM_AOTH + 16] = A2[:, 0].reshape(B, 16)
    cam[:, 1, _hip.CAM_AOWN:_hip.CAM_AOWN + 16] = A2[:, 1].reshape(B, 16)
    cam[:, 1, _hip.CAM_AOTH:_hip.CAM_AOTH + 16] = A1[:, 1].reshape(B, 16)

    def k4(K):  # fx fy cx cy
        return torch.stack((K[..., 0, 0], K[..., 1, 1], K[..., 0, 2], K[..., 1, 2]), -1)

    cam[:, :, _hip.CAM_KQ:_hip.CAM_KQ + 4] = k4(qry_K[:, 0])[:, None, :]
    kc = k4(ctx_K)
    cam[:, :, _hip.CAM_KC:_hip.CAM_KC + 4] = kc
    cam[:, 0, _hip.CAM_KO:_hip.CAM_KO + 4] = kc[:, 1]
    cam[:, 1, _hip.CAM_KO:_hip.CAM_KO + 4] = kc[:, 0]
    cam[:, :, _hip.CAM_KN:_hip.CAM_KN + 9] = Kn.reshape(B, V, 9)
    return cam.reshape(B * V, _hip.CAM_STRIDE), Tq


# ----------------------------------------------------------------------------------------------
def frag_order_f32(m: torch.Tensor) -> torch.Tensor:
    """(N, K) fp32 row-major -> MFMA fragment order of v_mfma_f32_16x16x4_f32 as cpn_lightfield_decode reads it
    (include/coponerf_hip.h): [N/16][K/16][lane = row + 16 * k group][4] - lane l of fragment (t, kb) holds
    m[16 t + (l & 15)][16 kb + 4 (l >> 4) .. +4], so a wave's load of one fragment is 1 KiB of contiguous memory."""
    n, k = m.shape
    return m.reshape(n // 16, 16, k // 16, 4, 4).permute(0, 2, 3, 1, 4).contiguous()


def pack_key_ring(wk: torch.Tensor) -> torch.Tensor:
    """The folded key matrix (128, 2 * 832) fp16 in the order cpn_encode_key streams it through its LDS ring:
    [image j][slice n][tile t][k step][lane = row + 16 * 8-column group][8] - piece (t, k) of slice step (j, n) holds, in lane
    (a, g), wk[16 t + a][832 j + 64 n + 32 k + 8 g .. +8]: every 1 KiB DMA piece contiguous."""
    return wk.reshape(8, 16, 2, 13, 2, 4, 8).permute(2, 3, 0, 4, 5, 1, 6).contiguous()


def unit_rows(B: int, R: int, S: int, ray0: int, nrays: int, device=None) -> torch.Tensor:
    """(units * 16,) int64: for every row slot of a UNIT-order matrix of a launch over rays [ray0, ray0 + nrays) (include/
    coponerf_hip.h, cpn_encode_key kh_units / cpn_local_units) the row of the row-order matrix it holds - ((ray - ray0) * V + v) * S
    + s - or -1 for the dead rows of partial units.  Unit u = ((ray group - first group) * V + v) * ceil(S/4) + sample block, row
    slot c = (sample & 3) * 4 + (ray & 3)."""
    gpb, nsblk = (R + 3) // 4, (S + 3) // 4
    b_lo, b_hi = ray0 // R, (ray0 + nrays - 1) // R
    g0 = b_lo * gpb + (ray0 - b_lo * R) // 4
    g1 = b_hi * gpb + (ray0 + nrays - 1 - b_hi * R) // 4
    gq = torch.arange(g0, g1 + 1, device=device).view(-1, 1, 1, 1)
    v = torch.arange(V, device=device).view(1, -1, 1, 1)
    sblk = torch.arange(nsblk, device=device).view(1, 1, -1, 1)
    c = torch.arange(16, device=device).view(1, 1, 1, -1)
    b, rg = gq // gpb, gq % gpb
    r, s = rg * 4 + (c & 3), sblk * 4 + (c >> 2)
    ray = b * R + r
    live = (r < R) & (s < S) & (ray >= ray0) & (ray < ray0 + nrays)
    row = ((ray - ray0) * V + v) * S + s
    return torch.where(live, row, torch.full_like(row, -1)).reshape(-1)


def rows_from_unit_order(x: torch.Tensor, B: int, R: int, S: int, ray0: int, nrays: int) -> torch.Tensor:
    """A (rows, 128) fp16 matrix stored in unit order -> row-major (nrays * V * S, 128)."""
    idx = unit_rows(B, R, S, ray0, nrays, x.device)
    units = idx.numel() // 16
    t = x.reshape(-1)[:units * 16 * 128].reshape(units, 4, 4, 16, 8).permute(0, 3, 1, 2, 4).reshape(units * 16, 128)   # [unit][p][fg][c][8]
    out = torch.zeros(nrays * V * S, 128, dtype=x.dtype, device=x.device)
    keep = idx >= 0
    out[idx[keep]] = t[keep]
    return out


def _flat_tensors(obj):
    if isinstance(obj, torch.Tensor):
        yield obj
    elif isinstance(obj, (list, tuple)):
        for o in obj:
            yield from _flat_tensors(o)
    elif isinstance(obj, dict):
        for o in obj.values():
            yield from _flat_tensors(o)


class PendingHostTensor(torch.Tensor):
    """The caller contract's `pixel_val` (a CPU tensor, /root/reference models/CoPoNeRF.py:490) while its asynchronous
    device->host copy may still be running on the copy stream.  The reference's `.cpu()` blocks the host once per
    forward() call — 18 times per image in its own evaluation loop (test.py:176-190).  This subclass defers that wait to
    the first operation that touches the VALUES (any torch function, `.numpy()`, `torch.cat`, indexing ...): it
    synchronises on the copy's event there and then behaves as the plain pinned CPU tensor it wraps.  Metadata
    (`shape`, `device`, `dtype`, `size()`, `dim()`) and `.cpu()` on this already-CPU tensor do not wait.
    `RenderEngine.lazy_pixel_val = False` (or COPONERF_EAGER_PIXEL_VAL=1) hands out a plain tensor after the wait."""

    _NO_WAIT = frozenset(("shape", "device", "dtype", "size", "dim", "numel", "ndim", "is_cuda", "is_pinned", "stride",
                          "is_contiguous", "element_size", "nelement", "ndimension", "layout", "requires_grad", "is_cpu",
                          "names", "is_sparse", "is_quantized", "is_meta", "grad_fn", "grad", "is_leaf", "is_complex",
                          "is_floating_point", "__len__"))

    @staticmethod
    def wrap(host: torch.Tensor, ready, src: Optional[torch.Tensor] = None) -> "PendingHostTensor":
        """`ready`: anything with .synchronize() (the copy's event); `src`: the device tensor being copied, kept alive
        until the copy has been waited for (its block is also record_stream'ed for the copy stream by the engine)."""
        t = torch.Tensor._make_subclass(PendingHostTensor, host)
        t._cpn_ready = ready
        t._cpn_src = src
        return t

    @staticmethod
    def _cat_as_copies_arrive(tensors, dim=0, out=None, **other):
        """`torch.cat` of the callers' join (test.py:207: the per-chunk pixel_val along dim -3), chunk by chunk: each
        piece is copied into the result as soon as ITS device->host copy has landed, so the 67 MB host concatenation of a
        256x256x64 image runs under the GPU work of the later chunks instead of after the last one.  Same result as
        torch.cat; anything but a plain list of same-dtype PendingHostTensors falls back to it (returns None)."""
        if "axis" in other and len(other) == 1 and dim == 0:      # numpy-style spelling torch.cat also accepts
            dim, other = other["axis"], {}
        if other or out is not None or not isinstance(tensors, (list, tuple)) or len(tensors) < 2 or not all(
                isinstance(t, PendingHostTensor) and t.dtype == tensors[0].dtype and t.dim() == tensors[0].dim()
                for t in tensors):
            return None
        nd = tensors[0].dim()
        d = dim + nd if dim < 0 else dim
        if not 0 <= d < nd:
            return None
        with torch._C.DisableTorchFunctionSubclass():
            shape = list(tensors[0].shape)
            for t in tensors[1:]:
                if any(a != b for i, (a, b) in enumerate(zip(t.shape, shape)) if i != d):
                    return None
            shape[d] = sum(int(t.shape[d]) for t in tensors)
            # the result comes from torch's caching PINNED-host allocator like the pieces: a fresh 67 MB malloc is an
            # mmap whose first touch page-faults and whose release is an munmap (10-90 ms each on a virtualised host)
            res = torch.empty(shape, dtype=tensors[0].dtype, pin_memory=tensors[0].is_pinned())
            outer = int(math.prod(shape[:d]))
            unit = int(math.prod(shape[d + 1:])) * res.element_size()          # bytes of one index along d
            plain = outer <= 64 and res.is_contiguous() and all(t.is_contiguous() for t in tensors)
            off = 0
            for t in tensors:
                t.wait()
                n = int(t.shape[d])
                if plain:
                    # one memmove per outer index: a 3.7 MB piece split over torch's intra-op pool takes anything from
                    # 0.3 to 100 ms on a 128-thread host (tools/host_cat_probe.py), a single-threaded copy 0.4 ms
                    src, dst = t.data_ptr(), res.data_ptr() + off * unit
                    for o in range(outer):
                        ctypes.memmove(dst + o * shape[d] * unit, src + o * n * unit, n * unit)
                else:
                    res.narrow(d, off, n).copy_(t)
                off += n
        return res

    def wait(self) -> torch.Tensor:
        ev = self.__dict__.get("_cpn_ready")
        if ev is not None:
            ev.synchronize()
            self.__dict__["_cpn_ready"] = None
            self.__dict__["_cpn_src"] = None
        return self

    def plain(self) -> torch.Tensor:
        """The wrapped pinned CPU tensor as a plain torch.Tensor, after the wait."""
        self.wait()
        with torch._C.DisableTorchFunctionSubclass():
            return self.as_subclass(torch.Tensor)

    # Accessors to the BYTES that do not (or need not) go through __torch_function__: each waits first.  (Tensor.data_ptr,
    # .untyped_storage, .numpy, .tolist, .item and __dlpack__ do dispatch there today — tests/test_pending_host.py checks
    # every one of them — but the guarantee should not hang on that.)
    def data_ptr(self):
        return self.plain().data_ptr()

    def untyped_storage(self):
        return self.plain().untyped_storage()

    def storage(self):
        return self.plain().storage()

    def numpy(self, *a, **k):
        return self.plain().numpy(*a, **k)

    def tolist(self):
        return self.plain().tolist()

    def __array__(self, *a, **k):
        return self.plain().__array__(*a, **k)

    def __dlpack__(self, *a, **k):
        return self.plain().__dlpack__(*a, **k)

    def __dlpack_device__(self):
        with torch._C.DisableTorchFunctionSubclass():
            return self.as_subclass(torch.Tensor).__dlpack_device__()

    def __deepcopy__(self, memo):
        return self.plain().clone()            # a copy of the values is a plain CPU tensor (copy.deepcopy(out) of a caller)

    def __reduce_ex__(self, proto):
        return self.plain().__reduce_ex__(proto)

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        name = getattr(func, "__name__", "")
        if name == "__get__":                                   # property getters: Tensor.shape.__get__ ...
            name = getattr(getattr(func, "__self__", None), "__name__", "")
        if name == "cpu" and len(args) == 1 and not kwargs:
            return args[0]                                      # already on the CPU: Tensor.cpu() returns self
        if func is torch.cat:
            joined = cls._cat_as_copies_arrive(*args, **kwargs)
            if joined is not None:
                return joined
        if name not in cls._NO_WAIT:
            for t in _flat_tensors((args, kwargs)):
                if isinstance(t, PendingHostTensor):
                    t.wait()
        with torch._C.DisableTorchFunctionSubclass():
            return func(*args, **kwargs)


class RenderEngine:
    """Owns the device-side caches (packed fp16 weights, NHWC fp16 feature maps, workspace) of one model."""

    # per-sample 1x1 convs that run on the fp16 MFMA GEMM: name -> (N_out, K_in, packed leading dimension)
    GEMM_WEIGHTS = {
        "key_map_2": (128, 128, 128),
        "query_embed_2": (128, 128, 128),
        "query_repeat_embed_2": (128, 128, 128),
    }

    # automatic ray-chunk size: the per-sample workspaces (`hid`, 3.6 KB per sample and view; one per call lane) may take
    # this share of the device's memory together, up to MAX_AUTO_CHUNK rays per chunk (the largest launch the GPU tests cover)
    WORKSPACE_SHARE = 0.25
    FREE_SHARE = 0.5                # ... and at most this share of the memory that is free when the workspace is sized
    MAX_AUTO_CHUNK = 65536
    ATTEND_UNITS_MAX_T = 1684       # (160 KiB of LDS - 81 KiB of round-2 weights) / (3 x 4 rays x 4 bytes), csrc/attend_units.hip
    FEW_ROWS = 4096                 # per-ray GEMMs of at most this many rows take the few-row kernel (cpn_gemm_f16_fewrows: 17 vs 35 us at 3 641)
    # precision="auto": default guard threshold on the score sum_i w_i (1 - w_i) |l_i|: half the smallest score of a ray whose
    # fp16 rgb was off by > 5e-4 or a weight by > 1e-3 in the calibration sweep (tools/auto_calibrate.py)
    AUTO_THRESHOLD = 0.5062
    PRECISIONS = ("f16", "f32", "auto")
    TRAIN_PRECISIONS = ("f16", "f32")
    # what a copied engine keeps (__deepcopy__); caches, streams and workspace are derived state
    SETTINGS = ("chunk_rays", "lanes", "grad_scale_target", "call_lanes", "lazy_pixel_val", "precision", "f32_chunk_rays",
                "auto_threshold", "train_precision")

    def __init__(self, chunk_rays: int = 0, lanes: int = 1):
        # ONE per-sample formulation (round 6; rounds 2-5 kept their predecessors as switchable modes - gather + GEMM first layer,
        # un-fused key layer, row-order tails, stored coords_embed, layer-by-layer values, "project before you store": they are
        # in tools/experiments/r6_pruned/ with the measurements that retired them in HISTORY.md): node tables + K = 80 MFMA first
        # layer with the folded key layer behind it (cpn_encode_key), the query / key tails in unit order and both attention
        # rounds on the hidden activations, one launch per round (cpn_attend_units), the folded value projection per ray (cpn_gemm_f16).
        # rays per chunk of the per-sample stages; 0 = automatic (`_auto_chunk`): one 65 536-ray image is ONE chunk on a
        # 288 GB MI355X (28 GB of `hid` at 64 samples) — 4 launches of each per-sample kernel instead of 16 shave the
        # ramp / tail of the persistent grids: 26.6 -> 24.7 ms per image against chunks of 16 384
        self.chunk_rays = int(chunk_rays) or int(os.environ.get("COPONERF_CHUNK_RAYS", "0"))
        # training: every fp16 activation gradient carries a power-of-two scale chosen per backward pass so that the
        # largest entry of the first fp32 -> fp16 gradient lands near this value (train_fns.BackwardPass)
        self.grad_scale_target = 256.0
        # ray chunks are independent: `lanes` HIP streams, each with its own workspace, take the chunks round-robin so
        # that the HBM-bound stages of one chunk (gather, hidden sums) run under the MFMA-bound GEMMs of another
        self.lanes = max(1, int(lanes))
        self._lane_streams: List[torch.cuda.Stream] = []
        # precision="f32" (COPONERF_PRECISION=f32): the reference's arithmetic on this device in the SAME formulation - fp32 node
        # tables, fp32 blends, the first layer's K = 68 block and the 128-wide layers on the exact fp32 MFMA, hid as fp16 (hi, lo)
        # pairs with exact products in the folded key layer (csrc/encode_f32.hip, render_f32.py).  ~5 x slower than the fp16
        # default; the path for models whose attention is sharp enough to leave the fp16 envelope (tests/test_gpu_range.py); the
        # test suite bounds |rgb_f16 - rgb_f32| with it and bench.py reports it as `rays_per_s_f32` beside the headline.
        self.precision = os.environ.get("COPONERF_PRECISION", "f16")
        self.f32_chunk_rays = 16384
        # precision="auto" (COPONERF_PRECISION=auto; inference only, like "f32"): the fp16 default plus a per-ray logit guard
        # (csrc/guard.hip) - rays whose score sum_i w_i (1 - w_i) |l_i| exceeds auto_threshold are rendered again in the reference's
        # arithmetic and merged in before the decoder (_render_body).  inf: no ray; negative: every ray.  One host wait per call
        # (the flagged count).  last_exact_rays = (flagged, total) of the last auto call.
        self.auto_threshold = self.AUTO_THRESHOLD
        # train_precision="f32" (COPONERF_TRAIN_PRECISION=f32): render_train's per-sample stages in the f32 mode's arithmetic, as
        # autograd nodes (train_f32.py); the gradients of the attention sums and of every fp32 layer are fp32, hs's gradient and
        # the first layer's table-form backward keep fp16 operands.  "f16" (default): the fp16 formulation (train_fns.py).
        # `precision` governs render() only.
        self.train_precision = os.environ.get("COPONERF_TRAIN_PRECISION", "f16")
        self.last_exact_rays: Optional[Tuple[int, int]] = None
        self._guard_host: Optional[torch.Tensor] = None
        self._t32: Optional[Tuple[torch.Tensor, torch.Tensor]] = None     # the f32 path's node tables (_f32_inputs)
        self._t32_ready: Optional[torch.cuda.Event] = None                 # ... recorded after their build
        self._wkey = None
        self._w: Dict[str, torch.Tensor] = {}
        self._mkey = None
        self._mrefs: Tuple[torch.Tensor, ...] = ()
        self._maps: List[torch.Tensor] = []
        self._tabs: List[torch.Tensor] = []
        self._wgen = 0                  # bumped whenever the packed weights are rebuilt (the tables depend on them)
        self._l3_hint = None            # (z[3] tensor, its version, NHWC fp16 copy) handed over by get_z's conv_map kernel
        self._hostc = None              # (input tensors, their versions, host copies) of the last call's 4x4 inputs
        self._camc = None               # the device-side products of those inputs (_camera)
        self._next: List[Dict] = []     # what prepare_next() started for the (up to two) pairs after the current one
        self._early: Optional[Dict] = None   # the current pair's own host copy, started by render() ahead of its builds
        self._prep_stream: Optional[torch.cuda.Stream] = None
        self._ws: Dict[str, torch.Tensor] = {}
        self._interval: Dict[Tuple[int, str], torch.Tensor] = {}
        self._auto_chunk_memo: Optional[Tuple[Tuple, int]] = None     # (key, chunk) of the last _auto_chunk decision
        # optional per-kernel timing (bench.py): name -> list of (start_event, end_event, algorithmic_flops)
        self.profile: Optional[Dict[str, list]] = None
        self._copy_stream: Optional[torch.cuda.Stream] = None
        self._pinned_sizes: set = set()     # pixel_val sizes whose second pinned buffer has been parked (_start_host_copy)
        # pixel_val is handed to the caller as a PendingHostTensor (waits for its copy at the first use of the values)
        self.lazy_pixel_val = os.environ.get("COPONERF_EAGER_PIXEL_VAL", "0") != "1"
        self.epoch = 0                  # invalidate() calls so far (captured get_z graphs are keyed on it)
        # consecutive render() calls alternate over this many HIP streams (render() docstring); 1 = the caller's stream
        self.call_lanes = int(os.environ.get("COPONERF_CALL_LANES", "2"))
        self._call_streams: List[torch.cuda.Stream] = []
        self._call_streams_given = False    # set_call_streams() installed the caller's streams
        self._call_idx = 0
        self._ws_prefix = ""            # workspace of the call lane in flight
        self._misses = 0                # cache rebuilds so far (a call that rebuilt something must wait for the caller's stream)
        self._uv_seen = None            # (query-pixel base tensor, its version) of the last call

    # ---- caches --------------------------------------------------------------------------------
    def _buf(self, name: str, shape, dtype, device) -> torch.Tensor:
        n = int(math.prod(shape))
        name = self._ws_prefix + name
        t = self._ws.get(name)
        if t is None or t.numel() < n or t.dtype != dtype or t.device != device:
            t = torch.empty(n, dtype=dtype, device=device)
            self._ws[name] = t
        return t[:n].view(*shape)

    def invalidate(self) -> None:
        """Drop the packed-weight / feature-map caches.  The caches are keyed on tensor identity and `_version`;
        writes that bypass the version counter (`p.data.copy_`, `dist.broadcast(p.data)`: /root/reference
        train.py:58-60) must be followed by this call — CoPoNeRF.load_state_dict and dist.broadcast_parameters do."""
        self._wkey = None
        self._mkey = None
        self._mrefs = ()
        self._maps, self._tabs = [], []
        self._l3_hint = None
        self._hostc = None
        self._camc = None
        self._next = []
        self._early = None
        self._t32 = None
        self.epoch += 1

    def __deepcopy__(self, memo):
        new = RenderEngine()
        for name in self.SETTINGS:
            setattr(new, name, getattr(self, name))
        return new

    @staticmethod
    def _same_inputs(held, versions, mats) -> bool:
        return len(held) == len(mats) and all((a is b) and (a is None or a._version == v)
                                              for a, b, v in zip(held, mats, versions))

    def _host_inputs(self, *mats):
        """Host copies of the call's 4x4 inputs.  The device->host read is a stream synchronisation, and a full-image
        render calls forward() once per ray chunk with the SAME camera tensors (/root/reference test.py:176-190,
        wrapper.py:180-188): the copies are cached on tensor identity + version (the entry holds the tensors).  A copy
        that prepare_next() or _early_host_copy() started on the preparation stream is waited for and used instead of
        a synchronous read behind everything queued on the caller's stream."""
        c = self._hostc
        if c is not None and self._same_inputs(c[0], c[1], mats):
            return c[2]
        nx = next((e for e in [self._early] + self._next if e is not None and e["stage"] is not None and
                   self._same_inputs(e["mats"], e["versions"], mats)), None)
        if nx is not None:
            nx["copied"].synchronize()
            host = _split_host(mats, nx["stage"])
            nx["stage"] = nx["flat"] = None
        else:
            host = _to_host(*mats)
        self._early = None
        self._hostc = (mats, tuple(None if m is None else m._version for m in mats), host)
        return host

    def _camera_entry(self, mats, val: bool, H: int, dev):
        c = self._camc
        if c is not None and c[1] == (bool(val), H, dev) and c[3]["_flat"]._version == c[2] and \
                self._same_inputs(c[0][0], c[0][1], mats):
            return c[3]
        return None

    def _prep(self, dev) -> "torch.cuda.Stream":
        if self._prep_stream is None or self._prep_stream.device != dev:
            self._prep_stream = torch.cuda.Stream(device=dev)
        return self._prep_stream

    def _start_host_copy_of(self, mats, main, side) -> Dict:
        """One pinned device->host copy of the live 4x4 inputs on `side`, ordered after what `main` holds now."""
        ev = torch.cuda.Event()
        ev.record(main)
        side.wait_event(ev)
        e: Dict = {"mats": mats, "versions": tuple(None if m is None else m._version for m in mats), "stage": None,
                   "flat": None, "copied": None}
        with torch.cuda.stream(side):
            flat = _flat_on_device(mats)
            if flat is not None:
                e["flat"] = flat                # kept until the copy has been consumed
                e["stage"] = torch.empty(flat.numel(), dtype=torch.float32, pin_memory=True)
                e["stage"].copy_(flat, non_blocking=True)
                e["copied"] = torch.cuda.Event()
                e["copied"].record(side)
        return e

    def _early_host_copy(self, mats, val: bool, H: int, dev) -> None:
        """render() calls this BEFORE it queues a new pair's device-side builds (maps, tables, flow products): the copy of
        the 4x4 inputs to the host is ordered after the work queued so far only, so the host pose algebra of _camera
        (0.5 ms) runs while the device builds the tables instead of after them with the device idle."""
        if self._camera_entry(mats, val, H, dev) is not None:
            return
        c = self._hostc
        if c is not None and self._same_inputs(c[0], c[1], mats):
            return
        if any(e["stage"] is not None and self._same_inputs(e["mats"], e["versions"], mats) for e in self._next):
            return
        self._early = self._start_host_copy_of(mats, torch.cuda.current_stream(dev), self._prep(dev))

    def _camera(self, ctx_c2w, ctx_K, qry_c2w, qry_K, rel_pose, val: bool, H: int, dev) -> Dict[str, torch.Tensor]:
        """Device copies of everything the O(B) host pose algebra produces for a call (camera block, Tq, the output-side
        inverses, the ray constants of cpn_ray_outputs, rel_pose_flip): ONE pinned upload, cached on the identity and
        version of the five input tensors — a full-image render is 18 forward() calls with the same cameras
        (/root/reference test.py:176-190).  The entries are views of one flat buffer that is also handed to the caller
        (gt_rel_pose ...): an in-place write to any of them bumps the buffer's version and drops the entry."""
        if not val and torch.is_grad_enabled():
            # a training step: the geometry uses the given poses (CoPoNeRF.py:239-244, 325-332), rel_pose is this step's
            # network output and only its inverse would be taken here - which the caller forms on the device when it
            # differentiates (CoPoNeRF._render).  Left in, it made every step a cache miss whose device -> host read
            # waited for get_z (3.7 ms of host stall per step, tools/host_step_profile.py)
            rel_pose = None
        mats = (ctx_c2w, ctx_K, qry_c2w, qry_K, rel_pose)
        hit = self._camera_entry(mats, val, H, dev)
        if hit is not None:
            return hit
        self._misses += 1
        hc2w, hK, hqc2w, hqK, hrel = self._host_inputs(*mats)
        cam_cpu, Tq_cpu = build_camera_block(hc2w, hK, hqc2w, hqK, hrel, val, H)
        prods = host_pose_products(hc2w, hqc2w, hqK)
        host = dict(prods, cam=cam_cpu, Tq=Tq_cpu, rayc=build_ray_constants(prods, hK, Tq_cpu))
        if hrel is not None:
            host["rel_pose_flip"] = _rigid_inverse(hrel)
        up = _upload(host, dev)
        self._camc = ((mats, tuple(None if m is None else m._version for m in mats)), (bool(val), H, dev),
                      up["_flat"]._version, up)
        return up

    def adopt_level3(self, z3: torch.Tensor, nhwc16: torch.Tensor) -> None:
        """get_z's conv_map kernel already wrote the full-resolution level as NHWC fp16: use it for THIS z3 tensor
        (matched by identity and version) instead of converting it again."""
        self._l3_hint = (z3, z3._version, nhwc16)

    def _weights(self, params: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        key = tuple((id(p), p.data_ptr(), p._version) for p in params.values())
        if key == self._wkey:
            return self._w
        self._misses += 1
        dev = params["query_encode_latent.weight"].device
        w: Dict[str, torch.Tensor] = {}
        s = _stream()
        for name, (n_out, k_in, ld) in self.GEMM_WEIGHTS.items():
            src = params[name + ".weight"].detach().reshape(n_out, k_in).contiguous().float()
            dst = torch.empty(n_out, ld, dtype=torch.float16, device=dev)
            call("cpn_pack_weight_f16", src.data_ptr(), n_out, k_in, dst.data_ptr(), ld, s)
            w[name + ".w16"] = dst
            w[name + ".b"] = params[name + ".bias"].detach().float().contiguous()
        f32 = lambda n: params[n].detach().float().contiguous()
        w["query_encode_latent.b"] = f32("query_encode_latent.bias")
        # ---- folding: query_encode_latent_2 is linear and feeds only linear layers, so
        #      key_map and latent_value act directly on the 2 x 832 hidden activations [h_own ; h_other]:
        #      W' = [W_a . W2 | W_b . W2],  c' = W_a b2 + W_b b2 + b   (products in float64, then one rounding); the fp32 W'
        #      stays in the entry for the reference-arithmetic path (render_f32.weights)
        W2 = f32("query_encode_latent_2.weight").reshape(416, 832).double()
        b2 = f32("query_encode_latent_2.bias").double()

        def fold(wname, bname, n_out):
            Wx = f32(wname).reshape(n_out, 832).double()
            Wf = torch.cat((Wx[:, :416] @ W2, Wx[:, 416:] @ W2), dim=1)                  # (n_out, 1664)
            cf = Wx[:, :416] @ b2 + Wx[:, 416:] @ b2 + f32(bname).double()
            dst = torch.empty(n_out, 1664, dtype=torch.float16, device=dev)
            src = Wf.float().contiguous()
            call("cpn_pack_weight_f16", src.data_ptr(), n_out, 1664, dst.data_ptr(), 1664, s)
            return src, dst, cf.float().contiguous()

        w["key_fold.w"], w["key_fold.w16"], w["key_fold.b"] = fold("key_map.weight", "key_map.bias", 128)
        # the same matrix in the order cpn_encode_key streams it through its LDS ring: [image j][slice n][tile t][k][lane =
        # row + 16 * 8-column group][8] - every 1 KiB DMA piece contiguous
        w["key_fold.wpk"] = pack_key_ring(w["key_fold.w16"])
        w["value_fold.w"], w["value_fold.w16"], w["value_fold.b"] = fold("latent_value.weight", "latent_value.bias", 416)
        # the same matrix in MFMA fragment order for the few-row form of the per-ray value projection (cpn_gemm_f16_fewrows)
        w["value_fold.wpk"] = torch.empty(416 * 1664, dtype=torch.float16, device=dev)
        call("cpn_pack_gemm_frags", w["value_fold.w16"].data_ptr(), 1664, 416, 1664, w["value_fold.wpk"].data_ptr(), s)
        w["query_embed.w"] = f32("query_embed.weight").reshape(128, 16)
        w["query_embed.b"] = f32("query_embed.bias")
        wr = f32("query_repeat_embed.weight").reshape(128, 144)
        w["query_repeat_embed.w_z"] = wr[:, :128].contiguous()           # acts on encode_latent(z_local)
        w["query_repeat_embed.w_l"] = wr[:, 128:].contiguous()           # acts on local_coords (16)
        w["query_repeat_embed.b"] = f32("query_repeat_embed.bias")
        w["encode_latent.w"] = f32("encode_latent.weight").reshape(128, 416)
        w["encode_latent.b"] = f32("encode_latent.bias")
        lin_in = torch.zeros(128, 32, dtype=torch.float32, device=dev)   # K padded 18 -> 32
        lin_in[:, :18] = f32("phi.lin_in.weight")
        w["phi.lin_in.w"], w["phi.lin_in.b"] = lin_in, f32("phi.lin_in.bias")
        for k in range(3):
            wz = f32(f"phi.lin_z.{k}.weight")
            # phi sees [z_local ; z_local] (CoPoNeRF.py:547-554): fold the two 416-column halves
            w[f"phi.lin_z.{k}.w"] = (wz[:, :416] + wz[:, 416:]).contiguous()
            w[f"phi.lin_z.{k}.b"] = f32(f"phi.lin_z.{k}.bias")
            for fc in ("fc_0", "fc_1"):
                w[f"phi.blocks.{k}.{fc}.w"] = f32(f"phi.blocks.{k}.{fc}.weight")
                w[f"phi.blocks.{k}.{fc}.b"] = f32(f"phi.blocks.{k}.{fc}.bias")
        w["phi.lin_out.w"], w["phi.lin_out.b"] = f32("phi.lin_out.weight"), f32("phi.lin_out.bias")
        # the whole decoder as one block for cpn_lightfield_decode (layout: include/coponerf_hip.h)
        wout = torch.zeros(16, 128, dtype=torch.float32, device=dev)
        wout[:3] = w["phi.lin_out.w"]
        bout = torch.zeros(16, dtype=torch.float32, device=dev)
        bout[:3] = w["phi.lin_out.b"]
        fr = frag_order_f32
        parts = [fr(w["phi.lin_in.w"]), w["phi.lin_in.b"]]
        for k in range(3):
            parts += [fr(w[f"phi.lin_z.{k}.w"]), w[f"phi.lin_z.{k}.b"], fr(w[f"phi.blocks.{k}.fc_0.w"]), w[f"phi.blocks.{k}.fc_0.b"],
                      fr(w[f"phi.blocks.{k}.fc_1.w"]), w[f"phi.blocks.{k}.fc_1.b"]]
        w["phi.pack"] = torch.cat([t.reshape(-1) for t in parts + [fr(wout), bout]])
        assert w["phi.pack"].numel() == _hip.LIGHTFIELD_PACK_FLOATS
        # ---- "project, then interpolate" form of the first layer (csrc/encode.hip): MFMA fragments of the
        #      full-resolution / point-encoding columns and the table projection weights of the three coarse levels
        W1 = f32("query_encode_latent.weight").reshape(832, 835)
        w["enc.frag"] = torch.empty(_hip.ENC_FRAG_HALVES, dtype=torch.float16, device=dev)
        w["enc.wtab"] = torch.empty(_hip.TAB_LD, 768, dtype=torch.float16, device=dev)
        call("cpn_pack_encode_weights", W1.data_ptr(), 835, w["enc.frag"].data_ptr(), w["enc.wtab"].data_ptr(), s)
        w["enc.zero_bias"] = torch.zeros(_hip.TAB_LD, dtype=torch.float32, device=dev)
        self._w, self._wkey = w, key
        self._wgen += 1
        return w

    def _feature_maps(self, z: Sequence[torch.Tensor], w: Dict[str, torch.Tensor]):
        """NHWC fp16 copies of the four latent maps and, for the three coarse levels, their projection through the
        first encoder layer (tables, csrc/encode.hip).  Cached per (z tensors, weight generation): the entry holds
        strong references to the z tensors and compares identity, so a freed-and-reallocated tensor at the same
        address can never hit it."""
        key = self._maps_key(z)
        if self._same_maps(self._mkey, self._mrefs, key, z):
            return self._maps, self._tabs
        self._misses += 1
        nx = next((e for e in self._next if self._same_maps(e["mkey"], e["z"], key, z)), None)
        if nx is not None:
            # built by prepare_next() on its own stream while the previous pair rendered
            # Their blocks belong to the preparation stream's pool: record the adopting stream on them so that a block is
            # not handed out again before this stream's readers are done, whatever stream the NEXT preparation is issued
            # from (the preparation stream also begins every preparation by waiting for the caller's then-current stream,
            # which covers the chunk lanes: their completion is joined into the caller's stream before render() returns).
            cur = torch.cuda.current_stream(z[0].device)
            cur.wait_event(nx["built"])
            maps, tabs = nx["maps"], nx["tabs"]
            for t in list(maps) + list(tabs):
                t.record_stream(cur)
            nx["mkey"], nx["maps"], nx["tabs"] = None, None, None
        else:
            maps, tabs = self._build_maps(z, w)
        self._maps, self._tabs, self._mkey, self._mrefs = maps, tabs, key, tuple(z)
        self._t32 = None                # the f32 path's tables belong to the entry replaced
        return maps, tabs

    def _maps_key(self, z: Sequence[torch.Tensor]):
        return tuple((t._version, tuple(t.shape)) for t in z) + (self._wgen,)

    @staticmethod
    def _same_maps(held_key, held_z, key, z) -> bool:
        """A feature-map entry (its _maps_key and z tensors) is the one of `z`: same key and the same tensors by identity."""
        return held_key == key and len(held_z) == len(z) and all(a is b for a, b in zip(held_z, z))

    def _build_maps(self, z: Sequence[torch.Tensor], w: Dict[str, torch.Tensor]):
        """The launches behind _feature_maps, on the current stream."""
        maps, tabs, s = [], [], _stream()
        hint = self._l3_hint
        for i, t in enumerate(z):
            if i == 3 and hint is not None and hint[0] is t and hint[1] == t._version:
                maps.append(hint[2])
                continue
            src = t.detach().float().contiguous()
            n, c, h, w_ = src.shape
            dst = torch.empty(n, h, w_, c, dtype=torch.float16, device=src.device)
            call("cpn_nchw_to_nhwc_f16", src.data_ptr(), dst.data_ptr(), n, c, h, w_, s)
            maps.append(dst)
        # node tables of the three coarse levels (csrc/encode.hip): sample the levels at every node of the common
        # grid, then project the (nodes, 768) features through the first layer's column blocks in ONE GEMM
        nimg, Hf, Wf = maps[3].shape[0], maps[3].shape[1], maps[3].shape[2]
        nodes = nimg * int(_hip.lib().cpn_encode_table_nodes(Hf, Wf))
        feat = torch.empty(nodes, 768, dtype=torch.float16, device=maps[0].device)
        call("cpn_node_features", maps[0].data_ptr(), maps[1].data_ptr(), maps[2].data_ptr(), Hf, Wf, nimg,
             feat.data_ptr(), s)
        tab = torch.empty(nodes, _hip.TAB_LD, dtype=torch.float16, device=feat.device)
        call("cpn_gemm_f16", feat.data_ptr(), 768, w["enc.wtab"].data_ptr(), 768, w["enc.zero_bias"].data_ptr(),
             tab.data_ptr(), _hip.TAB_LD, nodes, _hip.TAB_LD, 768, 0, 0, s)
        tabs.append(tab)
        return maps, tabs

    def _f32_inputs(self, pz, w: Dict[str, torch.Tensor], H: int, W: int):
        """(w, (tab, map3)): the weight entry with its f32 section and the fp32 node tables of the current pair (_t32, dropped
        with the _feature_maps entry and by invalidate()), built on the stream of the first call that needs them.  Every reader,
        on any call lane, waits for that build and is recorded on the tables (their blocks are the building stream's)."""
        params, z = pz
        cur = torch.cuda.current_stream(z[0].device)
        if self._t32 is None:
            render_f32.weights(w, params)
            self._t32 = render_f32.node_tables(z, w, H, W, _stream())
            self._t32_ready = torch.cuda.Event()
            self._t32_ready.record(cur)
        cur.wait_event(self._t32_ready)
        for t in self._t32:
            t.record_stream(cur)
        return w, self._t32

    @torch.no_grad()
    def prepare_next(self, params: Dict[str, torch.Tensor], ctx_c2w, ctx_K, qry_c2w, qry_K, z: Sequence[torch.Tensor],
                     rel_pose, flow=None, width: Optional[int] = None) -> None:
        """Start the per-pair preparation of the pair that will be rendered AFTER the one about to be rendered (or being
        rendered): the device->host copy of its 4x4 inputs, the NHWC fp16 copies of its latent maps, its node tables and,
        with `flow` and `width` (the context images' height) given, its flow products — on a stream of their own that is
        ordered after everything queued on the caller's stream so far.  The render() call on these SAME tensors (identity
        + version) then finds them instead of rebuilding: its host pose algebra needs no device synchronisation behind the
        previous pair's kernels, and its table build ran beside them (0.35 ms of kernels at 256x256).
        Call it before render() of the current pair is queued so that the copy is not ordered behind that render:
            prepare_next(pair[i+1]); render(pair[i]); prepare_next(pair[i+2]); render(pair[i+1]); ...
        Two prepared pairs are held (the one about to be rendered and the one after it); a third replaces the older.
        Results are those of an unprepared call, bit for bit (the same kernels on the same inputs).
        Stream contract: issue prepare_next() and the render() that consumes it from the SAME torch stream (the loop above
        on one stream is the supported use).  The adopted maps and tables are record_stream-ed for the adopting stream,
        so rendering from another stream is memory-safe, but the staged host copy of the 4x4 inputs is ordered only
        against the stream prepare_next() was called on."""
        dev = z[0].device
        if dev.type != "cuda":
            raise RuntimeError("coponerf_amd renders on a HIP device only (got z on %s)" % dev)
        if self.precision == "f32":
            return
        main = torch.cuda.current_stream(dev)
        w = self._weights(params)
        side = self._prep(dev)
        mats = (ctx_c2w, ctx_K, qry_c2w, qry_K, rel_pose)
        nx = self._start_host_copy_of(mats, main, side)
        nx["z"] = tuple(z)
        with torch.cuda.stream(side):
            key = self._maps_key(z)
            if self._same_maps(self._mkey, self._mrefs, key, z):
                nx["mkey"], nx["maps"], nx["tabs"], nx["built"] = None, None, None, None
            else:
                nx["maps"], nx["tabs"] = self._build_maps(z, w)
                nx["mkey"] = key
                nx["built"] = torch.cuda.Event()
                nx["built"].record(side)
        if flow is not None and width is not None:
            from .aux_outputs import prepare_flow_products
            prepare_flow_products(flow, int(width), side)
        # entries whose pieces were all consumed have nothing left to hand over
        self._next = [nx] + [e for e in self._next if e["stage"] is not None or e["mkey"] is not None][:1]

    # ---- geometry shared by the inference and the training pass (never differentiated) ----------------
    @torch.no_grad()
    def _geometry(self, ctx_c2w, ctx_K, qry_c2w, qry_K, uv, rel_pose, val, S, H, W):
        dev = uv.device
        B, _, R, _ = uv.shape
        up = self._camera(ctx_c2w, ctx_K, qry_c2w, qry_K, rel_pose, val, H, dev)
        uvc, uvs = _uv_rows(uv, B, R)
        new = lambda name, shape, dt: torch.empty(shape, dtype=dt, device=dev)
        g = self._launch_geometry(new, up["cam"], uvc, uvs, self._sample_interval(S, dev), B, R, S, H, W)
        g["Tq"], g["host"] = up["Tq"], up
        return g

    def _sample_interval(self, S: int, dev) -> torch.Tensor:
        """linspace(0, 1, S) on the device (a CPU linspace, as the oracle's), made once per (S, device): a build is a miss."""
        ikey = (S, str(dev))
        if ikey not in self._interval:
            self._interval[ikey] = torch.linspace(0, 1, S).to(dev)
            self._misses += 1
        return self._interval[ikey]

    @staticmethod
    def _launch_geometry(new, cam, uvc, uvs, interval, B, R, S, H, W, lvu=None) -> Dict[str, torch.Tensor]:
        """The geometry launches of render() and render_train(), on the current stream, into tensors from new(name, shape,
        dtype): per ray and view coords9, seg, overlaps (cpn_project_rays); per sample pixel_val, pt, sec_grid, pe6, loc8 and,
        given `lvu`, the unit-order inputs of cpn_local_units (cpn_sample_geometry)."""
        N = B * V
        shapes = {"coords9": (N, R, 9), "seg": (N, R, 4), "overlaps": (N, R), "pixel_val": (N, R, S, 2), "pt": (N, R, S, 3),
                  "sec_grid": (N, R, S, 2), "pe6": (N, R, S, 6), "loc8": (N, R, S, 8)}
        g = {k: new(k, shape, torch.uint8 if k == "overlaps" else torch.float32) for k, shape in shapes.items()}
        s = _stream()
        call("cpn_project_rays", cam.data_ptr(), uvc.data_ptr(), uvs, B, V, R, g["coords9"].data_ptr(), g["seg"].data_ptr(),
             g["overlaps"].data_ptr(), s)
        call("cpn_sample_geometry", cam.data_ptr(), g["coords9"].data_ptr(), g["seg"].data_ptr(), interval.data_ptr(),
             B, V, R, S, H, W, g["pixel_val"].data_ptr(), g["pt"].data_ptr(), g["sec_grid"].data_ptr(),
             g["pe6"].data_ptr(), g["loc8"].data_ptr(), _ptr(lvu), s)
        return g

    def _start_host_copy(self, t):
        """Device->host copy of `t` into pinned memory on the side stream, ordered after the work queued so far; returns
        (host tensor, event to synchronize on before handing it out)."""
        dev = t.device
        if self._copy_stream is None or self._copy_stream.device != dev:
            self._copy_stream = torch.cuda.Stream(device=dev)
        host = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
        nbytes = t.numel() * t.element_size()
        if nbytes not in self._pinned_sizes:
            # a caller that still holds one call's pixel_val while it makes the next call (`out = model(...)` in a loop) needs two
            # such buffers, and pinning 67 MB takes milliseconds: the second one is pinned with the first, inside the first call
            # of this size, and parked in torch's caching host allocator (a loop's SECOND call was 3.8 ms slower than its third)
            self._pinned_sizes.add(nbytes)
            spare = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
            del spare
        ready = torch.cuda.Event()
        ready.record()
        with torch.cuda.stream(self._copy_stream):
            self._copy_stream.wait_event(ready)
            host.copy_(t, non_blocking=True)
            done = torch.cuda.Event()
            done.record()
        # `t` was allocated on the caller's / call lane's stream and the copy stream reads it after the caller may have
        # dropped it: tell the caching allocator, or the block can be handed to the next call on that lane while the
        # copy is still reading it
        t.record_stream(self._copy_stream)
        return host, done

    # ---- the differentiable render pass (training; gradients to the render weights and to z) ------------
    def render_train(self, params: Dict[str, torch.Tensor], ctx_c2w, ctx_K, qry_c2w, qry_K, uv,
                     z: Sequence[torch.Tensor], rel_pose, val: bool, S: int, H: int, W: int) -> Dict[str, torch.Tensor]:
        """Same forward kernels as render(), wrapped in autograd Functions; all rays of the call form one chunk (training uses
        <= 4096 rays per pair, /root/reference train.py:87).  `train_precision` picks the per-sample stages: "f16" the fp16
        formulation (coponerf_amd/train_fns.py), "f32" the f32 mode's arithmetic (coponerf_amd/train_f32.py).  `precision`
        is not consulted: it governs render() only ("auto" has no training form)."""
        if self.train_precision not in self.TRAIN_PRECISIONS:
            raise ValueError(f"RenderEngine.train_precision must be 'f16' or 'f32' (got {self.train_precision!r})")
        from .train_fns import (AttendHiddenFn, BackwardPass, EncodeFn, GemmFn, KeyForward, KeyLayerFn, LinearF32Fn,
                                LocalHiddenFn)
        dev = uv.device
        if dev.type != "cuda":
            raise RuntimeError("coponerf_amd renders on a HIP device only (got uv on %s)" % dev)
        B, _, R, _ = uv.shape
        if B * R > 32768:
            raise ValueError("render_train keeps all activations of the call: at most 32768 rays per call")
        g = self._geometry(ctx_c2w, ctx_K, qry_c2w, qry_K, uv, rel_pose, val, S, H, W)
        pixel_val_cpu, copy_done = self._start_host_copy(g["pixel_val"])    # the caller contract's CPU copy, off the main stream
        dims = (B, V, R, S)
        bp = BackwardPass(self.grad_scale_target)   # the fp16 gradient scale and the nodes' hand-offs of this backward pass
        P = params
        mat = lambda n, rows: P[n + ".weight"].reshape(rows, -1)
        bias = lambda n: P[n + ".bias"]
        W2, b2 = mat("query_encode_latent_2", 416), bias("query_encode_latent_2")

        def fold(name, n_out):                                   # differentiable fp32 fold
            Wa, Wb = mat(name, n_out).chunk(2, 1)                # one split node, not four slices (each a fill + copy + add backward)
            if self.train_precision == "f32":                    # its products in float64, as _weights folds for render()
                W2d, Wa, Wb = W2.double(), Wa.double(), Wb.double()
                return (torch.cat((Wa @ W2d, Wb @ W2d), dim=1).float(),
                        ((Wa + Wb) @ b2.double() + bias(name).double()).float())
            return torch.cat((Wa @ W2, Wb @ W2), dim=1), (Wa + Wb) @ b2 + bias(name)

        Wkf, ckf = fold("key_map", 128)
        Wvf, cvf = fold("latent_value", 416)
        if self.train_precision == "f32":
            from .train_f32 import render_samples
            zl, w1 = render_samples(P, mat, bias, z, g, (Wkf, ckf), (Wvf, cvf), dims, (H, W), bp)
            return self._train_outputs(P, g, zl, w1, B, R, pixel_val_cpu, copy_done)
        kf = KeyForward(Wkf, ckf)                   # the folded key layer's forward rides in the first layer's kernel
        # the first layer on the node tables with the key layer behind it, as in inference: no gathered input in the forward pass
        hid = EncodeFn.apply(z[0], z[1], z[2], z[3], mat("query_encode_latent", 832), bias("query_encode_latent"),
                             g["pixel_val"], g["sec_grid"], g["pe6"], dims, (H, W), bp, kf)
        hid2 = hid.view(-1, 1664)
        # the last consumer of hid in the backward pass: adds the parts the attention sums parked and masks by hid > 0
        kh = KeyLayerFn.apply(hid2, Wkf, ckf, kf, dims, bp)
        # in_relu: its data gradient comes back masked by kh > 0, handed over to the key layer
        key2 = GemmFn.apply(kh, mat("key_map_2", 128), bias("key_map_2"), False, False, bp, True)
        hq = LocalHiddenFn.apply(g["loc8"], g["coords9"], mat("query_embed", 128), bias("query_embed"), None, dims, bp)
        ce = GemmFn.apply(hq, mat("query_embed_2", 128), bias("query_embed_2"), False, False, bp)
        hbar1, w1 = AttendHiddenFn.apply(key2, ce, hid2, dims, bp, True)       # coords_embed is shared by the two rounds
        z1 = GemmFn.apply(hbar1, Wvf, cvf, False, True, bp)
        ze = LinearF32Fn.apply(z1, mat("encode_latent", 128), bias("encode_latent"), None, False, False)
        Wr_z, Wr_l = mat("query_repeat_embed", 128).split((128, 16), 1)
        aq = LinearF32Fn.apply(ze, Wr_z.contiguous(), None, None, False, False)
        q2h = LocalHiddenFn.apply(g["loc8"], g["coords9"], Wr_l.contiguous(), bias("query_repeat_embed"), aq, dims, bp)
        q2 = GemmFn.apply(q2h, mat("query_repeat_embed_2", 128), bias("query_repeat_embed_2"), False, False, bp)
        hbar2, _ = AttendHiddenFn.apply(q2, ce, hid2, dims, bp, False)
        zs = GemmFn.apply(hbar2, Wvf, cvf, False, True, bp)
        zl = zs + float(V) * z1                                  # CoPoNeRF.py:481-485
        return self._train_outputs(P, g, zl, w1, B, R, pixel_val_cpu, copy_done)

    @staticmethod
    def _train_outputs(P, g, zl, w1, B, R, pixel_val_cpu, copy_done) -> Dict[str, torch.Tensor]:
        """render_train's tail for either train_precision: the decoder on z_local (fp32, LinearF32Fn), the white background
        and the outputs; w1 = the round-1 softmax weights (at_wt)."""
        from .train_fns import LinearF32Fn
        dev = zl.device
        nray = B * R
        c18 = torch.zeros(nray, 32, dtype=torch.float32, device=dev)
        c18[:, :18] = g["coords9"].view(B, V, R, 9).permute(0, 2, 1, 3).reshape(nray, 18)
        x = LinearF32Fn.apply(c18, torch.nn.functional.pad(P["phi.lin_in.weight"], (0, 14)), P["phi.lin_in.bias"], None,
                              False, False)
        for k in range(3):
            Wz_a, Wz_b = P[f"phi.lin_z.{k}.weight"].chunk(2, 1)
            x = LinearF32Fn.apply(zl, Wz_a + Wz_b, P[f"phi.lin_z.{k}.bias"], x, False, False)
            net = LinearF32Fn.apply(x, P[f"phi.blocks.{k}.fc_0.weight"], P[f"phi.blocks.{k}.fc_0.bias"], None, True, False)
            x = LinearF32Fn.apply(net, P[f"phi.blocks.{k}.fc_1.weight"], P[f"phi.blocks.{k}.fc_1.bias"], x, True, False)
        raw = LinearF32Fn.apply(x, P["phi.lin_out.weight"], P["phi.lin_out.bias"], None, True, False)     # (nray, 3)
        valid = g["overlaps"].view(B, V, R).any(dim=1).float()
        rgb = raw.view(B, R, 3) * valid[..., None] + (1 - valid[..., None])
        copy_done.synchronize()
        return {"rgb": rgb.view(B, 1, R, 3), "valid_mask": valid[..., None], "pixel_val": g["pixel_val"],
                "pixel_val_cpu": pixel_val_cpu, "pt": g["pt"], "at_wt": w1, "coords": g["coords9"],
                "z_local": zl, "Tq": g["Tq"], "sec_grid": g["sec_grid"], "rgb_raw": raw, "host": g["host"]}

    def _auto_chunk(self, S: int, dev, nrays: int = 0) -> int:
        """Largest multiple of 1024 rays (<= MAX_AUTO_CHUNK) whose per-sample workspace, summed over ALL the call lanes
        that can be in flight (each keeps its own `hid`), fits both WORKSPACE_SHARE of the device and FREE_SHARE of the
        memory that is free right now (plus what this engine's workspace and torch's cache already hold): beside a
        training job or captured get_z graphs in the same process the chunks shrink instead of the call running out of
        memory.  The decision is kept per (S, device, settings) for as long as the workspace of the current call lane already
        holds a chunk of `nrays` rays at that size (nothing would be allocated); otherwise free memory is consulted again."""
        key = (S, str(dev), self.lanes, self.call_lanes)
        hit = self._auto_chunk_memo
        if hit is not None and hit[0] == key:
            have = self._ws.get(self._ws_prefix + "hid.0")
            if have is not None and have.device == dev and have.numel() >= min(hit[1], max(1, nrays)) * V * S * 2 * 832:
                return hit[1]
        nws = max(1, self.lanes) * max(1, self.call_lanes)                              # workspaces alive at once
        per_ray = V * S * (2 * 832 * 2 + 128 * 2 + 4) * nws                             # hid + kh of the fused key layer + logits
        total = torch.cuda.get_device_properties(dev).total_memory
        budget = int(total * self.WORKSPACE_SHARE)
        try:
            free, _ = torch.cuda.mem_get_info(dev)
            own = sum(t.numel() * t.element_size() for t in self._ws.values() if t.device == dev)
            cached = max(0, torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev))
            budget = min(budget, int((free + own + cached) * self.FREE_SHARE))
        except RuntimeError:
            pass
        fit = budget // per_ray
        C = int(max(1024, min(self.MAX_AUTO_CHUNK, fit // 1024 * 1024)))
        self._auto_chunk_memo = (key, C)
        return C

    # ---- the render pass -------------------------------------------------------------------------
    def set_call_streams(self, streams: Optional[Sequence[torch.cuda.Stream]]) -> None:
        """Streams the consecutive render() calls alternate over instead of the engine's own (None: back to those) —
        e.g. CU-masked lanes inside the render share of a partitioned chip (coponerf_amd/streams.py).  The caller keeps
        them alive and orders their work before dropping them."""
        self._call_streams = list(streams) if streams else []
        self._call_streams_given = bool(streams)
        self._call_idx = 0
        self._uv_seen = None        # new streams have waited for nothing: the next call must order itself behind the caller's

    def _call_stream(self, dev) -> Optional[torch.cuda.Stream]:
        if self.call_lanes <= 1:
            return None
        if self._call_streams_given:
            if len(self._call_streams) != self.call_lanes or self._call_streams[0].device != dev:
                raise RuntimeError("set_call_streams: need call_lanes streams on the render device")
        elif len(self._call_streams) != self.call_lanes or self._call_streams[0].device != dev:
            self._call_streams = [torch.cuda.Stream(device=dev) for _ in range(self.call_lanes)]
            self._uv_seen = None    # (see set_call_streams)
        self._call_idx = (self._call_idx + 1) % self.call_lanes
        return self._call_streams[self._call_idx]

    @torch.no_grad()
    def render(self, params: Dict[str, torch.Tensor], ctx_c2w, ctx_K, qry_c2w, qry_K, uv, z: Sequence[torch.Tensor],
               rel_pose, val: bool, S: int, H: int, W: int, debug: bool = False, inp: Optional[Dict] = None,
               flow=None) -> Dict[str, torch.Tensor]:
        """uv (B,1,R,2) on the device; 4x4 inputs on any device.  Returns device tensors:
        rgb (B,1,R,3), valid_mask (B,R,1), pixel_val (N,R,S,2), pt (N,R,S,3), at_wt (N,R,S),
        coords (N,R,9), z_local (B*R,416), Tq (B,V,4,4) (device copy of the host pose algebra); `pixel_val_cpu` is the
        pinned CPU copy (a PendingHostTensor while the copy stream may still be writing it); with `inp` and `flow` given,
        `aux` = the per-ray auxiliary outputs (aux_outputs.ray_outputs).  debug=True adds sec_grid / rgb_raw (and, with
        precision="auto", guard_score (B,R) fp32: each ray's logit-guard score).

        Consecutive calls are independent (a full-image render is 18 of them in the reference's callers, test.py:176-190),
        so they alternate over `call_lanes` HIP streams: the small per-ray kernels and the tails of the persistent
        per-sample kernels of one call run under the next call's kernels (18-call loop: 28.7 -> 25.5 ms, the time of ONE
        full-image call).  Stream discipline: (1) everything cached (packed weights, feature tables, camera block, flow
        products) is looked up / rebuilt on the CALLER's stream before the switch; (2) the call's stream waits for the
        caller's stream only if one of those lookups missed or the query-pixel tensor is new — otherwise all inputs were
        already ordered before an earlier call and a wait would serialise the call behind its predecessor; (3) outputs are
        allocated on the call's stream and `record_stream`-ed for the caller's; (4) the caller's stream waits for the
        call's completion event (no host wait)."""
        dev = uv.device
        if dev.type != "cuda":
            raise RuntimeError("coponerf_amd renders on a HIP device only (got uv on %s)" % dev)
        B, _, R, _ = uv.shape
        if z[0].shape[0] != B * V or len(z) != 4:
            raise ValueError("expected 4 latent maps with a leading dimension of B*2")
        if self.precision not in self.PRECISIONS:
            raise ValueError(f"RenderEngine.precision must be 'f16', 'f32' or 'auto' (got {self.precision!r})")
        main = torch.cuda.current_stream()
        miss0 = self._misses
        w = self._weights(params)
        # a new pair: its 4x4 inputs start their way to the host first, its device-side builds are queued next, and the
        # host pose algebra (which has to wait for that copy only) runs while the device builds
        self._early_host_copy((ctx_c2w, ctx_K, qry_c2w, qry_K, rel_pose), val, H, dev)
        maps, tabs = self._feature_maps(z, w)
        fp = None
        if flow is not None and inp is not None:
            from .aux_outputs import flow_products
            fp, hit = flow_products(flow, inp["context"]["rgb"].shape[-2])
            self._misses += 0 if hit else 1
        up = self._camera(ctx_c2w, ctx_K, qry_c2w, qry_K, rel_pose, val, H, dev)
        interval = self._sample_interval(S, dev)
        uvc, uvs = _uv_rows(uv, B, R)
        base = uv._base if uv._base is not None else uv
        side = self._call_stream(dev)            # may install new lane streams, which resets _uv_seen (-> fresh)
        seen = self._uv_seen
        fresh = self._misses != miss0 or seen is None or seen[0] is not base or seen[1] != base._version or \
            uvc.untyped_storage().data_ptr() != uv.untyped_storage().data_ptr()
        self._uv_seen = (base, base._version)
        pre = (w, maps, tabs, up, interval, uvc, uvs, fp, (params, z))
        if side is None:
            self._ws_prefix = ""
            return self._render_body(pre, B, R, S, H, W, dev, debug, inp)
        if fresh:
            ready = torch.cuda.Event()
            ready.record(main)
            for st in self._call_streams:                # every lane: the next call on the other lane skips its wait
                st.wait_event(ready)
        self._ws_prefix = f"c{self._call_idx}."
        with torch.cuda.stream(side):
            out = self._render_body(pre, B, R, S, H, W, dev, debug, inp)
            for t in _flat_tensors([v for k, v in out.items() if k not in ("host", "pixel_val_cpu", "uv_rows")]):
                if t.is_cuda:
                    t.record_stream(main)
            done = torch.cuda.Event()
            done.record(side)
        main.wait_event(done)
        return out

    def _render_body(self, pre, B, R, S, H, W, dev, debug, inp) -> Dict[str, torch.Tensor]:
        """The launches of one render call on the current stream; `pre` = what render() resolved from the caches."""
        w, maps, tabs, up, interval, uvc, uvs, fp = pre[:8]
        N = B * V
        s = _stream()

        f32, f16 = torch.float32, torch.float16
        # the geometry the call hands out is fresh memory, the rest of it workspace
        new = lambda name, shape, dt: torch.empty(shape, dtype=dt, device=dev) if name in ("coords9", "pixel_val", "pt") \
            else self._buf(name, shape, dt, dev)
        # the per-sample inputs of the two query MLPs once more in the UNIT order cpn_local_units multiplies in (one coalesced
        # line per unit instead of scattered reads of loc8 / coords9; include/coponerf_hip.h, cpn_sample_geometry)
        lvu = None
        if self.precision != "f32":
            had = self._ws.get(self._ws_prefix + "lvu")
            lvu = self._buf("lvu", (B * ((R + 3) // 4) * V * ((S + 3) // 4) * 64, 4), f32, dev)
            if self._ws[self._ws_prefix + "lvu"] is not had:
                # slots of rays / samples that do not exist (R or S no multiple of 4) are never written: whatever finite values
                # they hold feed MFMA columns of their own whose results are dropped - fresh memory is cleared once so that
                # nothing there is a NaN pattern either (a fill per call cost the callers' 18-call loop a launch per call)
                self._ws[self._ws_prefix + "lvu"].zero_()
        g = self._launch_geometry(new, up["cam"], uvc, uvs, interval, B, R, S, H, W, lvu)
        coords9, overlaps, pixel_val, pt = g["coords9"], g["overlaps"], g["pixel_val"], g["pt"]
        sec_grid, pe6, loc8 = g["sec_grid"], g["pe6"], g["loc8"]
        at_wt = torch.empty(N, R, S, dtype=f32, device=dev)

        # the caller contract wants pixel_val on the CPU (CoPoNeRF.py:490): start the 8*N*R*S-byte device->host copy
        # now, into pinned memory on a side stream, so it overlaps the GEMMs instead of stalling the step's tail
        pixel_val_cpu, copy_done = self._start_host_copy(pixel_val)

        nray_total = B * R
        zl = torch.empty(nray_total, 416, dtype=f32, device=dev)
        auto = self.precision == "auto"
        # precision="auto": every ray's guard score, written by the two cpn_logit_guard launches of its chunk
        score = self._buf("guard.score", (nray_total,), f32, dev) if auto else None
        C = min(self.chunk_rays if self.chunk_rays > 0 else self._auto_chunk(S, dev, nray_total), nray_total)
        T = V * S                       # rows per ray for the attention stage
        # one launch per attention round (cpn_attend_units) as far as a ray group's logits and weights fit the CU's LDS beside the
        # layer-2 weights; more samples per ray than that (S > 842) take the two kernels the launch is made of, which hand the
        # logits over through memory: same results, the only shapes cpn_attend_units rejects
        fused = T <= self.ATTEND_UNITS_MAX_T
        nchunks = (nray_total + C - 1) // C
        nlanes = min(self.lanes, nchunks)
        if nlanes > 1 and (len(self._lane_streams) < nlanes or self._lane_streams[0].device != dev):
            self._lane_streams = [torch.cuda.Stream(device=dev) for _ in range(nlanes)]
        main = torch.cuda.current_stream()

        def lane_buffers(lane):
            t = lambda name, shape, dt: self._buf(f"{name}.{lane}", shape, dt, dev)
            # kh in unit order: 16 rows per unit incl. the dead rows of partial units (at most one ray group more per batch
            # element and chunk edge)
            rows128 = ((C + 3) // 4 + B + 1) * V * ((S + 3) // 4) * 16
            # (lg: the raw logits in row order - the guard's input with precision = "auto", the hand-over of the two-kernel pair
            #  beyond what cpn_attend_units holds in LDS; otherwise the logits never leave the CU)
            return {"lg": t("lg", (C * T,), f32) if (auto or not fused) else None,
                    "z1": t("z1", (C, 416), f32), "ze": t("ze", (C, 128), f32), "addq": t("addq", (C, 128), f32),
                    "hbar": t("hbar", (C, 1664), f16), "zs": t("zs", (C, 416), f32),
                    "hid": t("hid", (C * T * 2, 832), f16), "khf": t("khf", (rows128, 128), f16)}

        def timed(name, flops, fn):
            """fn() between two events when bench.py asked for per-kernel times (self.profile)"""
            prof = self.profile
            if prof is None:
                return fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            prof.setdefault(name, []).append((e0, e1, flops))

        def value_fold(s, hbar, out, m):
            """the folded value projection of a round's summed hidden vector, per RAY (CoPoNeRF.py:404 after :387-397)"""
            if m <= self.FEW_ROWS:
                # a small call's per-ray GEMM: 30 of the 256-row tiles would walk K alone (37 us at 3 641 rays); bit-identical
                fn = lambda: call("cpn_gemm_f16_fewrows", hbar.data_ptr(), 1664, w["value_fold.wpk"].data_ptr(),
                                  w["value_fold.b"].data_ptr(), out.data_ptr(), 416, m, 416, 1664, 0, s)
            else:
                fn = lambda: call("cpn_gemm_f16", hbar.data_ptr(), 1664, w["value_fold.w16"].data_ptr(), 1664,
                                  w["value_fold.b"].data_ptr(), out.data_ptr(), 416, m, 416, 1664, 0, 1, s)
            timed("gemm_f16:value_fold", 2.0 * m * 416 * 1664, fn)

        # ---- the stages of one chunk, in serial order.  Every stage takes the chunk's first ray, its buffers and the raw stream.
        def run_chunk(ray0, bf, s):
            n = min(C, nray_total - ray0)
            rows2 = n * T * 2
            # E: first encoder layer + the folded key_map layer -> hid, kh (unit order)  [CoPoNeRF.py:384-397, 404-407]
            # (third profile entry: canonical FLOPs of the FIRST layer; bench.py adds the fused key layer's by kernel name)
            timed("encode_key", 2.0 * rows2 * 832 * 835, lambda: call(
                "cpn_encode_key", tabs[0].data_ptr(), maps[3].data_ptr(), H, W, pixel_val.data_ptr(), sec_grid.data_ptr(),
                pe6.data_ptr(), w["enc.frag"].data_ptr(), w["query_encode_latent.b"].data_ptr(), w["key_fold.wpk"].data_ptr(),
                w["key_fold.b"].data_ptr(), B, V, R, S, ray0, n, bf["hid"].data_ptr(), bf["khf"].data_ptr(), 1, s))
            # G A1: coords_embed (both query_embed layers), key_map_2 on kh, <key, coords_embed>, and behind them - in the SAME launch,
            #    for other rays of the chunk - the joint softmax over the 2 x S samples of a ray + the weighted hidden sum, round 1
            #    (cpn_attend_units; the logits reach the sum through LDS)  [:408, :446, :450-461]
            lg = bf["lg"].data_ptr() if (auto or not fused) else 0
            r1 = (0, loc8.data_ptr(), coords9.data_ptr(), w["query_embed.w"].data_ptr(), 16,
                  w["query_embed.b"].data_ptr(), 0, w["query_embed_2.w16"].data_ptr(), 128, w["query_embed_2.b"].data_ptr(),
                  w["key_map_2.w16"].data_ptr(), 128, w["key_map_2.b"].data_ptr(), 0, 0, 0, bf["khf"].data_ptr())
            if fused:
                timed("attend_units:round1", 2.0 * n * T * (128 * (128 + 128 + 16) + 1664), lambda: call(
                    "cpn_attend_units", *r1, bf["hid"].data_ptr(), B, V, R, S, ray0, n, lvu.data_ptr(),
                    bf["hbar"].data_ptr(), at_wt.data_ptr(), lg, s))
            else:
                timed("local_units:query_embed+key_map_2", 2.0 * n * T * 128 * (128 + 128 + 16), lambda: call(
                    "cpn_local_units", *r1, B, V, R, S, ray0, n, 0, lvu.data_ptr(), lg, s))
                timed("attend_hidden:round1", 2.0 * n * T * 1664, lambda: call(
                    "cpn_attend_hidden", 0, 0, lg, bf["hid"].data_ptr(), B, V, R, S, ray0, n,
                    bf["hbar"].data_ptr(), at_wt.data_ptr(), s))
            if auto:                    # guard score of round 1 (before round 2 overwrites lg)
                timed("logit_guard:round1", 0.0, lambda: call(
                    "cpn_logit_guard", lg, B, V, R, S, ray0, n, score.data_ptr(), 0, s))
            # V1 L M2 A2: value projection of the round-1 sum, encode_latent, the second query, its logits (coords_embed formed
            #    again from the local coordinates: mode 2) and round 2 of the attention  [:467-485]
            z1, ze, addq = bf["z1"], bf["ze"], bf["addq"]
            value_fold(s, bf["hbar"], z1, n)
            call("cpn_linear_f32", z1.data_ptr(), 416, w["encode_latent.w"].data_ptr(), 416,
                 w["encode_latent.b"].data_ptr(), 0, 0, ze.data_ptr(), 128, n, 128, 416, 0, 0, s)
            call("cpn_linear_f32", ze.data_ptr(), 128, w["query_repeat_embed.w_z"].data_ptr(), 128, 0, 0, 0,
                 addq.data_ptr(), 128, n, 128, 128, 0, 0, s)
            r2 = (2, loc8.data_ptr(), coords9.data_ptr(), w["query_repeat_embed.w_l"].data_ptr(), 16,
                  w["query_repeat_embed.b"].data_ptr(), addq.data_ptr(), w["query_repeat_embed_2.w16"].data_ptr(), 128,
                  w["query_repeat_embed_2.b"].data_ptr(), w["query_embed_2.w16"].data_ptr(), 128, w["query_embed_2.b"].data_ptr(),
                  w["query_embed.w"].data_ptr(), 16, w["query_embed.b"].data_ptr(), 0)
            if fused:
                timed("attend_units:round2", 2.0 * n * T * (128 * (2 * 128 + 2 * 16) + 1664), lambda: call(
                    "cpn_attend_units", *r2, bf["hid"].data_ptr(), B, V, R, S, ray0, n, lvu.data_ptr(),
                    bf["hbar"].data_ptr(), 0, lg, s))
            else:
                timed("local_units:round2+query_embed", 2.0 * n * T * 128 * (2 * 128 + 2 * 16), lambda: call(
                    "cpn_local_units", *r2, B, V, R, S, ray0, n, 0, lvu.data_ptr(), lg, s))
                timed("attend_hidden:round2", 2.0 * n * T * 1664, lambda: call(
                    "cpn_attend_hidden", 0, 0, lg, bf["hid"].data_ptr(), B, V, R, S, ray0, n,
                    bf["hbar"].data_ptr(), 0, s))
            if auto:                    # ... max'ed with round 2's
                timed("logit_guard:round2", 0.0, lambda: call(
                    "cpn_logit_guard", lg, B, V, R, S, ray0, n, score.data_ptr(), 1, s))
            # V2: value projection of the round-2 sum; the round-1 vector sits in both view slots when the views are summed
            #    (CoPoNeRF.py:481-485)
            value_fold(s, bf["hbar"], bf["zs"], n)
            torch.add(bf["zs"][:n], z1[:n], alpha=float(V), out=zl[ray0:ray0 + n])

        dims = (B, R, S, H, W)
        f32_inputs = lambda: self._f32_inputs(pre[8], w, H, W)
        if self.precision == "f32":
            render_f32.per_sample(*f32_inputs(), g, zl, at_wt, dims, self.f32_chunk_rays, self._buf, s)
        elif nlanes == 1:
            bf = lane_buffers(0)
            for ray0 in range(0, nray_total, C):
                run_chunk(ray0, bf, s)
        else:
            ready = torch.cuda.Event()
            ready.record()                              # geometry, weights, maps and zl are queued on the main stream
            for ci, ray0 in enumerate(range(0, nray_total, C)):
                lane = ci % nlanes
                st = self._lane_streams[lane]
                if ci < nlanes:
                    st.wait_event(ready)
                with torch.cuda.stream(st):
                    run_chunk(ray0, lane_buffers(lane), st.cuda_stream)
            for lane in range(nlanes):
                done = torch.cuda.Event()
                done.record(self._lane_streams[lane])
                main.wait_event(done)
        if auto:
            # list the rays whose guard score exceeds auto_threshold (cpn_select_rays), read their count - the mode's ONE host
            # wait per call - and render those rays again in the reference's arithmetic before the decoder runs
            lst = self._buf("guard.list", (nray_total,), torch.int32, dev)
            cnt = self._buf("guard.count", (1,), torch.int32, dev)
            call("cpn_select_rays", score.data_ptr(), nray_total, float(self.auto_threshold), lst.data_ptr(), cnt.data_ptr(), s)
            if self._guard_host is None:
                self._guard_host = torch.empty(1, dtype=torch.int32, pin_memory=True)
            self._guard_host.copy_(cnt, non_blocking=True)
            copied = torch.cuda.Event()
            copied.record()
            copied.synchronize()
            k = int(self._guard_host[0])
            self.last_exact_rays = (k, nray_total)
            if k > 0:
                render_f32.per_sample(*f32_inputs(), g, zl, at_wt, dims, self.f32_chunk_rays, self._buf, s, rays=lst, nsel=k)

        # ---- light-field decoder phi over all rays (lightfield.py:131-167) + white background, exact fp32, one launch
        rgb = torch.empty(B, 1, R, 3, dtype=f32, device=dev)
        valid = torch.empty(B, R, 1, dtype=f32, device=dev)
        rgb_raw = torch.empty(nray_total, 3, dtype=f32, device=dev) if debug else None
        call("cpn_lightfield_decode", coords9.data_ptr(), zl.data_ptr(), w["phi.pack"].data_ptr(), overlaps.data_ptr(),
             B, V, R, rgb.data_ptr(), valid.data_ptr(), _ptr(rgb_raw), s)
        if self.lazy_pixel_val:
            pixel_val_cpu = PendingHostTensor.wrap(pixel_val_cpu, copy_done, pixel_val)
        else:
            copy_done.synchronize()
        out = {"rgb": rgb, "valid_mask": valid, "pixel_val": pixel_val, "pixel_val_cpu": pixel_val_cpu, "pt": pt, "at_wt": at_wt, "coords": coords9, "z_local": zl, "Tq": up["Tq"],
               "host": up, "uv_rows": (uvc, uvs)}
        if fp is not None:
            from .aux_outputs import ray_outputs
            out["aux"] = ray_outputs(inp, fp, at_wt, pt, up["rayc"], (uvc, uvs))
        if debug:
            out["sec_grid"], out["rgb_raw"] = sec_grid.clone(), rgb_raw
            if auto:
                out["guard_score"] = score.view(B, R).clone()
        return out
