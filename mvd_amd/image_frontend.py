"""Device image front end of the data loader: the alpha composite on white, PIL's LANCZOS resize and the
``/ 127.5 - 1.0`` normalisation that the reference's dataset and ``utils.load_image`` run with PIL on the host, as one call of
``mvd_op_image_frontend`` (csrc/imageio.hip).  The bytes equal PIL's and the floats equal the CPU's, bit for bit; only the decode
of the file stays on the host.  There is no fallback: a CPU tensor is an error.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import MvdError


def spans() -> dict:
    """the workgroup tiles of the two kernels: output columns x source rows of the horizontal one, output columns x output rows of
    the vertical one (tests plant values on both sides of every boundary)"""
    v = (C.c_int * 4)()
    _lib.call("mvd_op_image_frontend_spans", v)
    return {"h_cols": v[0], "h_rows": v[1], "v_cols": v[2], "v_rows": v[3]}


def workspace_bytes(batch: int, h: int, w: int, channels: int, out_h: int, out_w: int) -> int:
    need = _lib.lib().mvd_op_image_frontend_workspace_bytes(batch, h, w, channels, out_h, out_w)
    if need < 0:
        raise MvdError(f"mvd_op_image_frontend_workspace_bytes: {_lib.last_error()}")
    return need


_workspaces: dict = {}     # (device, stream) -> uint8 buffer, grown on demand: calls on one stream are ordered, two streams never share one


def _workspace(device: torch.device, need: int) -> torch.Tensor:
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < need:
        _workspaces[key] = None
        ws = _workspaces[key] = torch.empty(need, dtype=torch.uint8, device=device)
    return ws


def composite_resize(images_u8: torch.Tensor, size, out: str = "float"):
    """``images_u8``: (B, h, w, 3 | 4) or (h, w, 3 | 4) uint8 on the device -- ``np.array(Image.open(...))``'s layout.  ``size`` is
    PIL's (width, height).  ``out``: "float" -> (B, 3, H, W) fp32 in [-1, 1]; "uint8" -> (B, H, W, 3) uint8, PIL's bytes; "both" ->
    (float, uint8).  Runs on the current stream and does not synchronise; the workspace is per (device, stream), so streams do not
    share one (two host threads on ONE stream must serialise their calls themselves).  Limit: a horizontal downscale above about 9
    (1024 wide to under 108) is refused with ``MvdError`` -- the source span of one workgroup no longer fits its LDS rows; resize
    such images on the host (``utils.load_image``, ``ObjaverseDataset(frontend="host")``)."""
    if out not in ("float", "uint8", "both"):
        raise MvdError(f"composite_resize: out={out!r} (\"float\", \"uint8\" or \"both\")")
    if not isinstance(images_u8, torch.Tensor) or images_u8.dtype != torch.uint8:
        raise MvdError("composite_resize: images_u8 must be a uint8 tensor")
    if not images_u8.is_cuda:
        raise MvdError("composite_resize: images_u8 is a CPU tensor; the front end runs on the device only (no host fallback)")
    x = images_u8.unsqueeze(0) if images_u8.dim() == 3 else images_u8
    if x.dim() != 4 or x.shape[-1] not in (3, 4):
        raise MvdError(f"composite_resize: expected (B, h, w, 3 | 4), got {tuple(images_u8.shape)}")
    x = x.contiguous()
    B, h, w, ch = x.shape
    ow, oh = int(size[0]), int(size[1])
    ws = _workspace(x.device, workspace_bytes(B, h, w, ch, oh, ow))
    f = torch.empty((B, 3, oh, ow), dtype=torch.float32, device=x.device) if out != "uint8" else None
    u = torch.empty((B, oh, ow, 3), dtype=torch.uint8, device=x.device) if out != "float" else None
    with torch.cuda.device(x.device):
        _lib.call("mvd_op_image_frontend", C.c_void_p(x.data_ptr()), B, h, w, ch, oh, ow, C.c_void_p(u.data_ptr() if u is not None else None),
                  C.c_void_p(f.data_ptr() if f is not None else None), C.c_void_p(ws.data_ptr()), ws.numel(), _lib.stream())
    return f if out == "float" else u if out == "uint8" else (f, u)


def decode_image(source):
    """a path or file object -> (h, w, 3 | 4) uint8 numpy array on the host; modes other than RGB / RGBA are converted to RGB by PIL
    first (what ``convert("RGB")`` does to them in the host path)"""
    try:
        from PIL import Image
    except ImportError as e:
        raise MvdError("decoding an image needs the 'Pillow' package (PIL), which is not installed") from e
    import numpy as np
    im = Image.open(source)
    if im.mode not in ("RGB", "RGBA"):
        im = im.convert("RGB")
    return np.array(im)


def load_image_device(path, target_size=(768, 768), device="cuda") -> torch.Tensor:
    """``utils.load_image`` with only the decode on the host: (1, 3, H, W) float32 in [-1, 1] on ``device``, the same values
    (``composite_resize``'s limit on the horizontal downscale applies; ``utils.load_image`` has none)"""
    device = torch.device(device)
    if device.type != "cuda":
        raise MvdError(f"load_image_device: device {device} is not a GPU; use utils.load_image on the host")
    raw = torch.from_numpy(decode_image(path)).to(device)
    return composite_resize(raw, target_size, out="float")
