"""Python handle on the C-ABI engine (include/mvd_hip.h).  torch is used only for device
memory, streams and the one-time weight packing; every FLOP of the forward runs in
libmvd_hip.so.  There is no CPU path: constructing an engine without a GPU raises."""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional

import torch

from . import _lib as L
from .config import UNetConfig
from .layout import ViewLayout
from .main_options import TODO_METHODS, MainOptions, check_todo
from .packing import pack_camera, pack_unet


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


class MVDEngine:
    def __init__(self, cfg: UNetConfig, cam_output_dim: int = 1024, cam_hidden_dim: int = 512,
                 simple_cam_encoder: bool = False, cam_modulation_strength: float = 0.2, device="cuda:0",
                 small_batch_twins: Optional[bool] = None, fold_tail: bool = True):
        if not torch.cuda.is_available():
            raise L.MvdError("MVDEngine needs a MI355X (torch.cuda.is_available() is False); there is no CPU fallback")
        self.cfg = cfg
        self.device = torch.device(device)
        # second packed copies only a batch-1 forward reads (packing.pack_unet): on unless MVD_PACK_SMALL_BATCH_TWINS=0
        self.small_batch_twins = (os.environ.get("MVD_PACK_SMALL_BATCH_TWINS", "1") != "0") if small_batch_twins is None \
            else bool(small_batch_twins)
        # ff.net.2 and proj_out of every transformer block packed as one K-concatenated GEMM (packing.compose_tail); False packs the
        # two separate layers and the engine runs two launches (the A/B switch: the route follows the registered slots)
        self.fold_tail = bool(fold_tail)
        c = L.mvd_config_t()
        c.in_channels, c.out_channels, c.num_levels = cfg.in_channels, cfg.out_channels, cfg.num_levels
        for i in range(cfg.num_levels):
            c.block_out_channels[i] = cfg.block_out_channels[i]
            c.num_heads[i] = cfg.num_heads[i]
        c.layers_per_block, c.cross_attention_dim = cfg.layers_per_block, cfg.cross_attention_dim
        c.norm_num_groups, c.norm_eps = cfg.norm_num_groups, cfg.norm_eps
        c.cam_output_dim, c.cam_hidden_dim = cam_output_dim, cam_hidden_dim
        c.simple_cam_encoder, c.cam_modulation_strength = int(simple_cam_encoder), cam_modulation_strength
        self.cam_output_dim = cam_output_dim
        h = C.c_void_p()
        L.call("mvd_engine_create", C.byref(c), C.byref(h))
        self._h = h
        self._weights: List[Dict[str, torch.Tensor]] = [{}, {}]   # keeps packed tensors alive
        self._arenas: Dict[torch.dtype, torch.Tensor] = {}        # one flat buffer per dtype once consolidated
        self._arenas_stale = True
        self._ws = None
        self._rc = None
        self._ws_key = None
        self._ws_resize = False
        self._ws_args = None
        self.options = MainOptions()                              # what the set_* / clear_* methods below have set the main pass to
        self._dc = None                                           # the bound buffer of the stored deep feature

    # what callers and tests read off an engine: views of ``options``, which is the only state
    freeu, tome = property(lambda self: self.options.freeu), property(lambda self: self.options.tome)
    todo, deepcache = property(lambda self: self.options.todo), property(lambda self: self.options.deepcache)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                L.lib().mvd_engine_destroy(self._h)
                self._h = None
        except Exception:
            pass

    # ------------------------------------------------------------------ weights
    def _register(self, set_id: int, packed: Dict[str, torch.Tensor]):
        for slot, t in packed.items():
            assert t.is_cuda and t.is_contiguous()
            L.call("mvd_engine_set_weight", self._h, set_id, slot.encode(), _ptr(t), t.numel(), L.dtype_code(t))
        self._weights[set_id].update(packed)
        self._arenas_stale = True

    def load_base(self, sd: Dict[str, torch.Tensor], adapter: bool, ref_scale: float):
        """``sd``: diffusers keys of base_unet (+ ``...processor.*`` adapter keys when ``adapter``)."""
        with torch.no_grad():
            self._register(0, pack_unet(sd, self.cfg, self.device, adapter, ref_scale, self.small_batch_twins, self.fold_tail))

    def load_camera(self, sd: Dict[str, torch.Tensor]):
        with torch.no_grad():
            self._register(0, pack_camera(sd, self.device, len(self.cfg.block_out_channels)))

    def load_image_encoder(self, sd: Dict[str, torch.Tensor]):
        with torch.no_grad():
            self._register(1, pack_unet(sd, self.cfg, self.device, False, 0.0, self.small_batch_twins, self.fold_tail))
        self.share_encoder_weights(False)

    def share_encoder_weights(self, enable: bool = True):
        """N4 (training.py:60-65): the image encoder's UNet equals the frozen base UNet -> the encoder pass reads weight
        set 0 and the second packed weight set (1.73 GB bf16) is dropped."""
        L.call("mvd_engine_share_encoder_weights", self._h, int(enable))
        if enable:
            L.call("mvd_engine_clear_weights", self._h, 1)
            self._weights[1] = {}
            self._arenas_stale = True

    def consolidate_weights(self):
        """Re-home every registered weight (both sets) in ONE flat device buffer per dtype and re-register the slots
        (same contents, 256-byte aligned views).  Makes the multi-GPU start-up broadcast a few large in-place
        transfers (mvd_amd/distributed.py) and the weights one contiguous HBM region."""
        if self._arenas and not self._arenas_stale:
            return
        from .distributed import pack_into_arenas
        flat = {f"{i}/{k}": t for i, d in enumerate(self._weights) for k, t in d.items()}
        if not flat:
            return
        self._arenas, views = pack_into_arenas(flat)
        for name, v in views.items():
            i, k = name.split("/", 1)
            self._weights[int(i)][k] = v
        for i, d in enumerate(self._weights):
            for slot, t in d.items():
                L.call("mvd_engine_set_weight", self._h, i, slot.encode(), _ptr(t), t.numel(), L.dtype_code(t))
        self._arenas_stale = False

    def weight_bytes(self) -> int:
        return sum(t.numel() * t.element_size() for d in self._weights for t in d.values())

    # ------------------------------------------------------------------ workspace
    def _ensure_workspace(self, batch, h, w, text_len, ref_batch, keep_features, lay=ViewLayout()):
        key = (batch, h, w, text_len, ref_batch, keep_features) + (() if lay.views else (0,)) + lay.key()
        if self._ws_key == key and not self._ws_resize:
            return
        # (FreeU was set since the workspace was sized: the same shape may need more.  Buffers that are large enough stay bound as
        #  they are -- re-binding would drop the cached reference, which does not depend on the setting)
        keep_bound = self._ws_key == key
        self._ws_args = (batch, h, w, text_len, ref_batch, keep_features, lay)
        if lay.rows:
            # a shared-reference forward (MVD_SHARE_REF) is sized from its argument block: the positional entry describes
            # an ordinary forward, whose Q4 re-chunking fails when the views do not divide the reference tokens
            a = L.mvd_forward_args_t()
            a.batch, a.height, a.width, a.text_len, a.ref_batch, a.views = batch, h, w, text_len, ref_batch, lay.views
            a.cam_rows, a.cam_batch = 4, lay.rows
            a.flags = L.MVD_USE_CAMERA | L.MVD_USE_IMAGE | L.MVD_SHARE_REF
            suffix, beside = self._entry(lay)
            ws = getattr(L.lib(), "mvd_engine_workspace_bytes" + (suffix or "_args"))(self._h, C.byref(a), *beside)
        else:
            ws = L.lib().mvd_engine_workspace_bytes(self._h, batch, h, w, text_len, ref_batch)
        if ws < 0:
            raise L.MvdError(f"workspace_bytes: {L.last_error()}")
        rc = 0
        if ref_batch > 0:
            rc = L.lib().mvd_engine_refcache_bytes(self._h, ref_batch, h, w, int(keep_features))
            if rc < 0:
                raise L.MvdError(f"refcache_bytes: {L.last_error()}")
        self._ws_resize = False
        if keep_bound and self._ws is not None and self._ws.numel() >= ws:
            return
        if self._ws is None or self._ws.numel() < ws:
            self._ws = None
            self._ws = torch.empty(ws, dtype=torch.uint8, device=self.device)
        if rc and (self._rc is None or self._rc.numel() < rc):
            self._rc = None
            self._rc = torch.empty(rc, dtype=torch.uint8, device=self.device)
        L.call("mvd_engine_bind_workspace", self._h, _ptr(self._ws), self._ws.numel(),
               _ptr(self._rc) if rc else None, self._rc.numel() if rc else 0)
        self._ws_key = key
        self._ref_valid = None      # re-binding drops the engine's cached reference K/V

    # ------------------------------------------------------------------ forward
    def forward(self, sample: torch.Tensor, timesteps: torch.Tensor, text: torch.Tensor,
                source_camera: Optional[torch.Tensor] = None, target_camera: Optional[torch.Tensor] = None,
                fourier_proj: Optional[torch.Tensor] = None, source_latents: Optional[torch.Tensor] = None,
                encoder_text: Optional[torch.Tensor] = None, reuse_ref: bool = False,
                keep_features: bool = False, out: Optional[torch.Tensor] = None, *, views: Optional[int] = None,
                objects: Optional[int] = None, deep_cache: Optional[str] = None) -> torch.Tensor:
        """All tensors fp32 contiguous on ``self.device``; returns fp32 NCHW.  ``views`` (an int >= 1): the shared-reference
        forward (``MVD_SHARE_REF``, include/mvd_hip.h) -- ``sample`` holds g * views rows ``[uncond x views | cond x views]``,
        ``text`` g rows, ``source_latents`` / ``encoder_text`` one row, the cameras 1 or ``views`` rows.  ``objects`` (O > 1, with
        ``views``; ``mvd_unet_forward_objects``): O objects x ``views`` views -- ``sample`` holds g * O * views rows, object-major
        inside a guidance half, ``text`` g * O rows, ``source_latents`` / ``encoder_text`` O rows, the cameras 1 or O * views rows;
        ``None`` / 1: the forward without it.  ``views`` a SEQUENCE ``(V_0, .., V_{O-1})`` (``mvd_unet_forward_ragged``): O objects
        with V_o >= 1 views each, R = sum of the counts -- ``sample`` holds g * R rows, object-major inside a guidance half, the
        cameras 1 or R rows, everything else as with ``objects = O`` (which ``objects`` must be, or ``None``).

        ``deep_cache`` (DeepCache, after ``set_deepcache``): ``"refresh"`` -- this forward, which also stores its deep feature
        (``MVD_DEEPCACHE_REFRESH``); ``"reuse"`` -- the shallow forward around the stored feature (``MVD_DEEPCACHE_SHALLOW``; with
        image conditioning it needs ``reuse_ref``); ``None``: neither."""
        if deep_cache not in (None, "refresh", "reuse"):
            raise L.MvdError(f"engine.forward: deep_cache={deep_cache!r}: expected None, 'refresh' or 'reuse'")
        B, Cin, H, W = sample.shape
        Lt = text.shape[1]
        for t in (sample, timesteps, text, source_camera, target_camera, fourier_proj, source_latents, encoder_text):
            if t is not None:
                if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                    raise L.MvdError("engine.forward expects contiguous fp32 CUDA tensors")
        lay = ViewLayout.parse(views, objects, "engine")
        views, objects, counts = lay
        if counts and lay.g(B) not in (1, 2):
            raise L.MvdError(f"engine.forward: batch {B} is not 1 or 2 rows for each of the {lay.rows} views of {counts}")
        if views and B % views:
            raise L.MvdError(f"engine.forward: batch {B} is not a multiple of views {views}")
        if text.shape[0] != lay.text_rows(B) or timesteps.shape != (B,):
            raise L.MvdError(f"engine.forward: text batch {text.shape[0]} / timesteps {tuple(timesteps.shape)} vs batch {B}"
                             + (f" in {views} views" if views else "") + (f" in views {counts}" if counts else ""))
        use_cam = target_camera is not None
        use_img = source_latents is not None or reuse_ref
        ref_batch = 0
        if use_img:
            ref_batch = source_latents.shape[0] if source_latents is not None else self._last_ref_batch
            self._last_ref_batch = ref_batch
        if lay.rows and not use_img:
            raise L.MvdError("engine.forward: views needs image conditioning (source_latents or reuse_ref)")
        if counts and ref_batch != len(counts):
            raise L.MvdError(f"engine.forward: views {counts} need {len(counts)} reference rows (one per object), got {ref_batch}")
        if objects and (ref_batch != objects or B % (objects * views)):
            raise L.MvdError(f"engine.forward: {objects} objects x {views} views need a multiple of {objects * views} sample rows and "
                             f"{objects} reference rows, got {B} and {ref_batch}")
        self._ensure_workspace(B, H, W, Lt, ref_batch, keep_features, lay)
        if deep_cache == "refresh":
            # (a shallow forward reads the buffer its refresh forward bound: growing it here would throw the stored feature away)
            self._ensure_deepcache(B, H, W)
        graph = getattr(self, "_graph", False)
        user_out = out
        if graph:
            # hipGraph replay needs the SAME device buffers every call: stage the inputs into persistent buffers (tiny
            # device-to-device copies on the caller's stream) and run on the engine's own stream (captures are illegal on the
            # legacy default stream); mvd_engine_set_graph in include/mvd_hip.h
            stage = lambda name, t: None if t is None else self._staged(name, t)   # noqa: E731
            sample, timesteps, text = stage("sample", sample), stage("timesteps", timesteps), stage("text", text)
            source_camera, target_camera = stage("src_cam", source_camera), stage("tgt_cam", target_camera)
            fourier_proj, source_latents = stage("proj", fourier_proj), stage("lat", source_latents)
            encoder_text = stage("enc_text", encoder_text)
            out = self._staged("out", torch.empty(0), shape=(B, self.cfg.out_channels, H, W))
        elif out is None:
            out = torch.empty(B, self.cfg.out_channels, H, W, dtype=torch.float32, device=self.device)
        a = L.mvd_forward_args_t()
        a.batch, a.height, a.width, a.text_len = B, H, W, Lt
        a.sample, a.timesteps, a.text = sample.data_ptr(), timesteps.data_ptr(), text.data_ptr()
        flags = 0
        if use_cam:
            if source_camera is None or fourier_proj is None:
                raise L.MvdError("camera conditioning needs source_camera, target_camera and fourier_proj")
            Bc = target_camera.shape[0]
            if source_camera.shape[0] != Bc or Bc < 1 or Bc > B or B % Bc:
                raise L.MvdError(f"camera batch {tuple(source_camera.shape)} / {tuple(target_camera.shape)} must be equal "
                                 f"and divide the sample batch {B}")
            a.source_camera, a.target_camera = source_camera.data_ptr(), target_camera.data_ptr()
            a.cam_rows = source_camera.shape[1]
            a.cam_batch = Bc        # Bc < B: the FiLM scale/shift broadcast over the sample rows (CFG, pipeline.py:141-152)
            a.fourier_proj = fourier_proj.data_ptr()
            flags |= L.MVD_USE_CAMERA
        if use_img:
            flags |= L.MVD_USE_IMAGE
            if reuse_ref:
                flags |= L.MVD_REUSE_REF
            else:
                if encoder_text is None or encoder_text.shape[0] != ref_batch:
                    raise L.MvdError("image conditioning needs encoder_text with the reference batch")
                a.source_latents, a.encoder_text = source_latents.data_ptr(), encoder_text.data_ptr()
            if keep_features:
                flags |= L.MVD_KEEP_FEATURES
        if lay.rows:
            flags |= L.MVD_SHARE_REF
            a.views = views                 # (0 with counts: they travel beside the argument block, like the object count)
        if deep_cache is not None:
            flags |= L.MVD_DEEPCACHE_REFRESH if deep_cache == "refresh" else L.MVD_DEEPCACHE_SHALLOW
        a.ref_batch, a.flags = ref_batch, flags
        a.out = out.data_ptr()
        suffix, beside = self._entry(lay)
        entry = ("mvd_unet_forward" + suffix, self._h, C.byref(a), *beside)
        if graph:
            cur = torch.cuda.current_stream(self.device)
            self._gstream.wait_stream(cur)
            with torch.cuda.stream(self._gstream):
                L.call(*entry, L.stream())
            cur.wait_stream(self._gstream)
            out = out.clone() if user_out is None else user_out.copy_(out)
        else:
            L.call(*entry, L.stream())
        if use_img and not reuse_ref:
            self._ref_valid = (B, H, W, Lt, ref_batch) + lay.key()
        return out

    # ------------------------------------------------------------------ reference pass in two halves (global Q2 statistics)
    def reference_encode(self, source_latents: torch.Tensor, encoder_text: torch.Tensor, main_batch: int) -> torch.Tensor:
        """First half (``mvd_engine_reference_encode``): the image-encoder pass on ``source_latents``; the raw features stay in
        the engine, the LOCAL per-pixel statistics come back as ``[pixels][3]`` fp32 rows (n, mean, M2) with n = ref_batch * C
        of the pixel's feature -- what ``distributed.merge_reference_stats`` exchanges.  ``main_batch`` is the batch of the
        forwards that will follow (the workspace is bound once for both)."""
        for t in (source_latents, encoder_text):
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                raise L.MvdError("engine.reference_encode expects contiguous fp32 CUDA tensors")
        Br, _, H, W = source_latents.shape
        Lt = encoder_text.shape[1]
        if encoder_text.shape[0] != Br:
            raise L.MvdError("image conditioning needs encoder_text with the reference batch")
        self._last_ref_batch = Br
        self._ensure_workspace(main_batch, H, W, Lt, Br, True)
        npix = L.lib().mvd_engine_reference_pixels(self._h, H, W)
        stats = torch.empty(npix, 2, dtype=torch.float32, device=self.device)
        a = L.mvd_forward_args_t()
        a.batch, a.height, a.width, a.text_len = main_batch, H, W, Lt
        a.source_latents, a.encoder_text = source_latents.data_ptr(), encoder_text.data_ptr()
        a.ref_batch, a.flags = Br, L.MVD_USE_IMAGE
        L.call("mvd_engine_reference_encode", self._h, C.byref(a), _ptr(stats), L.stream())
        self._ref_valid = None
        self._ref_pending = (main_batch, H, W, Lt, Br)
        n = torch.empty(npix, dtype=torch.float32, device=self.device)
        off = 0
        c_, h_, w_ = C.c_int(), C.c_int(), C.c_int()
        for i in range(L.lib().mvd_engine_num_features(self._h)):
            L.call("mvd_engine_feature_shape", self._h, i, C.byref(c_), C.byref(h_), C.byref(w_))
            n[off:off + h_.value * w_.value] = float(Br * c_.value)
            off += h_.value * w_.value
        return torch.cat([n[:, None], stats], dim=1)

    def reference_finish(self, mean_k: torch.Tensor) -> None:
        """Second half (``mvd_engine_reference_finish``): ``mean_k`` = ``[pixels][2]`` fp32 (mean, 0.5 / max(std, 1e-6)) after the
        merge.  Afterwards ``forward(..., reuse_ref=True, keep_features=True)`` runs on this reference."""
        pend = getattr(self, "_ref_pending", None)
        if pend is None:
            raise L.MvdError("reference_finish without a pending reference_encode")
        npix = L.lib().mvd_engine_reference_pixels(self._h, pend[1], pend[2])
        if not (mean_k.is_cuda and mean_k.dtype == torch.float32 and mean_k.is_contiguous() and tuple(mean_k.shape) == (npix, 2)):
            raise L.MvdError(f"reference_finish expects a contiguous fp32 CUDA tensor [{npix}, 2]")
        L.call("mvd_engine_reference_finish", self._h, _ptr(mean_k), L.stream())
        self._ref_pending = None
        self._ref_valid = pend

    def set_graph(self, enable: bool) -> None:
        """Replay repeated forwards (same shapes / flags) as one hipGraphLaunch each (``mvd_engine_set_graph``)."""
        L.call("mvd_engine_set_graph", self._h, int(bool(enable)))
        self._graph = bool(enable)
        if enable and getattr(self, "_gstream", None) is None:
            self._gstream = torch.cuda.Stream(device=self.device)
            self._gbufs = {}

    def set_freeu(self, s1: float, s2: float, b1: float, b2: float) -> None:
        """FreeU on the main UNet pass (``mvd_engine_set_freeu``; diffusers' ``enable_freeu`` argument order): up block 0 scales
        the lower half of its backbone channels by ``b1`` and the lowest spatial frequencies of its skip maps by ``s1``, up block 1
        by ``b2`` / ``s2``.  The encoder pass and the cached reference do not depend on it."""
        L.call("mvd_engine_set_freeu", self._h, float(s1), float(s2), float(b1), float(b2))
        self._options_changed(freeu=(s1, s2, b1, b2))

    def clear_freeu(self) -> None:
        """Back to the forward without FreeU (``mvd_engine_clear_freeu``): the launches it made before."""
        L.call("mvd_engine_clear_freeu", self._h)
        self._options_changed(freeu=None)

    def _options_changed(self, **fields) -> None:
        """The tail of the setters whose option moves the workspace's size: the same shape may now need more (or, token merging
        cleared, more than while it was on)."""
        self.options = self.options._replace(**fields)
        self._ws_resize = True
        if self._ws_key is not None and self._ws_args is not None:
            # now, not in the next forward: whoever asks reference_cache_valid first gets the answer that holds
            self._ensure_workspace(*self._ws_args)

    def set_tome(self, ratio: float = 0.5, max_downsample: int = 1, keep_tables: bool = False) -> None:
        """Token merging in front of self-attention on the main UNet pass (``mvd_engine_set_tome``; tomesd's ``apply_patch`` names):
        blocks whose map is at most ``max_downsample`` times coarser than the latent run ``attn1`` on ``N - int(N * ratio)`` rows.
        ``keep_tables``: ``tome_tables()`` reads the blocks' slot tables after a forward (test plumbing)."""
        L.call("mvd_engine_set_tome", self._h, float(ratio), int(max_downsample), int(bool(keep_tables)))
        self._options_changed(tome=(ratio, max_downsample), tome_keep=keep_tables)

    def clear_tome(self) -> None:
        """Back to the forward without token merging (``mvd_engine_clear_tome``): the launches it made before."""
        L.call("mvd_engine_clear_tome", self._h)
        self._options_changed(tome=None)

    def tome_tables(self):
        """``{feature name: slot table (batch, H*W) int32}`` of the blocks that merged in the last issued forward (needs
        ``set_tome(..., keep_tables=True)``)."""
        out = {}
        for i, (_, name, _, _) in enumerate(self.cfg.transformers()):
            n = L.lib().mvd_engine_tome_table(self._h, i, None, None)
            if n < 0:
                raise L.MvdError(f"tome_table: {L.last_error()}")
            if n:
                t = torch.empty(n, dtype=torch.int32, device=self.device)
                if L.lib().mvd_engine_tome_table(self._h, i, _ptr(t), C.c_void_p(torch.cuda.current_stream().cuda_stream)) != n:
                    raise L.MvdError(f"tome_table: {L.last_error()}")
                out[name] = t
        return out

    def set_todo(self, factor: int = 2, factor_level_2: int = 1, method: str = "nearest") -> None:
        """Token downsampling of the self-attention keys and values on the main UNet pass (``mvd_engine_set_todo``): blocks at the
        latent's own resolution pool K/V by ``factor``, blocks one level below by ``factor_level_2`` (1: untouched); ``method`` is
        ``"nearest"`` or ``"area"``.  Refused while token merging is set."""
        factor, factor_level_2, method = check_todo(factor, factor_level_2, method)
        L.call("mvd_engine_set_todo", self._h, factor, factor_level_2, TODO_METHODS.index(method))
        self._options_changed(todo=(factor, factor_level_2, method))

    def clear_todo(self) -> None:
        """Back to the forward without token downsampling (``mvd_engine_clear_todo``): the launches it made before."""
        L.call("mvd_engine_clear_todo", self._h)
        self._options_changed(todo=None)

    def todo_keys(self) -> Dict[str, int]:
        """``{feature name: Nk}`` of the blocks whose self-attention ran on downsampled keys in the last issued forward."""
        names = [name for _, name, _, _ in self.cfg.transformers()]
        out = (C.c_int * len(names))()
        if L.lib().mvd_engine_todo_keys(self._h, out, len(names)) < 0:
            raise L.MvdError(f"todo_keys: {L.last_error()}")
        return {name: int(nk) for name, nk in zip(names, out) if nk}

    def set_taps(self, enable: bool = True) -> None:
        """Main-pass taps (``mvd_engine_set_taps``; test plumbing): with them on, ``taps()`` reads every block output of the last
        forward's main pass.  The forward's output does not depend on the switch; its workspace may grow."""
        L.call("mvd_engine_set_taps", self._h, int(bool(enable)))
        self._options_changed(taps=enable)

    def taps(self) -> Dict[str, torch.Tensor]:
        """``{name: (B, C, H, W) fp32}`` of the block outputs of the last issued forward's main pass, in execution order (the names:
        include/mvd_hip.h; needs ``set_taps()``)."""
        n = L.lib().mvd_engine_num_taps(self._h)
        if n < 0:
            raise L.MvdError(f"num_taps: {L.last_error()}")
        out = {}
        name = C.create_string_buffer(128)
        b, c, h, w = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        for i in range(n):
            L.call("mvd_engine_tap_info", self._h, i, name, len(name), C.byref(b), C.byref(c), C.byref(h), C.byref(w))
            t = torch.empty(b.value, c.value, h.value, w.value, dtype=torch.float32, device=self.device)
            L.call("mvd_engine_get_tap", self._h, i, _ptr(t), L.stream())
            out[name.value.decode()] = t
        return out

    def set_deepcache(self, branch: int = 0) -> None:
        """DeepCache on the main UNet pass (``mvd_engine_set_deepcache``): ``forward(..., deep_cache="refresh")`` stores the hidden
        input of ``up_blocks.{n-1}.resnets.{Lb-1-branch}``, ``deep_cache="reuse"`` runs only ``down_blocks.0`` layers ``0..branch``
        and the last ``branch + 2`` layers of the last up block around it.  Setting invalidates a stored feature."""
        L.call("mvd_engine_set_deepcache", self._h, int(branch))
        self.options = self.options._replace(deepcache=branch)

    def clear_deepcache(self) -> None:
        """Back to the engine without DeepCache (``mvd_engine_clear_deepcache``); the buffer is released."""
        L.call("mvd_engine_clear_deepcache", self._h)
        L.call("mvd_engine_bind_deepcache", self._h, None, 0)
        self.options, self._dc = self.options._replace(deepcache=None), None

    def _ensure_deepcache(self, batch, h, w):
        # (a buffer that is large enough stays bound: binding invalidates the stored feature)
        need = L.lib().mvd_engine_deepcache_bytes(self._h, batch, h, w)
        if need < 0:
            raise L.MvdError(f"deepcache_bytes: {L.last_error()}")
        if self._dc is None or self._dc.numel() < need:
            self._dc = None
            self._dc = torch.empty(need, dtype=torch.uint8, device=self.device)
            L.call("mvd_engine_bind_deepcache", self._h, _ptr(self._dc), self._dc.numel())

    def _staged(self, name: str, t: torch.Tensor, shape=None) -> torch.Tensor:
        shape = tuple(t.shape) if shape is None else tuple(shape)
        buf = self._gbufs.get((name, shape))
        if buf is None:
            buf = self._gbufs[(name, shape)] = torch.empty(shape, dtype=torch.float32, device=self.device)
        if name != "out":
            buf.copy_(t)
        return buf

    @staticmethod
    def _entry(lay):
        # (suffix of the C entries for this layout, forward and sizing -- whose plain form is ``_args`` --, what goes beside the block)
        if lay.counts:
            return "_ragged", ((C.c_int * len(lay.counts))(*lay.counts), len(lay.counts))
        return ("_objects", (lay.objects,)) if lay.objects else ("", ())

    @staticmethod
    def _ref_key(batch, h, w, text_len, ref_batch, views=0, objects=0):
        return (batch, h, w, text_len, ref_batch) + ViewLayout.parse(views, objects, "key").key()

    def reference_cache_valid(self, batch, h, w, text_len, ref_batch, views=0, objects=0) -> bool:
        """True when the engine still holds reference K/V computed for exactly this shape (Q5 reuse is then legal); ``views``:
        by a shared-reference forward of that many views (of each of ``objects`` objects), or of exactly these view counts."""
        return getattr(self, "_ref_valid", None) == self._ref_key(batch, h, w, text_len, ref_batch, views, objects)

    # ------------------------------------------------------------------ measurement
    PROFILE_CLASSES = {0: "gemm_256x160", 1: "gemm_256x128", 2: "gemm_128x160", 3: "gemm_128x128", 4: "gemm_128x64",
                       5: "gemm_64x64", 6: "gemm_pp_256x320_geglu", 7: "gemm_pp_256x320_dense", 8: "attn_1wave", 9: "attn_2wave", 10: "attn_4wave", 11: "attn_8wave",
                       12: "gemm_128x320", 13: "gemm_pp_256x320_conv3x3", 14: "gemm_pp_256x320_splitk", 15: "gemm_pp_256x320_ln_dense",
                       16: "groupnorm", 17: "layernorm",
                       # small-M kernels (gemm_sm.hip), by tile
                       20: "gemm_sm_64x64", 21: "gemm_sm_128x64", 22: "gemm_sm_64x128", 23: "gemm_sm_128x128", 24: "gemm_sm_64x160",
                       25: "gemm_sm_128x160", 26: "gemm_sm_64x320",
                       # X-stationary short-K kernels (gemm_xs.hip)
                       30: "gemm_xs_dense", 31: "gemm_xs_residual", 32: "gemm_xs_ln_dense", 33: "gemm_xs_geglu",
                       # weight-streaming convolution of one image's 8x8 / 16x16 map (conv_ws.hip)
                       34: "conv_ws"}

    def set_profiling(self, enable):
        """False / 0: off.  True / 1: per-launch HIP events on ONE stream (serial kernel times).  2: per-launch events with the
        forward's own two-stream schedule kept (durations while the two passes share the chip)."""
        L.call("mvd_engine_set_profiling", self._h, int(enable))

    def profile_shapes(self) -> str:
        """Per-shape table of the recorded launches (call before profile_summary, which resets the records)."""
        buf = C.create_string_buffer(1 << 18)
        n = L.lib().mvd_engine_profile_shapes(self._h, buf, len(buf))
        if n < 0:
            raise L.MvdError(f"profile_shapes: {L.last_error()}")
        return buf.raw[:n].decode()

    def profile_summary(self):
        """{class name: dict(launches, ms, flops, bytes)} of the launches recorded since the last call."""
        cap = 32
        cls, n_l = (C.c_int * cap)(), (C.c_int * cap)()
        ms, fl, by = (C.c_double * cap)(), (C.c_double * cap)(), (C.c_double * cap)()
        n = L.lib().mvd_engine_profile_summary(self._h, cap, cls, n_l, ms, fl, by)
        if n < 0:
            raise L.MvdError(f"profile_summary: {L.last_error()}")
        return {self.PROFILE_CLASSES.get(cls[i], f"class{cls[i]}"): dict(launches=n_l[i], ms=ms[i], flops=fl[i], bytes=by[i])
                for i in range(n)}

    # ------------------------------------------------------------------ introspection (parity tests)
    def features(self) -> Dict[str, torch.Tensor]:
        names = [t[1] for t in self.cfg.transformers()]
        res = {}
        for i, n in enumerate(names):
            c, h, w = C.c_int(), C.c_int(), C.c_int()
            L.call("mvd_engine_feature_shape", self._h, i, C.byref(c), C.byref(h), C.byref(w))
            t = torch.empty(self._last_ref_batch, c.value, h.value, w.value, dtype=torch.float32, device=self.device)
            L.call("mvd_engine_get_feature", self._h, i, _ptr(t), L.stream())
            res[n] = t
        return res

    def camera_embedding(self, batch: int) -> torch.Tensor:
        t = torch.empty(batch, self.cam_output_dim, dtype=torch.float32, device=self.device)
        L.call("mvd_engine_get_camera_embedding", self._h, _ptr(t), L.stream())
        return t

    def hooked_modulators(self):
        """[(name, dim)] of the modulators the hooks address, in the engine's order (``mid`` is never addressed, Q3)."""
        ch = list(self.cfg.block_out_channels)
        n = len(ch)
        return [(f"down_{i}", ch[i]) for i in range(n)] + [(f"up_{i}", ch[n - 1 - i]) for i in range(n)] + [("output", 4)]

    def film_params(self, emb: torch.Tensor, out_rows: Optional[int] = None) -> Dict[str, tuple]:
        """{modulator: (scale, shift)}, (out_rows, dim) fp32 each, from a camera embedding (cam_batch, cam_output_dim): the FiLM
        parameters as the forward's camera path computes them (same function, same launches); rows beyond cam_batch repeat the
        cameras cyclically."""
        emb = emb.to(device=self.device, dtype=torch.float32).contiguous()
        assert emb.dim() == 2 and emb.shape[1] == self.cam_output_dim
        bc = emb.shape[0]
        rows = bc if out_rows is None else int(out_rows)
        if self._ws is None:
            self._ensure_workspace(max(rows, 1), 8, 8, 8, 0, False)
        mods = self.hooked_modulators()
        out = torch.empty(rows * 2 * sum(d for _, d in mods), dtype=torch.float32, device=self.device)
        L.call("mvd_engine_film_params", self._h, _ptr(emb), bc, rows, _ptr(out), L.stream())
        res, off = {}, 0
        for name, d in mods:
            res[name] = (out[off:off + rows * d].view(rows, d), out[off + rows * d:off + 2 * rows * d].view(rows, d))
            off += 2 * rows * d
        return res

    def time_projection(self, timesteps: torch.Tensor) -> Dict[int, torch.Tensor]:
        """{resnet index (module order): (B, cout) fp32}: every resnet's ``time_emb_proj(silu(time_embedding(t)))`` as the forward's
        time path computes it on the base weights."""
        t = timesteps.to(device=self.device, dtype=torch.float32).contiguous().view(-1)
        b = t.shape[0]
        if self._ws is None:
            self._ensure_workspace(max(b, 1), 8, 8, 8, 0, False)
        couts = [cout for _key, _cin, cout in self.cfg.resnets()]
        out = torch.empty(b, sum(couts), dtype=torch.float32, device=self.device)
        L.call("mvd_engine_time_projection", self._h, _ptr(t), b, _ptr(out), L.stream())
        res, off = {}, 0
        for i, c in enumerate(couts):
            res[i] = out[:, off:off + c]
            off += c
        return res
