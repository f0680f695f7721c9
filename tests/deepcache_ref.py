"""Reference for DeepCache, shared by tests/test_deepcache_cpu.py and tests/test_deepcache_gpu.py.

``deepcache_oracle``: a context manager under which the MAIN pass of the oracle's forwards (``oracle.sd21_unet.unet_forward`` and
everything built on it, ``oracle.mvd.multiview_unet_forward`` included) records, or replays, the DEEP FEATURE of a branch b: the
hidden half (not the skip half) of the concatenated input of ``up_blocks.{n-1}.resnets.{j0}``, j0 = layers_per_block - 1 - b.

  mode "record"   the forward is what it was; ``store["deep"]`` is a copy of ``x[:, :hid]`` at that resnet;
  mode "replay"   ``x[:, :hid]`` is REPLACED by ``store["deep"]`` there; everything else runs as ever.

A shallow forward is, by definition, the full forward with that one tensor replaced by the stored one: every layer it executes
lies behind the replacement or reads nothing that depends on the replaced layers, so the replayed oracle forward is its
reference -- the oracle simply also computes the deep layers whose result is then thrown away.  The encoder pass (the one
forward that passes ``capture``) is untouched.

Plain helper module, no fixtures; nothing here touches the code under test and ``oracle/`` is not edited: two module attributes
are swapped for the duration of the ``with`` block and put back, exactly as ``tests/freeu_ref.freeu_oracle`` does (the two nest)."""
import contextlib

import torch

from oracle import sd21_unet as OU


def deep_key(cfg, branch: int = 0) -> str:
    """the resnet whose hidden input is the deep feature of ``branch``"""
    j0 = cfg.layers_per_block - 1 - branch
    if not 0 <= branch < cfg.layers_per_block:
        raise ValueError(f"branch {branch} outside [0, {cfg.layers_per_block})")
    return f"up_blocks.{cfg.num_levels - 1}.resnets.{j0}"


@contextlib.contextmanager
def deepcache_oracle(mode, store: dict, branch: int = 0):
    """``mode``: "record" or "replay", or a callable k -> "record" / "replay" asked once per MAIN-pass forward with that forward's
    0-based number inside the block (a denoising loop: ``deepcache_loop``); ``store``: the dict that holds the feature under
    "deep" (written / read)."""
    if not callable(mode) and mode not in ("record", "replay"):
        raise ValueError(mode)
    count = {"k": 0, "mode": None if callable(mode) else mode}
    orig_forward, orig_resnet = OU.unet_forward, OU.resnet_block
    state = {"cfg": None}

    def forward(p, cfg, sample, timestep, text, attn_hook=None, block_hook=None, capture=None, **kw):
        prev = state["cfg"]
        state["cfg"] = cfg if capture is None else None
        if capture is None and callable(mode):
            count["mode"] = mode(count["k"])
            assert count["mode"] in ("record", "replay"), count["mode"]
            count["k"] += 1
        try:
            return orig_forward(p, cfg, sample, timestep, text, attn_hook=attn_hook, block_hook=block_hook, capture=capture, **kw)
        finally:
            state["cfg"] = prev

    def resnet(p, key, x, temb_act, groups, eps):
        cfg = state["cfg"]
        if cfg is not None and key == deep_key(cfg, branch):
            j0 = cfg.layers_per_block - 1 - branch
            hid = OU.up_block_resnet_channels(cfg)[cfg.num_levels - 1][j0][0]
            if count["mode"] == "record":
                store["deep"] = x[:, :hid].clone()
            else:
                deep = store["deep"]
                assert deep.shape == x[:, :hid].shape, (tuple(deep.shape), tuple(x[:, :hid].shape))
                x = torch.cat([deep.to(x.dtype), x[:, hid:]], dim=1)
        return orig_resnet(p, key, x, temb_act, groups, eps)

    OU.unet_forward, OU.resnet_block = forward, resnet
    try:
        yield store
    finally:
        OU.unet_forward, OU.resnet_block = orig_forward, orig_resnet


def deepcache_loop(interval: int, branch: int = 0):
    """The oracle under which a denoising loop (one main-pass forward per step, ``tests/sampler_ref.denoise_loop``) runs DeepCache:
    step i records iff ``i % interval == 0`` and replays otherwise.  One ``with`` block per loop: the step count starts at 0."""
    return deepcache_oracle(lambda k: "record" if k % interval == 0 else "replay", {}, branch)
