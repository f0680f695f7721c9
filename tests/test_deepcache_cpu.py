"""DeepCache without a GPU: the reference of tests/deepcache_ref.py discriminates, and the host logic --
the interval schedule, the argument checks, the ``--deepcache`` parser and the trace of ``deep_cache`` keywords the denoising
loop hands to the UNet.

The reference (tiny topology, batch 2, 16 x 16 latents, text length 7; first step: seed-0 inputs at t = 500; second step: the same
with the ``sample`` of seed 1, at t = 100).  "replay" is the oracle in replay mode on the second step's inputs with the feature
recorded at the first step; "full" / "first" the plain oracle on the second / first step's inputs.  rel-L2, measured here:

                                            j0 = 1 (branch 0)   j0 = 0 (branch 1)
  replay vs full (second-step inputs)            0.87                0.48
  replay vs first-step output                    0.76                1.01
  replay vs full, identical inputs               exactly 0           exactly 0

so a forward that ignores the stored feature (it would equal "full"), one that returns the old output ("first"), and one that
stores at the wrong branch are each at least 4 x 3e-2 (four times the engine's parity cap) from the replay."""
from types import SimpleNamespace

import pytest
import torch

from tests import deepcache_ref as DR
from tests.freeu_ref import PARITY_BOUND_MAX


# ------------------------------------------------------------------------------------------------ the reference discriminates
@pytest.fixture(scope="module")
def steps():
    from oracle import mvd as OM
    from oracle import sd21_unet as OU
    from tests.parity_util import make_inputs
    cfg = OU.UNetConfig.tiny()
    params = OM.init_mvd_params(cfg, 0, cam_dim=96, cam_hidden=48)
    a = make_inputs(cfg, 2, 16, 7, 0, 96)
    b = dict(a, sample=make_inputs(cfg, 2, 16, 7, 1, 96)["sample"])

    def fwd(inp, t):
        with torch.no_grad():
            return OM.multiview_unet_forward(params, cfg, inp["sample"], torch.tensor(t), inp["text"], inp["src"], inp["tgt"], inp["lat"],
                                             fourier_proj=inp["proj"], img_ref_scale=0.3, cam_modulation_strength=0.2)
    return SimpleNamespace(cfg=cfg, a=a, b=b, fwd=fwd, first=fwd(a, 500), full=fwd(b, 100))


@pytest.mark.parametrize("branch", [0, 1])
def test_the_replayed_oracle_is_neither_the_full_forward_nor_the_old_output(steps, branch):
    from tests.parity_util import rel_l2
    store = {}
    with DR.deepcache_oracle("record", store, branch):
        rec = steps.fwd(steps.a, 500)
    assert torch.equal(rec, steps.first)                       # recording changes nothing
    j0 = steps.cfg.layers_per_block - 1 - branch
    hid = steps.cfg.block_out_channels[0] if j0 >= 1 else steps.cfg.block_out_channels[1]
    assert tuple(store["deep"].shape) == (2, hid, 16, 16)
    with DR.deepcache_oracle("replay", store, branch):
        replay = steps.fwd(steps.b, 100)
    e_full, e_first = rel_l2(replay, steps.full), rel_l2(replay, steps.first)
    print(f"deepcache oracle branch {branch} (j0 = {j0}): replay vs full {e_full:.3f}, replay vs first-step output {e_first:.3f}", flush=True)
    assert e_full >= 4 * PARITY_BOUND_MAX and e_first >= 4 * PARITY_BOUND_MAX, (e_full, e_first)
    # identical inputs: the replayed forward IS the full forward
    same = {}
    with DR.deepcache_oracle("record", same, branch):
        steps.fwd(steps.b, 100)
    with DR.deepcache_oracle("replay", same, branch):
        again = steps.fwd(steps.b, 100)
    assert torch.equal(again, steps.full)
    # the two branches store different tensors: a feature recorded at the other branch does not even fit, or is another function
    other = {}
    with DR.deepcache_oracle("record", other, 1 - branch):
        steps.fwd(steps.a, 500)
    assert other["deep"].shape != store["deep"].shape or not torch.equal(other["deep"], store["deep"])


def test_the_context_manager_puts_the_oracle_back(steps):
    from oracle import sd21_unet as OU
    f, r = OU.unet_forward, OU.resnet_block
    with DR.deepcache_oracle("record", {}, 0):
        assert OU.unet_forward is not f and OU.resnet_block is not r
    assert OU.unet_forward is f and OU.resnet_block is r
    assert DR.deep_key(steps.cfg, 0) == "up_blocks.3.resnets.1" and DR.deep_key(steps.cfg, 1) == "up_blocks.3.resnets.0"
    with pytest.raises(ValueError):
        DR.deep_key(steps.cfg, 2)


# ------------------------------------------------------------------------------------------------ host logic
def test_interval_schedule():
    from mvd_amd.pipeline import deepcache_schedule
    assert deepcache_schedule(None, 5) is None
    assert deepcache_schedule((1, 0), 5) is None                                  # interval 1: the loop as it always was
    assert deepcache_schedule((3, 0), 7) == ["refresh", "reuse", "reuse", "refresh", "reuse", "reuse", "refresh"]
    assert deepcache_schedule((2, 1), 5) == ["refresh", "reuse", "refresh", "reuse", "refresh"]
    assert deepcache_schedule((5, 0), 3) == ["refresh", "reuse", "reuse"]
    for n in (1, 2, 3, 5):
        s = deepcache_schedule((n, 0), 20) or ["refresh"] * 20
        assert [i for i, m in enumerate(s) if m == "refresh"] == list(range(0, 20, n))


def test_argument_checks():
    from mvd_amd.mvd_unet import check_deepcache
    assert check_deepcache(3, 0, 2) == (3, 0) and check_deepcache(1, 1, 2) == (1, 1) and check_deepcache(2.0, "1", 2) == (2, 1)
    for bad in ((0, 0), (-1, 0), (3, 2), (3, -1), (2.5, 0), (3, 0.5), ("x", 0), (None, 0), (True, 0)):
        with pytest.raises(ValueError):
            check_deepcache(*bad, 2)


def test_unet_and_pipeline_switches():
    """enable / disable on the module and through the pipeline; the keyword is refused while DeepCache is off -- all before any
    engine exists (no GPU)"""
    from mvd_amd._lib import MvdError
    from mvd_amd.config import UNetConfig
    from mvd_amd.mvd_unet import MultiViewUNet
    from mvd_amd.pipeline import MVDPipeline
    m = MultiViewUNet(None, unet_config=UNetConfig.tiny(), init="empty", cam_output_dim=96, cam_hidden_dim=48)
    assert m.deepcache is None
    m.enable_deepcache()
    assert m.deepcache == (3, 0)
    m.enable_deepcache(cache_interval=5, cache_branch_id=1)
    assert m.deepcache == (5, 1)
    with pytest.raises(ValueError):
        m.enable_deepcache(3, 2)                                                  # tiny: layers_per_block = 2
    assert m.deepcache == (5, 1)
    m.disable_deepcache()
    assert m.deepcache is None
    pipe = MVDPipeline(m, scheduler=None)
    pipe.enable_deepcache(2)
    assert m.deepcache == (2, 0)
    pipe.disable_deepcache()
    assert m.deepcache is None
    x = torch.zeros(1, 4, 16, 16)
    with pytest.raises(MvdError, match="enable_deepcache"):
        m(x, 1, torch.zeros(1, 7, 32), deep_cache="refresh")
    with pytest.raises(MvdError, match="expected None, 'refresh' or 'reuse'"):
        m(x, 1, torch.zeros(1, 7, 32), deep_cache="shallow")


def test_deepcache_parser():
    from mvd_amd.val import parse_deepcache
    assert parse_deepcache(None) is None and parse_deepcache("") is None and parse_deepcache(False) is None
    assert parse_deepcache("3") == (3, 0) and parse_deepcache("3,1") == (3, 1) and parse_deepcache(" 5 , 0 ") == (5, 0)
    assert parse_deepcache(3) == (3, 0) and parse_deepcache([2, 1]) == (2, 1) and parse_deepcache((4,)) == (4, 0)
    for bad in ("0", "3,-1", "3,1,2", "a", "2.5", "3,x", [1, 2, 3], True, ","):
        with pytest.raises(ValueError):
            parse_deepcache(bad)


def test_val_flag_reaches_the_parser():
    from mvd_amd import val
    with pytest.raises(SystemExit):
        val.main(["--ckpt", "x", "--dataset-path", "y", "--deepcache", "0"])


class _TraceUNet:
    """enough of MultiViewUNet for the loop: records the ``deep_cache`` keyword of every call"""
    def __init__(self, setting):
        self.deepcache, self.calls, self.resets = setting, [], 0

    def _exec_device(self):
        return torch.device("cpu")

    def reset_reference_cache(self):
        self.resets += 1

    def __call__(self, **kw):
        self.calls.append(kw.get("deep_cache", "absent"))
        return SimpleNamespace(sample=0.5 * kw["sample"])


class _TraceScheduler:
    init_noise_sigma = 1.0

    def set_timesteps(self, n):
        self.timesteps = torch.linspace(900, 0, n).long()

    def step(self, out, t, latents, noise=None):
        return SimpleNamespace(prev_sample=latents - 0.1 * out)


@pytest.mark.parametrize("setting, want", [
    ((3, 0), ["refresh", "reuse", "reuse", "refresh", "reuse", "reuse", "refresh"]),
    ((2, 1), ["refresh", "reuse", "refresh", "reuse", "refresh", "reuse", "refresh"]),
    ((1, 0), ["absent"] * 7),
    (None, ["absent"] * 7),
], ids=["interval3", "interval2", "interval1", "off"])
def test_generation_trace(setting, want):
    """7 steps: the UNet receives refresh, reuse, reuse, refresh, reuse, reuse, refresh under interval 3; no keyword at all with
    interval 1 or DeepCache off; the reference cache (and with it the stored feature) is reset once, before the first step"""
    from mvd_amd.pipeline import MVDDenoiser
    unet = _TraceUNet(setting)
    lat = MVDDenoiser(unet, _TraceScheduler())(torch.zeros(1, 7, 32), num_inference_steps=7, guidance_scale=1.0,
                                               latents=torch.ones(1, 4, 4, 4))
    assert unet.calls == want and unet.resets == 1
    assert lat.shape == (1, 4, 4, 4) and torch.isfinite(lat).all()


# ------------------------------------------------------------------------------------------------ the C ABI's host side (dry runs, no GPU)
def test_sizing_entries_and_setting_checks():
    """the sizing entries size the forward the bits describe (a shallow forward never needs more than the full one: checked in
    the library, and smaller here), and the setting's rejections come without a GPU"""
    import ctypes as C

    from mvd_amd import _lib as L
    from mvd_amd.config import UNetConfig
    from tests.test_cabi_cpu import _mk_engine
    import os
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = L.lib()
    rc, h = _mk_engine(lib, UNetConfig.sd21())
    assert rc == 0, L.last_error()

    def args(flags, batch=2, views=0):
        a = L.mvd_forward_args_t()
        a.batch, a.height, a.width, a.text_len, a.ref_batch, a.cam_rows, a.views = batch, 64, 64, 77, 1 if views else batch, 4, views
        a.cam_batch = batch
        a.flags = flags
        return a
    base = L.MVD_USE_CAMERA | L.MVD_USE_IMAGE
    full = lib.mvd_engine_workspace_bytes_args(h, C.byref(args(base)))
    assert full > 0, L.last_error()
    # the bits without the setting
    for bit in (L.MVD_DEEPCACHE_REFRESH, L.MVD_DEEPCACHE_SHALLOW):
        assert lib.mvd_engine_workspace_bytes_args(h, C.byref(args(base | bit))) == -1
        assert "without mvd_engine_set_deepcache" in L.last_error()
    assert lib.mvd_engine_set_deepcache(h, 2) == -1 and "outside [0, 2)" in L.last_error()
    assert lib.mvd_engine_set_deepcache(h, -1) == -1
    sizes = {}
    for branch in (0, 1):
        assert lib.mvd_engine_set_deepcache(h, branch) == 0, L.last_error()
        assert lib.mvd_engine_workspace_bytes_args(h, C.byref(args(base | L.MVD_DEEPCACHE_REFRESH))) == full
        sizes[branch] = lib.mvd_engine_workspace_bytes_args(h, C.byref(args(base | L.MVD_DEEPCACHE_SHALLOW)))
        assert 0 < sizes[branch] < full, (sizes, full, L.last_error())
        both = lib.mvd_engine_workspace_bytes_args(h, C.byref(args(base | L.MVD_DEEPCACHE_REFRESH | L.MVD_DEEPCACHE_SHALLOW)))
        assert both == -1 and "one or the other" in L.last_error()
        # the views and ragged forms
        v = args(base | L.MVD_SHARE_REF | L.MVD_DEEPCACHE_SHALLOW, batch=8, views=4)
        fv = args(base | L.MVD_SHARE_REF, batch=8, views=4)
        v.cam_batch = fv.cam_batch = 4                                              # (one camera per view)
        assert 0 < lib.mvd_engine_workspace_bytes_args(h, C.byref(v)) < lib.mvd_engine_workspace_bytes_args(h, C.byref(fv))
        counts = (C.c_int * 2)(2, 1)
        r = args(base | L.MVD_SHARE_REF | L.MVD_DEEPCACHE_SHALLOW, batch=6)
        r.ref_batch, r.cam_batch = 2, 3
        fr = args(base | L.MVD_SHARE_REF, batch=6)
        fr.ref_batch, fr.cam_batch = 2, 3
        assert 0 < lib.mvd_engine_workspace_bytes_ragged(h, C.byref(r), counts, 2) < lib.mvd_engine_workspace_bytes_ragged(h, C.byref(fr), counts, 2), L.last_error()
    assert sizes[0] <= sizes[1]
    # the buffer: [batch][H][W][max(C0, C1)] bf16, for any branch
    assert lib.mvd_engine_deepcache_bytes(h, 2, 64, 64) == 2 * 64 * 64 * 640 * 2
    assert lib.mvd_engine_deepcache_bytes(h, 0, 64, 64) == -1
    assert lib.mvd_engine_bind_deepcache(h, C.c_void_p(128), 1 << 20) == -1 and "256-byte aligned" in L.last_error()
    # the encoder pass alone takes neither bit; a forward without a workspace still fails on the bits first
    a = args(base | L.MVD_DEEPCACHE_REFRESH)
    assert lib.mvd_engine_reference_encode(h, C.byref(a), C.c_void_p(256), None) == -1 and "DeepCache bits" in L.last_error()
    assert lib.mvd_engine_clear_deepcache(h) == 0
    assert lib.mvd_engine_workspace_bytes_args(h, C.byref(args(base | L.MVD_DEEPCACHE_SHALLOW))) == -1
    lib.mvd_engine_destroy(h)
