"""Token downsampling of the self-attention keys (ToDo) without a GPU: the restatement of tests/todo_ref.py
against torch's own ``F.interpolate`` / ``F.avg_pool2d``, linearity (pooling K/V rows is K/V of pooled tokens), which blocks are
downsampled, that every op-level fault would fail the operator checks of tests/test_todo_ops_gpu.py, how far every wrong variant
of the oracle lies from the right one (what the engine test's bound rests on), and the host plumbing from ``--todo`` and the
pipeline's three entry points down to the engine's setting.

Engine-level separation, tiny topology, 16 x 16, seeds 0..3 of the engine tests' inputs (rel-L2 from the ToDo oracle of the same
setting; the engine test's parity bound is capped at ``todo_ref.PARITY_BOUND_MAX`` = 3e-2, so 1.2e-1 is four bounds).  Measured:
  (2, 1, nearest): plain oracle 1.86e-1 .. 2.42e-1, levels_shift 2.12e-1 .. 2.71e-1, factor_off 3.27e-1 .. 3.87e-1,
                   swap_method 2.72e-1 .. 3.22e-1, corner 2.88e-1 .. 3.52e-1, also_ref 1.66e-2 .. 2.09e-2
  (2, 2, area):    plain oracle 2.09e-1 .. 2.36e-1, levels_shift 2.01e-1 .. 2.27e-1, factor_off 1.03e-1 .. 1.21e-1 (four bounds at
                   seed 2 only), swap_method 3.02e-1 .. 3.32e-1, also_ref 3.80e-2 .. 4.69e-2
``also_ref`` (the reference K/V downsampled too) reaches four bounds at no seed: the adapter's branch enters with img_ref_scale 0.3,
and at a scale large enough to lift it (4.0: 1.1e-1 .. 1.5e-1) the plain oracle itself falls to 0.9e-1 .. 1.2e-1.  It is NOT judged
by the parity bound.  What judges it: the engine test asserts that the ToDo forward lies closer to the right oracle than to the
``also_ref`` oracle, and the operator takes no reference pointer at all -- the engine hands the reference K/V to the attention
launch as it always did (problem 1 of the launch, untouched by the branch).  ``factor_off`` is also pinned by ``todo_keys()`` ==
``todo_blocks()`` in the engine test and by the output's shape at operator level; ``corner`` and ``swap_method`` are bit-pinned
at operator level (tests/test_todo_ops_gpu.py)."""
import functools
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from tests import todo_ref as T

GEOMETRIES = [(7, 9, 2), (7, 10, 3), (9, 9, 4), (8, 8, 2), (6, 10, 2)]


def _map(B, H, W, C, seed, integer=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-8, 9, (B, H * W, C), generator=g).float() if integer else torch.randn(B, H * W, C, generator=g)
    return x.to(torch.bfloat16)


def _nchw(x, H, W):
    return x.reshape(x.shape[0], H, W, -1).permute(0, 3, 1, 2)


def _rows(m):
    return m.permute(0, 2, 3, 1).reshape(m.shape[0], -1, m.shape[1])


# ------------------------------------------------------------------------------------------------ the restatement is torch's
@pytest.mark.parametrize("H,W,f", GEOMETRIES)
def test_nearest_is_interpolate_nearest(H, W, f):
    x = _map(2, H, W, 16, 1)
    want = _rows(F.interpolate(_nchw(x.float(), H, W), scale_factor=1 / f, mode="nearest")).to(torch.bfloat16)
    got = T.downsample(x, H, W, f, "nearest")
    assert got.shape[1] == T.key_grid(H, W, f)[2] and torch.equal(got, want)


@pytest.mark.parametrize("H,W,f", GEOMETRIES)
def test_area_is_avg_pool2d(H, W, f):
    xi = _map(2, H, W, 16, 2, integer=True)
    assert torch.equal(T.downsample(xi, H, W, f, "area"), _rows(F.avg_pool2d(_nchw(xi.float(), H, W), f)).to(torch.bfloat16))
    xg = _map(2, H, W, 64, 3)
    got = T.downsample(xg, H, W, f, "area")
    want = _rows(F.avg_pool2d(_nchw(xg.double(), H, W), f))
    ulp = torch.maximum(want.abs(), torch.tensor(2.0 ** -126, dtype=torch.float64)).log2().floor().exp2() * 2.0 ** -7      # one bf16 ulp at |want|
    assert ((got.double() - want).abs() <= ulp).all()
    # fp32 / fp64 rows (the oracle's): the same mean in that type
    assert torch.allclose(T.downsample(xg.double(), H, W, f, "area"), want, rtol=1e-14, atol=0)


@pytest.mark.parametrize("H,W,f", GEOMETRIES)
def test_pooling_kv_rows_is_kv_of_pooled_tokens(H, W, f):
    """to_k / to_v are row-wise and bias-free: nearest commutes exactly (integer data: every sum exact whatever its order), area by
    linearity (fp64)"""
    g = torch.Generator().manual_seed(4)
    C = 24
    xi = torch.randint(-4, 5, (2, H * W, C), generator=g).double()
    wi = torch.randint(-3, 4, (C, C), generator=g).double()
    assert torch.equal(T.downsample(F.linear(xi, wi), H, W, f, "nearest"), F.linear(T.downsample(xi, H, W, f, "nearest"), wi))
    x, w = torch.randn(2, H * W, C, generator=g, dtype=torch.float64), torch.randn(C, C, generator=g, dtype=torch.float64)
    assert torch.allclose(T.downsample(F.linear(x, w), H, W, f, "area"), F.linear(T.downsample(x, H, W, f, "area"), w), rtol=1e-12, atol=1e-13)


# ------------------------------------------------------------------------------------------------ which blocks
LEVEL0 = ["down_block_0_attn_0", "down_block_0_attn_1", "up_block_3_attn_0", "up_block_3_attn_1", "up_block_3_attn_2"]
LEVEL1 = ["down_block_1_attn_0", "down_block_1_attn_1", "up_block_2_attn_0", "up_block_2_attn_1", "up_block_2_attn_2"]


@pytest.mark.parametrize("which", ["tiny", "sd21"])
def test_todo_blocks_against_a_hand_count(which):
    """both topologies have four levels with five transformer blocks at each of levels 0 and 1; deeper blocks never take part"""
    from mvd_amd.config import UNetConfig
    from mvd_amd.unet_params import todo_blocks
    cfg = getattr(UNetConfig, which)()

    def both(l0, l1):
        return {**{n: l0 for n in LEVEL0 if l0}, **{n: l1 for n in LEVEL1 if l1}}
    assert todo_blocks(cfg, 16, 16, 2, 1) == both((16, 16, 2, 64), None)
    assert todo_blocks(cfg, 16, 16, 2, 2) == both((16, 16, 2, 64), (8, 8, 2, 16))
    assert todo_blocks(cfg, 16, 16, 4, 1) == both((16, 16, 4, 16), None)
    assert todo_blocks(cfg, 16, 16, 1, 3) == both(None, (8, 8, 3, 4))
    assert todo_blocks(cfg, 16, 32, 2, 1) == both((16, 32, 2, 128), None)
    assert todo_blocks(cfg, 16, 32, 3, 3) == both((16, 32, 3, 50), (8, 16, 3, 10))
    assert todo_blocks(cfg, 64, 64, 2, 1) == both((64, 64, 2, 1024), None)
    assert todo_blocks(cfg, 64, 64, 2, 2) == both((64, 64, 2, 1024), (32, 32, 2, 256))
    assert todo_blocks(cfg, 64, 64, 3, 4) == both((64, 64, 3, 441), (32, 32, 4, 64))
    assert todo_blocks(cfg, 96, 96, 2, 1) == both((96, 96, 2, 2304), None)
    assert todo_blocks(cfg, 96, 96, 4, 2) == both((96, 96, 4, 576), (48, 48, 2, 576))
    assert todo_blocks(cfg, 64, 64, 1, 1) == {}
    assert todo_blocks(cfg, 8, 8, 4, 4) == both((8, 8, 4, 4), (4, 4, 4, 1))
    assert todo_blocks(cfg, 8, 16, 3, 4) == both((8, 16, 3, 10), (4, 8, 4, 2))
    assert todo_blocks(cfg, 8, 8, 1, 3) == both(None, (4, 4, 3, 1))
    # the oracle's rule is the same rule
    for (h, w) in ((16, 16), (16, 32), (64, 64), (96, 96), (8, 8)):
        for fs in ((2, 1), (2, 2), (4, 3), (1, 4)):
            got = todo_blocks(cfg, h, w, *fs)
            for lv in range(4):
                H, W = h >> lv, w >> lv
                f = T.block_factor((h, w), H, W, *fs)
                names = [n for n, v in got.items() if v[:2] == (H, W)]
                assert (f > 1) == bool(names) and all(got[n][2:] == (f, T.key_grid(H, W, f)[2]) for n in names), (h, w, fs, lv)


# ------------------------------------------------------------------------------------------------ op-level faults are caught
def _applies(fault, case, method):
    B, H, W, C, f = case
    return {"corner": method == "nearest", "sum order reversed": method == "area", "truncation for RNE": method == "area",
            "incomplete last cell included": bool(H % f or W % f), "batch stride hw*C for hw*ld": B > 1}.get(fault, True)


@pytest.mark.parametrize("case", T.OP_CASES, ids=T.case_id)
def test_every_op_level_fault_fails_the_operator_checks(case):
    """the GPU test runs ``check_op`` on every (case, width, input kind, method); a kernel with one of these faults fails at least
    one of them -- and the fault-free restatement passes all"""
    B, H, W, C, f = case
    caught = {name: False for name in T.OP_FAULTS}
    for width in T.OP_WIDTHS:
        for kind in T.OP_INPUTS:
            qkv = T.fused_rows(case, width, kind)
            for method in T.METHODS:
                T.check_op(T.reference_kv(qkv, C, H, W, f, method), qkv, case, method)
                for name, kw in T.OP_FAULTS.items():
                    if not _applies(name, case, method):
                        continue
                    try:
                        T.check_op(T.reference_kv(qkv, C, H, W, f, method, **kw), qkv, case, method)
                    except AssertionError:
                        caught[name] = True
    applicable = {name for name in T.OP_FAULTS if any(_applies(name, case, m) for m in T.METHODS)}
    assert all(caught[name] for name in applicable), {n: caught[n] for n in applicable}
    # every fault is applicable somewhere in the case list
    assert all(any(_applies(name, c, m) for c in T.OP_CASES for m in T.METHODS) for name in T.OP_FAULTS)


def test_the_cancel_inputs_depend_on_the_order_of_the_sum():
    """the reversed sum differs from the forward one in a large share of the outputs, for every factor"""
    for case in ((1, 8, 8, 320, 2), (2, 7, 10, 320, 3), (1, 9, 9, 1280, 4)):
        B, H, W, C, f = case
        k = T.fused_rows(case, 3, "cancel")[..., C:2 * C]
        a, b = T.downsample(k, H, W, f, "area"), T.downsample(k, H, W, f, "area", reverse_sum=True)
        share = (a != b).float().mean().item()
        print(f"cancel inputs f={f}: {100 * share:.1f} % of the means depend on the order")
        assert share > 0.2


# ------------------------------------------------------------------------------------------------ engine-level separation
@functools.lru_cache(maxsize=None)
def _oracle_setup():
    from oracle import mvd as OM
    from oracle import sd21_unet as OU
    cfg = OU.UNetConfig.tiny()
    return cfg, OM.init_mvd_params(cfg, 0, cam_dim=96, cam_hidden=48)


def _forward(inp):
    from oracle import mvd as OM
    cfg, params = _oracle_setup()
    with torch.no_grad():
        return OM.multiview_unet_forward(params, cfg, inp["sample"], torch.tensor(500), inp["text"], inp["src"], inp["tgt"], inp["lat"],
                                         fourier_proj=inp["proj"], img_ref_scale=0.3, cam_modulation_strength=0.2)


NOT_BY_THE_BOUND = ("also_ref",)
SEEDS = (0, 1, 2, 3)


@pytest.mark.parametrize("setting", [T.PARITY_SETTING, dict(factor=2, factor_level_2=2, method="area")], ids=["2_1_nearest", "2_2_area"])
def test_every_wrong_variant_is_four_bounds_from_the_todo_oracle(setting):
    """per variant the distances at a handful of seeds (seed 0: the engine test's inputs); all but ``NOT_BY_THE_BOUND`` reach four
    bounds at one of them at least, the plain oracle at every one"""
    from tests.parity_util import make_inputs, rel_l2
    cfg, _ = _oracle_setup()
    variants = [("levels_shift", dict(levels_shift=1)), ("factor_off", dict(factor_off=True)), ("also_ref", dict(also_ref=True)),
                ("swap_method", dict(swap_method=True))]
    if setting["method"] == "nearest":
        variants.append(("corner", dict(corner=True)))
    dist = {name: [] for name in ["plain oracle"] + [v[0] for v in variants]}
    for seed in SEEDS:
        inp = make_inputs(cfg, 2, 16, 7, seed, 96)
        rec = {}
        with T.todo_oracle(**setting, record=rec):
            want = _forward(inp)
        expect = {n: 64 for n in LEVEL0}
        if setting["factor_level_2"] > 1:
            expect.update({n: 16 for n in LEVEL1})
        assert rec == expect
        dist["plain oracle"].append(rel_l2(_forward(inp), want))
        for name, kw in variants:
            with T.todo_oracle(**setting, **kw):
                dist[name].append(rel_l2(_forward(inp), want))
    print(f"{setting}: " + ", ".join(f"{k} " + " ".join(f"{d:.3e}" for d in v) for k, v in dist.items()))
    assert min(dist["plain oracle"]) >= 4 * T.PARITY_BOUND_MAX
    for name, d in dist.items():
        if name in NOT_BY_THE_BOUND:
            assert min(d) > 0.0, name
        else:
            assert max(d) >= 4 * T.PARITY_BOUND_MAX, (name, d)


def test_the_48x48_inputs_separate_on_from_off_on_the_oracle():
    """``todo_ref.parity_inputs`` at 48 x 48 (576 keys at level 0): with white noise alone the oracle's ToDo result is closer to its
    plain result than four parity bounds can be (measured 5.6e-2; four bounds are 7.5e-2 at the least); with the period-2 component
    it is at least four CAPS away (measured 2.66e-1), and so is the other corner (4.26e-1).  The smaller cases are what they were"""
    from tests.parity_util import make_inputs, rel_l2
    cfg, _ = _oracle_setup()
    for hw in (16, (16, 32)):
        a, b = T.parity_inputs(cfg, 2, hw), make_inputs(cfg, 2, hw, 7, 0, 96)
        assert all(torch.equal(a[k], b[k]) for k in b)
    inp, white = T.parity_inputs(cfg, 2, 48), make_inputs(cfg, 2, 48, 7, 0, 96)
    assert not torch.equal(inp["sample"], white["sample"]) and all(torch.equal(inp[k], white[k]) for k in white if k != "sample")
    assert abs(float((inp["sample"] - white["sample"]).mean())) < 1e-6
    dist = {}
    for name, x in (("white noise", white), ("with the period-2 component", inp)):
        plain = _forward(x)
        with T.todo_oracle(**T.PARITY_SETTING):
            want = _forward(x)
        dist[name] = rel_l2(plain, want)
    with T.todo_oracle(**T.PARITY_SETTING, corner=True):
        dist["corner"] = rel_l2(_forward(inp), want)
    print("48 x 48, oracle, ToDo (2, 1, nearest) to plain: " + ", ".join(f"{k} {v:.3e}" for k, v in dist.items()))
    assert dist["with the period-2 component"] >= 4 * T.PARITY_BOUND_MAX and dist["corner"] >= 4 * T.PARITY_BOUND_MAX
    assert dist["white noise"] < dist["with the period-2 component"]


def test_the_oracle_leaves_the_encoder_pass_alone_and_puts_the_modules_back():
    from oracle import mvd as OM
    from oracle import sd21_unet as OU
    from tests.parity_util import make_inputs
    cfg, _ = _oracle_setup()
    inp = make_inputs(cfg, 2, 16, 7, 0, 96)
    orig = (OU.unet_forward, OU.transformer_2d, OM.image_cross_attention)
    seen = []
    real = T.downsample

    def spy(x, H, W, f, method, **kw):
        seen.append((tuple(x.shape), f, method))
        return real(x, H, W, f, method, **kw)
    T.downsample = spy
    try:
        with T.todo_oracle(2, 2, "area"):
            _forward(inp)
    finally:
        T.downsample = real
    assert (OU.unet_forward, OU.transformer_2d, OM.image_cross_attention) == orig
    # five level-0 and five level-1 blocks of the main pass, attn1 only; the encoder pass (which passes ``capture``) would double them
    assert sorted(seen) == sorted([((2, 256, 64), 2, "area")] * 5 + [((2, 64, 128), 2, "area")] * 5), seen
    with T.todo_oracle(1, 1):
        assert torch.equal(_forward(inp), _forward(inp))


# ------------------------------------------------------------------------------------------------ host plumbing
def _model():
    from mvd_amd.config import UNetConfig
    from mvd_amd.mvd_unet import MultiViewUNet
    return MultiViewUNet(None, unet_config=UNetConfig.tiny(), init="empty", cam_output_dim=96, cam_hidden_dim=48)


def test_enable_todo_on_the_three_surfaces_and_the_mutual_refusal():
    from mvd_amd.pipeline import MVDPipeline
    m = _model()
    pipe = MVDPipeline(m, SimpleNamespace(init_noise_sigma=1.0))
    assert m.todo is None
    m.base_unet.enable_todo()
    assert m.todo == (2, 1, "nearest") == m.base_unet.todo
    m.enable_todo(3, 2, "area")
    assert m.todo == (3, 2, "area")
    pipe.enable_todo(factor_level_2=4, method="area")
    assert m.todo == (2, 4, "area")
    for surface in (m.base_unet, m, pipe):
        for bad in ((0, 1, "nearest"), (5, 1, "nearest"), (2, 0, "nearest"), (2, 5, "area"), (2.0, 1, "nearest"), (True, 1, "nearest"), (2, 1, "bilinear"), (2, 1, 0)):
            with pytest.raises(ValueError, match="token downsampling"):
                surface.enable_todo(*bad)
        with pytest.raises(ValueError, match="alternatives"):
            surface.enable_tome(0.5)
        assert m.todo == (2, 4, "area") and m.tome is None           # a refusal changes nothing
    pipe.disable_todo()
    assert m.todo is None and m.base_unet.todo is None
    pipe.enable_tome(0.5)
    for surface in (m.base_unet, m, pipe):
        with pytest.raises(ValueError, match="alternatives"):
            surface.enable_todo()
        assert m.todo is None and m.tome == (0.5, 1)
    m.enable_todo(1, 1)                                              # both factors 1 touch nothing: not an alternative to anything
    m.enable_tome(0.0)
    m.enable_todo(2)                                                 # ratio 0 merges nothing
    with pytest.raises(ValueError, match="main pass only"):
        m.image_encoder.unet.enable_todo()


def test_parse_todo():
    from mvd_amd.val import parse_todo
    assert parse_todo(None) is None and parse_todo("") is None
    assert parse_todo("2") == (2, 1, "nearest") == parse_todo(2) == parse_todo([2]) == parse_todo(" 2 , 1")
    assert parse_todo("2,2") == (2, 2, "nearest") == parse_todo([2, 2])
    assert parse_todo("3,1,area") == (3, 1, "area") == parse_todo([3, 1, "area"])
    for bad in ("2,1,area,4", "a", "5", "2,0", "2.5", "2,1,bilinear", True, [1, 2, 3, 4]):
        with pytest.raises(ValueError):
            parse_todo(bad)


@pytest.mark.parametrize("flag", [None, "2", "2,2,area"])
def test_val_flag_reaches_the_config_and_the_pipeline(monkeypatch, tmp_path, flag):
    import mvd_amd.dataset as D
    import mvd_amd.val as V
    seen = {}
    monkeypatch.setattr(V, "load_config", lambda path: dict(image_size=[32, 32], max_views_per_object=4))
    monkeypatch.setattr(V, "setup_pipeline", lambda config, ckpt, device: "pipe")
    monkeypatch.setattr(D, "ObjaverseDataset", lambda **kw: "dataset")
    monkeypatch.setattr(V, "run_validation", lambda pipeline, dataset, config, device, output_dir, **kw: (seen.update(config), ([], {}))[1])
    argv = ["--ckpt", "x.ckpt", "--dataset-path", "data", "--output-dir", str(tmp_path)] + (["--todo", flag] if flag else [])
    assert V.main(argv) == 0
    assert seen.get("todo") == flag
    with pytest.raises(SystemExit):
        V.main(argv[:6] + ["--todo", "7"])
    monkeypatch.undo()
    calls = []

    class Stop(Exception):
        pass

    class Pipe:
        def enable_todo(self, *a):
            calls.append(a)
            raise Stop
    if flag:
        with pytest.raises(Stop):
            V.run_validation(Pipe(), [], dict(batch_size=1, num_workers=0, todo=flag), "cpu", tmp_path, metrics=object())
        assert calls == [V.parse_todo(flag)]


class _StubEngine:
    """records what ``MultiViewUNet._ensure_engine`` hands down and every forward"""
    device = torch.device("cpu")
    _graph = False

    def __init__(self):
        from mvd_amd.main_options import MainOptions
        self.log, self.options = [], MainOptions()

    def set_todo(self, *a):
        self.log.append(("set_todo",) + a)
        self.options = self.options._replace(todo=a)

    def clear_todo(self):
        self.log.append(("clear_todo",))
        self.options = self.options._replace(todo=None)

    def set_tome(self, *a, **kw):
        assert self.options.todo is None, "set_tome while token downsampling is set: the engine would refuse"
        self.log.append(("set_tome",) + a)
        self.options = self.options._replace(tome=a)

    def clear_tome(self):
        self.log.append(("clear_tome",))
        self.options = self.options._replace(tome=None)

    def forward(self, x, t, text, **kw):
        self.log.append(("forward", self.options.todo))
        return torch.zeros_like(x)

    def reference_cache_valid(self, *a, **kw):
        return False

    def camera_embedding(self, n):
        return torch.zeros(n, 96)


@pytest.mark.parametrize("entry", ["call", "views3", "objects2x2", "list21"])
def test_the_pipelines_entry_points_hand_the_setting_down(entry, monkeypatch):
    """``__call__``, ``generate_views`` and both forms of ``generate_views_batch`` run every UNet forward with the engine set as the
    pipeline was told -- and a setting changed between two calls reaches the engine before the next forward"""
    from mvd_amd import ops
    from mvd_amd.pipeline import MVDPipeline, _make_scheduler
    from tests import test_generation_trace_cpu as G
    for fn in G.OPS:
        monkeypatch.setattr(ops, fn.__name__, fn)
    m = _model()
    eng = _StubEngine()
    m._engine, m._dirty = eng, False
    m._exec_device = lambda: torch.device("cpu")
    m.fourier_projection = torch.zeros(1)
    pipe = MVDPipeline(m, _make_scheduler(None, "ddim"))
    prompts, rows, sources = G.LAYOUT[entry]
    dim = m.unet_config.cross_attention_dim

    def run():
        fn, kw = G._entry(pipe, entry)
        kw.update(prompt_embeds=G._rand(1, prompts, 7, dim), latents=G._rand(2, rows, 4, 2, 2), num_inference_steps=2, guidance_scale=3.0,
                  source_image_latents=G._rand(5, sources, 4, 2, 2), output_type="latent")
        del eng.log[:]
        fn(**kw)
        return [e for e in eng.log if e[0] != "forward"], {e[1] for e in eng.log if e[0] == "forward"}
    assert run() == ([], {None})
    pipe.enable_todo(2, 2, "area")
    assert run() == ([("set_todo", 2, 2, "area")], {(2, 2, "area")})
    assert run() == ([], {(2, 2, "area")})                              # unchanged: nothing is set again
    pipe.enable_todo(3)
    assert run() == ([("set_todo", 3, 1, "nearest")], {(3, 1, "nearest")})
    pipe.disable_todo()
    pipe.enable_tome(0.5)                                            # the one being switched off goes first
    sets, seen = run()
    assert [s[0] for s in sets] == ["clear_todo", "set_tome"] and seen == {None}
    pipe.disable_tome()
    pipe.enable_todo(1, 1)                                           # both factors 1: the engine is not touched
    sets, seen = run()
    assert [s[0] for s in sets] == ["clear_tome"] and seen == {None}


# ------------------------------------------------------------------------------------------------ the C ABI on the host
def test_c_symbols_resolve_and_refuse_on_the_host():
    import ctypes as C
    import os

    from mvd_amd import _lib as L
    from mvd_amd.config import UNetConfig
    from tests.test_cabi_cpu import _mk_engine
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = L.lib()
    for name in ("mvd_op_todo_downsample", "mvd_engine_set_todo", "mvd_engine_clear_todo", "mvd_engine_todo_keys"):
        assert getattr(lib, name) is not None
    assert lib.mvd_engine_set_todo(None, 2, 1, 0) == -1 and b"null engine" in lib.mvd_last_error()
    assert lib.mvd_engine_clear_todo(None) == -1
    # the operator's refusals need no device: every one comes before the launch
    p = C.c_void_p(0x10000)
    q = C.c_void_p(0x10000 + 640)
    o = C.c_void_p(0x4000000)
    ok = dict(k=p, v=q, ld=960, B=1, H=8, W=8, C=320, f=2, method=0, out=o)
    for change, msg in ((dict(f=1), "factor"), (dict(f=5), "factor"), (dict(method=2), "method"), (dict(method=-1), "method"), (dict(C=324), "multiple of 8"),
                        (dict(C=0), "multiple of 8"), (dict(ld=964), "row stride"), (dict(ld=312), "row stride"), (dict(k=None), "null"),
                        (dict(v=None), "null"), (dict(out=None), "null"), (dict(k=C.c_void_p(0x10008)), "aligned"), (dict(out=C.c_void_p(0x4000004)), "aligned"),
                        (dict(H=1), "no complete"), (dict(W=1, f=2), "no complete"), (dict(f=4, H=3), "no complete"), (dict(B=0), "batch"),
                        (dict(out=C.c_void_p(0x10000 + 960 * 2 * 10)), "overlaps"), (dict(out=C.c_void_p(0x10000 - 64)), "overlaps")):
        a = {**ok, **change}
        assert lib.mvd_op_todo_downsample(a["k"], a["v"], a["ld"], a["B"], a["H"], a["W"], a["C"], a["f"], a["method"], a["out"], None) == -1, change
        assert msg in L.last_error(), (change, L.last_error())
    # the engine's setting: validation, the mutual refusal with token merging, and the sizing entries (dry runs, no GPU)
    rc, h = _mk_engine(lib, UNetConfig.sd21())
    assert rc == 0, L.last_error()
    for bad in ((0, 1, 0), (5, 1, 0), (2, 0, 0), (2, 5, 0), (2, 1, 2), (2, 1, -1)):
        assert lib.mvd_engine_set_todo(h, *bad) == -1 and "set_todo" in L.last_error()
    keys = (C.c_int * 16)(*([7] * 16))
    assert lib.mvd_engine_todo_keys(h, keys, 16) == 16 and list(keys) == [0] * 16          # no forward yet
    plain = lib.mvd_engine_workspace_bytes(h, 2, 64, 64, 77, 2)
    plain16 = lib.mvd_engine_workspace_bytes(h, 16, 64, 64, 77, 16)
    assert plain > 0 and plain16 > 0, L.last_error()
    assert lib.mvd_engine_set_todo(h, 2, 1, 0) == 0, L.last_error()
    on, on16 = lib.mvd_engine_workspace_bytes(h, 2, 64, 64, 77, 2), lib.mvd_engine_workspace_bytes(h, 16, 64, 64, 77, 16)
    assert on >= plain and on16 >= plain16, (on, plain, on16, plain16)       # the pooled K/V live beside the q/k/v rows: never less
    print(f"workspace, SD-2.1 at 64 x 64: batch 2 {plain} -> {on} bytes, batch 16 {plain16} -> {on16} bytes")
    assert lib.mvd_engine_set_tome(h, 0.5, 1, 0) == -1 and "alternatives" in L.last_error()
    assert lib.mvd_engine_workspace_bytes(h, 2, 64, 64, 77, 2) == on                       # the refusal changed nothing
    assert lib.mvd_engine_set_tome(h, 0.0, 1, 0) == 0                                      # ratio 0 merges nothing: no conflict
    assert lib.mvd_engine_set_todo(h, 1, 1, 1) == 0
    assert lib.mvd_engine_workspace_bytes(h, 2, 64, 64, 77, 2) == plain                    # both factors 1: the forward it always was
    assert lib.mvd_engine_set_tome(h, 0.5, 1, 0) == 0
    merged = lib.mvd_engine_workspace_bytes(h, 2, 64, 64, 77, 2)
    assert lib.mvd_engine_set_todo(h, 2, 1, 0) == -1 and "alternatives" in L.last_error()
    assert lib.mvd_engine_set_todo(h, 1, 2, 1) == -1 and "alternatives" in L.last_error()
    assert lib.mvd_engine_workspace_bytes(h, 2, 64, 64, 77, 2) == merged
    assert lib.mvd_engine_set_todo(h, 1, 1, 0) == 0                                        # (1, 1) is no downsampling: allowed beside merging
    assert lib.mvd_engine_clear_tome(h) == 0
    assert lib.mvd_engine_set_todo(h, 4, 4, 1) == 0
    assert lib.mvd_engine_workspace_bytes(h, 1, 8, 8, 77, 1) > 0, L.last_error()             # level 1 is 4 x 4: one key; deeper maps are not touched
    assert lib.mvd_engine_clear_todo(h) == 0
    assert lib.mvd_engine_workspace_bytes(h, 2, 64, 64, 77, 2) == plain
    lib.mvd_engine_destroy(h)
