"""The transformer tail as one K-concatenated GEMM on the GPU (CPU side: tests/test_tail_fold_cpu.py).

Operator level: ``out = x + [ff | h].[Wp.W2 | Wp]^T + (Wp.b2 + bp)`` -- the weight composed and rounded by the packer's own functions
-- on every kernel route the engine can give the shape, against an fp64 evaluation of the UNFUSED formula
``x + (h + ff.W2^T + b2).Wp^T + bp`` on the same bf16 inputs.  Tolerance: tests/test_cfg4_shapes_gpu.py's for a dense GEMM with a
bf16 output (``close``: max-abs <= 2^-7 max|ref|, rel-L2 <= 6e-3).  The two launches the fold replaces go through the same check
and both errors are printed.

Engine level: the tiny configuration with the fold on and off against the CPU oracle (tests/test_engine_gpu.py's bounds), the fold
twice bit for bit, and the object / ragged entries with the fold on in the sense of their own tests."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

TOL_L2, TOL_MAX = 2e-2, 5e-2          # tests/test_engine_gpu.py


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mvd_amd import ops as O
    return O


def _rnd(*shape, scale=1.0, seed=0, dtype=torch.bfloat16):
    g = torch.Generator(device="cuda").manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g, device="cuda") * scale).to(dtype)


# (route, M, C, force_cfg, split): force_cfg as mvd_op_linear takes it -- 7 the 256x320 ping-pong kernel, 10 the 128x160 lock-step tile
# with LDS-DMA staging (what the engine launches), -1 the tiled kernels' own heuristic, None / "engine": the small-M plan the engine makes
CASES = [
    ("ping-pong 256x320", 512, 320, 7, 1),              # two row tiles, 25 slabs, the second source from slab 20
    ("lock-step 128x160", 256, 640, 10, 1),             # 2 x 4 tiles, 50 slabs
    ("tiled split-K", 256, 1280, -1, "engine"),         # the heuristic's tile (64x64) and split (6 slices of 16-17 slabs; slab 80 inside the fifth)
    ("small-M", 64, 1280, None, "engine"),              # 64x64 tiles, 8 slices of 12-13 slabs combined in the kernel
    ("small-M", 1024, 640, None, "engine"),             # 160 tiles of 64x64, unsplit
]


@pytest.mark.parametrize("route,m,c,force_cfg,split", CASES, ids=[f"{r.replace(' ', '_')}-M{m}-C{c}" for r, m, c, _, _ in CASES])
def test_fused_tail_gemm_on_every_route(ops, route, m, c, force_cfg, split):
    from mvd_amd.packing import compose_tail, round_bf16
    from tests.test_cfg4_shapes_gpu import close
    ff, h, x = _rnd(m, 4 * c, seed=1), _rnd(m, c, seed=2), _rnd(m, c, seed=3)
    w2, wp = _rnd(c, 4 * c, scale=1 / math.sqrt(4 * c), seed=4), _rnd(c, c, scale=1 / math.sqrt(c), seed=5)
    b2, bp = _rnd(c, seed=6, dtype=torch.float32), _rnd(c, seed=7, dtype=torch.float32)
    want = x.double() + (h.double() + ff.double() @ w2.double().T + b2.double()) @ wp.double().T + bp.double()
    wt, bt = compose_tail(w2, b2, wp, bp)
    wt, bt = round_bf16(wt).cuda().contiguous(), bt.float().cuda()

    plan = ops.engine_dense_route(m, c, 4 * c, c)
    if route == "small-M":
        assert plan["sm"] and plan["cfg"] == 0, plan                       # the engine's own route for this shape: 64x64 tiles
        force_cfg, split = plan["force_cfg"], plan["splitk"]
        assert split == (8 if m == 64 else 1), plan
    elif split == "engine":
        split = ops.engine_splitk(m, c, 5 * c)
        assert split == 6, split
    got = ops.linear(ff, wt, bt, a2=h, res=x, force_cfg=force_cfg, splitk=split)
    ran = ops.last_gemm_plan()
    if route == "ping-pong 256x320":
        assert ran["cfg"] == 7 and ran["splitk"] == 1 and ran["tiles"] == 2, ran
    elif route == "lock-step 128x160":
        assert ran["cfg"] == 2 and ran["splitk"] == 1 and ran["tiles"] == 8, ran
    elif route == "tiled split-K":
        assert ran["cfg"] == 5 and ran["splitk"] == 6 and ran["tiles"] == 4 * 20 * 6, ran
    else:
        assert ran["cfg"] == force_cfg >= 100 and ran["splitk"] == split and ran["tiles"] == (m // 64) * (c // 64) * split, ran

    # the two launches the fold replaces, on the same route (K = 4C, then K = C)
    h1 = ops.linear(ff, w2, b2, res=h, force_cfg=force_cfg, splitk=split)
    pair = ops.linear(h1, wp, bp, res=x, force_cfg=force_cfg, splitk=split)

    def figures(t):
        d = t.double() - want
        return d.abs().max().item() / want.abs().max().item(), (d.norm() / want.norm()).item()

    (fm, fl), (pm, pl) = figures(got), figures(pair)
    print(f"tail {route} M={m} C={c} cfg={ran['cfg']} split={ran['splitk']}: fused max {fm:.3e} rel-L2 {fl:.3e} | two launches max {pm:.3e} rel-L2 {pl:.3e}"
          f" (bound {2 ** -7:.3e} / 6e-3)", flush=True)
    close(got, want, what=f"fused tail {route} M={m} C={c}")
    close(pair, want, what=f"ff2 + proj_out {route} M={m} C={c}")


# ------------------------------------------------------------------------------------------------ engine level
def _pair(fold_tail):
    """tests.parity_util.build_pair with the packing keyword"""
    from mvd_amd.config import UNetConfig
    from mvd_amd.mvd_unet import MultiViewUNet
    from oracle import mvd as OM
    from oracle import sd21_unet as OU
    ocfg = OU.UNetConfig.tiny()
    params = OM.init_mvd_params(ocfg, 0, cam_dim=96, cam_hidden=48)
    model = MultiViewUNet(None, unet_config=UNetConfig.tiny(), init="empty", img_ref_scale=0.3, cam_modulation_strength=0.2,
                          cam_output_dim=96, cam_hidden_dim=48, fold_tail=fold_tail)
    missing, unexpected = model.load_state_dict(params, strict=False)
    assert not unexpected and not missing, (unexpected[:5], missing[:5])
    return ocfg, params, model.to("cuda").eval()


@pytest.fixture(scope="module")
def pairs():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return {True: _pair(True), False: _pair(False)}


@pytest.fixture(scope="module")
def oracle_outputs():
    return {}


def _run(model, inp, t):
    model.fourier_projection = inp["proj"]
    with torch.no_grad():
        return model(inp["sample"].cuda(), t, inp["text"].cuda(), source_camera=inp["src"].cuda(), target_camera=inp["tgt"].cuda(),
                     source_image_latents=inp["lat"].cuda()).sample


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("fold", [True, False])
def test_tiny_forward_parity_with_the_fold_on_and_off(pairs, oracle_outputs, fold, batch):
    from oracle import mvd as OM
    from tests.parity_util import make_inputs, max_rel, rel_l2
    cfg, params, model = pairs[fold]
    inp = make_inputs(cfg, batch, 16, 7, seed=batch, cam_dim=96)
    t = torch.tensor(321)
    if batch not in oracle_outputs:       # (one oracle evaluation per batch, shared by both packings)
        oracle_outputs[batch] = OM.multiview_unet_forward(params, cfg, inp["sample"], t, inp["text"], inp["src"], inp["tgt"], inp["lat"],
                                                          fourier_proj=inp["proj"], img_ref_scale=0.3, cam_modulation_strength=0.2)
    want = oracle_outputs[batch]
    got = _run(model, inp, t)
    # the route follows the registered slots: a missing slot is an error, never another kernel
    slots = model._engine._weights[0]
    key = model.unet_config.transformers()[0][0]
    assert (f"{key}.tail.w" in slots) == fold and (f"{key}.ff2.w" in slots) == (not fold) and (f"{key}.proj_out.w" in slots) == (not fold)
    assert got.shape == want.shape and torch.isfinite(got).all()
    print(f"tiny forward fold={fold} batch={batch}: rel-L2 {rel_l2(got, want):.3e} max {max_rel(got, want):.3e}", flush=True)
    assert rel_l2(got, want) <= TOL_L2, (rel_l2(got, want), max_rel(got, want))
    assert max_rel(got, want) <= TOL_MAX
    if fold:
        assert torch.equal(_run(model, inp, t), got), "two forwards with the fused tail differ"


def test_fold_does_not_grow_the_engines_weight_bytes(pairs):
    for fold in (True, False):
        pairs[fold][2]._sync_engine()
    on, off = pairs[True][2]._engine.weight_bytes(), pairs[False][2]._engine.weight_bytes()
    assert on <= off, (on, off)


def test_object_and_ragged_entries_with_the_fold(pairs):
    """``mvd_unet_forward_objects`` and the ragged entry with the fused tail, as their own tests hold them: against the independent
    per-(object, view) oracle calls, batch figure and row by row; equal counts through the ragged entry are the object forward bit
    for bit."""
    from tests.objects_util import objects_case
    from tests.parity_util import max_rel, rel_l2
    from tests.ragged_util import per_row, ragged_case
    _, _, model = pairs[True]

    def call(c, **kw):
        model.fourier_projection = c.proj
        with torch.no_grad():
            return model(c.sample.cuda(), c.t, c.text.cuda(), source_camera=c.src.cuda(), target_camera=c.tgt.cuda(),
                         source_image_latents=c.lat.cuda(), **kw).sample

    c = objects_case(2, 2, 1, 16, 0.3)
    got = call(c, views=c.V, objects=c.O)
    rows = [rel_l2(got[r], c.want[r]) for r in range(c.g * c.O * c.V)]
    print(f"object forward with the fold: rel-L2 {rel_l2(got, c.want):.3e} max {max_rel(got, c.want):.3e} rows {rows}", flush=True)
    assert rel_l2(got, c.want) <= TOL_L2 and max_rel(got, c.want) <= TOL_MAX and max(rows) <= 2 * TOL_L2
    assert torch.equal(call(c, views=(c.V,) * c.O), got)

    r = ragged_case((3, 1), 1, 16, 0.3)
    got = call(r, views=r.counts)
    rows = per_row(got, r.want)
    print(f"ragged forward with the fold: rel-L2 {rel_l2(got, r.want):.3e} max {max_rel(got, r.want):.3e} rows {rows}", flush=True)
    assert rel_l2(got, r.want) <= TOL_L2 and max_rel(got, r.want) <= TOL_MAX and max(rows) <= 2 * TOL_L2
