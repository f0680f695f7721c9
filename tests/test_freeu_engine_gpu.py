"""FreeU in the engine's main pass (``mvd_engine_set_freeu``) on the MI355X, tiny topology, against the
FreeU oracle of tests/freeu_ref.py (the oracle's own forward with FreeU in front of the resnets of up blocks 0 and 1).

The parity bound is measured, not fixed: the rel-L2 of the SAME inputs with FreeU off against the plain oracle (the parent's
figure for that case), times 1.5 -- amplified backbone channels amplify the bf16 error they carry -- and never more than 3e-2
(``freeu_ref.PARITY_BOUND_MAX``).  The parity setting is ``freeu_ref.PARITY_SETTING``: tests/test_freeu_cpu.py shows that under it
every wrong function (FreeU off, on blocks 0-2, b only, s only, the flipped (1, 1) mode, the two blocks' values swapped) is at
least four times that bound away, which the published SD-2.1 setting does not give on this topology; the SD-2.1 setting is held
to the same bound.

Measured on one MI355X (rel-L2; off = FreeU off vs the plain oracle -> bound; on = FreeU on vs the FreeU oracle, parity / SD-2.1 setting):
  16 x 16: off 1.349e-2 -> 2.023e-2, on 1.427e-2 / 1.342e-2;  16 x 32: off 1.399e-2 -> 2.098e-2, on 1.489e-2 / 1.402e-2;
  48 x 48: off 1.301e-2 -> 1.951e-2, on 1.374e-2 / 1.298e-2;  ragged (2, 1), g = 2: off 1.277e-2 -> 1.916e-2, on 1.436e-2;
  batch 1: off 1.308e-2 -> 1.962e-2, on 1.588e-2 (1.616e-2 to the forward without the batch-1 kernels);
  generate_views: 2.30e-2 to the FreeU oracle loops, 1.44e-1 to the loops without FreeU."""
import pytest
import torch

from tests import freeu_ref as FR

pytestmark = pytest.mark.gpu


def _pair():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tests.parity_util import build_pair
    return build_pair("tiny", 0, 96, 48, img_ref_scale=0.3)


@pytest.fixture(scope="module")
def tiny():
    return _pair()


def _oracle(params, cfg, inp, t=500, rows=slice(None)):
    from oracle import mvd as OM
    return OM.multiview_unet_forward(params, cfg, inp["sample"][rows], torch.tensor(t), inp["text"][rows], inp["src"][rows], inp["tgt"][rows],
                                     inp["lat"][rows], fourier_proj=inp["proj"], img_ref_scale=0.3, cam_modulation_strength=0.2)


def _engine(model, inp, t=500, rows=slice(None)):
    model.fourier_projection = inp["proj"]
    with torch.no_grad():
        return model(inp["sample"][rows].cuda(), torch.tensor(t), inp["text"][rows].cuda(), source_camera=inp["src"][rows].cuda(),
                     target_camera=inp["tgt"][rows].cuda(), source_image_latents=inp["lat"][rows].cuda()).sample.clone()


def _bound(off_err):
    return min(1.5 * off_err, FR.PARITY_BOUND_MAX)


@pytest.mark.parametrize("hw", [16, (16, 32), 48], ids=["16x16", "16x32", "48x48"])
def test_freeu_forward_matches_the_freeu_oracle(tiny, hw):
    """batch 2, camera and image conditioning; 48 x 48 latents give 6 x 6 and 12 x 12 maps (the 768 x 768 image in small)"""
    from tests.parity_util import make_inputs, max_rel, rel_l2
    cfg, params, model = tiny
    inp = make_inputs(cfg, 2, hw, 7, 0, 96)
    try:
        model.disable_freeu()
        off = rel_l2(_engine(model, inp), _oracle(params, cfg, inp))
        bound = _bound(off)
        for name, setting in (("parity", FR.PARITY_SETTING), ("sd21", FR.SD21)):
            with FR.freeu_oracle(**setting):
                want = _oracle(params, cfg, inp)
            model.enable_freeu(**setting)
            got = _engine(model, inp)
            assert got.shape == want.shape and torch.isfinite(got).all()
            err = rel_l2(got, want)
            print(f"freeu forward hw={hw} {name} {setting}: FreeU off {off:.3e}, bound {bound:.3e}, FreeU on rel-L2 {err:.3e} max {max_rel(got, want):.3e}", flush=True)
            assert err <= bound, (name, err, bound, off)
    finally:
        model.disable_freeu()


def test_freeu_ragged_forward_matches_the_freeu_oracle(tiny):
    """views = (2, 1), g = 2: the ragged forward with FreeU is the three independent FreeU oracle calls"""
    from tests.parity_util import rel_l2
    from tests.ragged_util import per_row, ragged_case
    _, _, model = tiny
    plain = ragged_case((2, 1), 2, 16, 0.3)
    with FR.freeu_oracle(**FR.PARITY_SETTING):
        c = ragged_case.__wrapped__((2, 1), 2, 16, 0.3)          # (not the cached plain case)

    def fwd(case):
        model.fourier_projection = case.proj
        with torch.no_grad():
            return model(case.sample.cuda(), case.t, case.text.cuda(), source_camera=case.src.cuda(), target_camera=case.tgt.cuda(),
                         source_image_latents=case.lat.cuda(), views=case.counts).sample.clone()
    try:
        model.disable_freeu()
        off = rel_l2(fwd(plain), plain.want)
        bound = _bound(off)
        model.enable_freeu(**FR.PARITY_SETTING)
        got = fwd(c)
        err, rows = rel_l2(got, c.want), per_row(got, c.want)
        print(f"freeu ragged (2, 1) g=2: FreeU off {off:.3e}, bound {bound:.3e}, FreeU on {err:.3e}; per row " + " ".join(f"{e:.2e}" for e in rows), flush=True)
        assert err <= bound, (err, bound)
        assert max(rows) <= 2 * bound, rows
        assert rel_l2(got, plain.want) >= 4 * bound
    finally:
        model.disable_freeu()


def test_clear_and_identity_setting_are_the_plain_forward_bit_for_bit(tiny):
    """FreeU clear after having been set == a fresh engine's forward; set_freeu(1, 1, 1, 1) == clear"""
    from tests.parity_util import make_inputs
    cfg, _, model = tiny
    inp = make_inputs(cfg, 2, 16, 7, 3, 96)
    _, _, fresh = _pair()
    want = _engine(fresh, inp)
    assert fresh._engine.freeu is None
    try:
        model.enable_freeu(**FR.SD21)
        on = _engine(model, inp)
        assert model._engine.freeu == (0.9, 0.2, 1.4, 1.6)
        model.disable_freeu()
        assert torch.equal(_engine(model, inp), want)
        assert model._engine.freeu is None
        model.enable_freeu(1.0, 1.0, 1.0, 1.0)
        assert torch.equal(_engine(model, inp), want)
        assert not torch.equal(on, want)
    finally:
        model.disable_freeu()


def test_reference_cache_does_not_depend_on_freeu():
    """a cold FreeU forward, then MVD_REUSE_REF forwards after toggling FreeU off and on: each equals its own cold result"""
    from tests.parity_util import make_inputs
    cfg, _, model = _pair()                                  # a fresh engine: its workspace is sized by this test's forwards alone
    inp = make_inputs(cfg, 2, 16, 7, 4, 96)
    x, text = inp["sample"].cuda(), inp["text"].cuda()
    kw = dict(source_camera=inp["src"].cuda(), target_camera=inp["tgt"].cuda(), source_image_latents=inp["lat"].cuda())
    model.fourier_projection = inp["proj"]

    def fwd(t):
        with torch.no_grad():
            return model(x, torch.tensor(t), text, **kw).sample.clone()
    model.cache_reference = False
    model.enable_freeu(**FR.SD21)
    cold_on = fwd(500)
    model.disable_freeu()
    cold_off = fwd(500)
    eng = model._engine
    calls, forward = [], eng.forward
    eng.forward = lambda *a, **k: (calls.append(bool(k.get("reuse_ref"))), forward(*a, **k))[1]
    try:
        model.cache_reference = True
        model.reset_reference_cache()
        model.enable_freeu(**FR.SD21)
        fwd(900)                                             # cold, FreeU on: fills the cache
        warm_on = fwd(500)
        model.disable_freeu()
        warm_off = fwd(500)
        model.enable_freeu(**FR.SD21)
        warm_on2 = fwd(500)
    finally:
        eng.forward = forward
        model.cache_reference = False
        model.disable_freeu()
    assert calls == [False, True, True, True], calls
    assert torch.equal(warm_on, cold_on) and torch.equal(warm_on2, cold_on) and torch.equal(warm_off, cold_off)
    assert not torch.equal(cold_on, cold_off)


def test_hip_graph_replay_with_freeu_and_after_clear(tiny):
    """replay with FreeU on is bit-exact against plain launches; after clear the next forward is the plain result, not a stale replay"""
    from tests.parity_util import make_inputs
    cfg, _, model = tiny
    inp = make_inputs(cfg, 2, 16, 7, 5, 96)
    try:
        model.use_hip_graph = False
        model.cache_reference = False
        model.disable_freeu()
        want_off = _engine(model, inp)
        model.enable_freeu(**FR.SD21)
        want_on = _engine(model, inp)
        model.use_hip_graph = True
        got_on = [_engine(model, inp) for _ in range(4)]                  # run, capture, replay, replay
        model.disable_freeu()
        got_off = [_engine(model, inp) for _ in range(3)]
        model.enable_freeu(**FR.SD21)
        again_on = [_engine(model, inp) for _ in range(3)]
    finally:
        model.use_hip_graph = False
        model.disable_freeu()
    assert not torch.equal(want_on, want_off)
    for i, g in enumerate(got_on + again_on):
        assert torch.equal(g, want_on), i
    for i, g in enumerate(got_off):
        assert torch.equal(g, want_off), i


def test_batch_one_routes(tiny):
    """a batch-1 forward with FreeU set (the small-M / weight-streaming kernels) against the FreeU oracle, and against the same forward
    with the batch-1 kernels off (debug flag NO_SM = 4), inside the parity bound"""
    from mvd_amd import _lib as L
    from tests.parity_util import make_inputs, rel_l2
    cfg, params, model = tiny
    inp = make_inputs(cfg, 2, 16, 7, 6, 96)
    one = slice(0, 1)
    try:
        model.disable_freeu()
        off = rel_l2(_engine(model, inp, rows=one), _oracle(params, cfg, inp, rows=one))
        bound = _bound(off)
        with FR.freeu_oracle(**FR.PARITY_SETTING):
            want = _oracle(params, cfg, inp, rows=one)
        model.enable_freeu(**FR.PARITY_SETTING)
        got = _engine(model, inp, rows=one)
        L.call("mvd_debug_set_flags", int(L.DebugFlag.NO_SM))
        try:
            tiled = _engine(model, inp, rows=one)
        finally:
            L.call("mvd_debug_set_flags", 0)
        e_oracle, e_tiled = rel_l2(got, want), rel_l2(got, tiled.cpu())
        print(f"freeu batch 1: FreeU off {off:.3e}, bound {bound:.3e}, FreeU on {e_oracle:.3e} to the oracle, {e_tiled:.3e} to the forward "
              "without the batch-1 kernels", flush=True)
        assert e_oracle <= bound and e_tiled <= bound, (e_oracle, e_tiled, bound)
    finally:
        model.disable_freeu()


def test_engine_refuses_a_one_pixel_map(tiny):
    """8 x 8 latents put a 1 x 1 map in up block 0: refused by the forward's own checks, before anything is launched"""
    from mvd_amd._lib import MvdError
    from tests.parity_util import make_inputs
    cfg, _, model = tiny
    inp = make_inputs(cfg, 2, 8, 7, 7, 96)
    try:
        model.enable_freeu(**FR.SD21)
        with pytest.raises(MvdError, match="FreeU needs maps of at least 2 x 2"):
            _engine(model, inp)
    finally:
        model.disable_freeu()


def test_pipeline_generate_views_with_freeu(tiny):
    """``pipe.enable_freeu`` then ``generate_views`` (DDIM, 4 steps, 2 views, guidance 3.0) against the per-view oracle loops run
    under the FreeU oracle: within 4e-2 (the loop bound of tests/test_ragged_gpu.py), and at least twice that from the loops
    WITHOUT FreeU (0.142 between the two oracle loops)."""
    from mvd_amd.config import UNetConfig
    from mvd_amd.mvd_unet import create_mvd_pipeline
    from mvd_amd.utils import orbit_cameras
    from tests import sampler_ref as R
    from tests.parity_util import make_inputs, rel_l2
    cfg, params, _ = tiny
    pipe = create_mvd_pipeline(None, dtype=torch.float32, img_ref_scale=0.3, cam_modulation_strength=0.2, cam_output_dim=96,
                               cam_hidden_dim=48, unet_config=UNetConfig.tiny(), init="empty", sampler="ddim")
    missing, unexpected = pipe.unet.load_state_dict(params, strict=False)
    assert not missing and not unexpected
    pipe = pipe.to("cuda")
    pipe.unet.eval()
    V, steps, gs = 2, 4, 3.0
    inp = make_inputs(cfg, 1, 16, 7, seed=23, cam_dim=96)
    g = torch.Generator().manual_seed(6)
    neg = torch.randn(1, 7, cfg.cross_attention_dim, generator=g)
    lat0 = torch.randn(V, 4, 16, 16, generator=g)
    src, tgt = orbit_cameras(1), orbit_cameras(V, elevation_deg=15.0, start_deg=40.0)
    sc = pipe.scheduler.config
    ts = R.timesteps("ddim", sc.num_train_timesteps, steps, sc.timestep_spacing, sc.steps_offset)

    def loops():
        return torch.cat([R.denoise_loop(params, cfg, pipe.scheduler.betas, inp["text"], neg, lat0[v:v + 1], src, tgt[v:v + 1], inp["lat"],
                                         "ddim", ts, gs, [inp["proj"]] * steps, set_alpha_to_one=getattr(sc, "set_alpha_to_one", True),
                                         img_ref_scale=0.3, cam_modulation_strength=0.2) for v in range(V)])
    plain = loops()
    with FR.freeu_oracle(**FR.SD21):
        want = loops()
    pipe.unet.fourier_projection = inp["proj"]
    pipe.unet.cache_reference = True
    pipe.enable_freeu(**FR.SD21)
    assert pipe.unet.freeu == (0.9, 0.2, 1.4, 1.6)
    got = pipe.generate_views(source_camera=src[0], target_cameras=tgt, latents=lat0.cuda(), prompt_embeds=inp["text"].cuda(),
                              negative_prompt_embeds=neg.cuda(), num_inference_steps=steps, guidance_scale=gs,
                              source_image_latents=inp["lat"].cuda(), output_type="latent")["images"]
    assert pipe.unet._engine.freeu == (0.9, 0.2, 1.4, 1.6)
    pipe.disable_freeu()
    e_on, e_plain = rel_l2(got, want), rel_l2(got, plain)
    print(f"generate_views with FreeU: rel-L2 {e_on:.3e} to the FreeU oracle loops, {e_plain:.3e} to the loops without FreeU", flush=True)
    assert got.shape == lat0.shape and torch.isfinite(got).all()
    assert e_on <= 4e-2, e_on
    assert e_plain >= 2 * 4e-2, e_plain
