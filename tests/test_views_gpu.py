"""V views of one object in one forward (N14, ``MultiViewUNet.forward(..., views=V)`` / ``MVDPipeline.generate_views``) on the GPU
against the CPU oracle.  The shared forward is DEFINED as V independent forwards of batch g with a one-row reference
(tests/views_util.py computes exactly that on the oracle), so every comparison here is against the per-view calls.

Tolerances: test_engine_gpu.py's (rel-L2 <= 2e-2, max <= 5e-2 max|ref|) for one forward; 4e-2 for four chained forwards
(test_tiny_denoise_loop_parity), twice that between two GPU results that are each within 4e-2 of the oracle."""
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL_L2, TOL_MAX = 2e-2, 5e-2          # tests/test_engine_gpu.py


def _pair(img_ref_scale):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tests.parity_util import build_pair
    return build_pair("tiny", 0, 96, 48, img_ref_scale=img_ref_scale)


@pytest.fixture(scope="module")
def tiny():
    return _pair(0.3)


@pytest.fixture(scope="module")
def tiny_full_scale():
    return _pair(1.0)


def _shared(model, c, **kw):
    model.fourier_projection = c.proj
    with torch.no_grad():
        return model(c.sample.cuda(), c.t, c.text.cuda(), source_camera=c.src.cuda(), target_camera=c.tgt.cuda(),
                     source_image_latents=kw.pop("lat", c.lat.cuda()), views=c.V, **kw).sample


# (3, *) is what the ordinary path cannot express: 3 divides no level's reference tokens
@pytest.mark.parametrize("V,g,hw", [(3, 1, 16), (4, 1, 16), (3, 2, 16), (4, 2, (16, 32)), (5, 2, 16)])
def test_shared_forward_matches_the_independent_oracle_calls(tiny, V, g, hw):
    from tests.parity_util import max_rel, rel_l2
    from tests.views_util import views_case
    _, _, model = tiny
    c = views_case(V, g, hw, 0.3)
    got = _shared(model, c)
    assert got.shape == c.want.shape and torch.isfinite(got).all()
    err, emax = rel_l2(got, c.want), max_rel(got, c.want)
    print(f"shared forward V={V} g={g} hw={hw}: rel-L2 {err:.3e} max {emax:.3e}", flush=True)
    assert err <= TOL_L2, (err, emax)
    assert emax <= TOL_MAX, emax
    # Row by row: a row answered with another view's camera or the other guidance half hides in the batch figure (one row of
    # ten at ~5e-2 moves it by 1.6e-2).  Each row is a forward of its own; its error may exceed the batch's by the spread
    # between rows, for which a factor of two is allowed.
    per_row = [rel_l2(got[r], c.want[r]) for r in range(g * V)]
    print("  per row:", " ".join(f"{e:.2e}" for e in per_row), flush=True)
    assert max(per_row) <= 2 * TOL_L2, per_row


@pytest.mark.parametrize("V", [3, 5])
def test_shared_forward_is_not_a_repeated_source_batch(tiny_full_scale, V):
    """img_ref_scale = 1.0, g = 2: the shared forward is closer to the independent calls than half the distance of the nearer
    wrong batching (source repeated V or 2V times, both on the oracle: tests/test_views_cpu.py holds them >= 8e-2 away), and
    closer than either of them.  Measured on the MI355X: see DESIGN.md section 9 N14."""
    from tests.parity_util import rel_l2
    from tests.views_util import views_case
    _, _, model = tiny_full_scale
    c = views_case(V, 2, 16, 1.0, True)
    got = _shared(model, c)
    err = rel_l2(got, c.want)
    print(f"shared forward V={V} g=2 img_ref_scale=1.0: rel-L2 {err:.3e}; wrong batchings {c.d_rep_v:.3e} / {c.d_rep_gv:.3e}", flush=True)
    assert torch.isfinite(got).all()
    assert err < 0.5 * min(c.d_rep_v, c.d_rep_gv), (err, c.d_rep_v, c.d_rep_gv)
    assert err < rel_l2(c.rep_v, c.want) and err < rel_l2(c.rep_gv, c.want)
    # and from the other side: the GPU result is far from both wrong batchings
    assert rel_l2(got, c.rep_v) > 0.5 * c.d_rep_v and rel_l2(got, c.rep_gv) > 0.5 * c.d_rep_gv


def test_shared_forward_reference_cache_is_exact_and_one_row():
    """Q5 with views: a second shared forward at another timestep is served from the cached reference K/V, bit-identical to
    recomputing them; the engine's reference cache is the ref_batch = 1 one (one copy of the K/V, not V)."""
    from mvd_amd import _lib as L
    from tests.views_util import views_case
    _, _, model = _pair(0.3)                       # a fresh engine: its buffers are sized by this test's forwards alone
    c = views_case(4, 2, 16, 0.3)
    lat = c.lat.cuda()
    model.cache_reference = False
    a = _shared(model, c, lat=lat)
    eng = model._engine
    model.reset_reference_cache()                  # (the calls below start without a cached reference, whatever addresses their tensors get)
    calls = []
    fwd = eng.forward
    eng.forward = lambda *args, **kw: (calls.append(bool(kw.get("reuse_ref"))), fwd(*args, **kw))[1]
    try:
        model.cache_reference = True
        text = c.text.cuda()
        with torch.no_grad():
            kw = dict(source_camera=c.src.cuda(), target_camera=c.tgt.cuda(), source_image_latents=lat, views=c.V)
            model(c.sample.cuda(), torch.tensor(900), text, **kw)
            b = model(c.sample.cuda(), c.t, text, **kw).sample                 # served from the cache
            plain = model(c.sample[[0, 4]].cuda(), c.t, text, source_camera=c.src[:1].cuda(), target_camera=c.tgt[:1].cuda(),
                          source_image_latents=lat).sample                     # another mode on the same tensors: no hit
    finally:
        eng.forward = fwd
        model.cache_reference = False
    assert calls == [False, True, False], calls
    assert torch.equal(a, b)
    assert torch.isfinite(plain).all()
    one = L.lib().mvd_engine_refcache_bytes(eng._h, 1, 16, 16, 0)
    assert eng._rc.numel() == one and one < L.lib().mvd_engine_refcache_bytes(eng._h, 4, 16, 16, 0)


def test_views_none_and_one_are_the_ordinary_forward(tiny):
    from tests.views_util import views_case
    _, _, model = tiny
    c = views_case(3, 2, 16, 0.3)
    model.fourier_projection = c.proj
    x = c.sample[[0, 3]].cuda()
    kw = dict(source_camera=c.src[:1].cuda(), target_camera=c.tgt[:1].cuda(), source_image_latents=c.lat.cuda())
    with torch.no_grad():
        today = model(x, c.t, c.text.cuda(), **kw).sample
        none = model(x, c.t, c.text.cuda(), **kw, views=None).sample
        one = model(x, c.t, c.text.cuda(), **kw, views=1).sample
    assert torch.equal(today, none) and torch.equal(today, one)


def test_shared_forward_hip_graph_replay_is_bit_exact(tiny):
    """``use_hip_graph`` with views: run, capture (both stream branches), replay, replay on refreshed inputs -- bit-identical to
    the plain launches (the graph key carries ``views`` and the flag: the batch-2 graph of the same engine is another one)."""
    from tests.views_util import views_case
    _, _, model = tiny
    c = views_case(3, 2, 16, 0.3)
    model.fourier_projection = c.proj
    xs = [(c.sample * s).cuda() for s in (1.0, 0.5, 0.25, 2.0)]
    text, lat, src, tgt = c.text.cuda(), c.lat.cuda(), c.src.cuda(), c.tgt.cuda()

    def fwd(x, t, views):
        rows = slice(None) if views else [0, 3]
        cams = dict(source_camera=src if views else src[:1], target_camera=tgt if views else tgt[:1])
        with torch.no_grad():
            return model(x[rows], torch.tensor(t), text, source_image_latents=lat, views=views, **cams).sample.clone()

    try:
        model.use_hip_graph = False
        model.cache_reference = False
        want = [fwd(x, 100 + 50 * i, 3) for i, x in enumerate(xs)]
        want_plain = [fwd(x, 100 + 50 * i, None) for i, x in enumerate(xs[:3])]
        model.use_hip_graph = True
        got = [fwd(x, 100 + 50 * i, 3) for i, x in enumerate(xs)]
        got_plain = [fwd(x, 100 + 50 * i, None) for i, x in enumerate(xs[:3])]
    finally:
        model.use_hip_graph = False
    for a, b in zip(got + got_plain, want + want_plain):
        assert torch.equal(a, b)


def test_views_rejections_in_python(tiny):
    from mvd_amd._lib import MvdError
    from tests.views_util import views_case
    _, _, model = tiny
    c = views_case(3, 2, 16, 0.3)
    kw = dict(source_camera=c.src.cuda(), target_camera=c.tgt.cuda())
    with torch.no_grad():
        with pytest.raises(MvdError, match="reference_stats_group"):
            model.reference_stats_group = True
            try:
                model(c.sample.cuda(), c.t, c.text.cuda(), source_image_latents=c.lat.cuda(), views=3, **kw)
            finally:
                model.reference_stats_group = None
        with pytest.raises(MvdError, match="ONE row"):
            model(c.sample.cuda(), c.t, c.text.cuda(), source_image_latents=c.lat.repeat(3, 1, 1, 1).cuda(), views=3, **kw)
        with pytest.raises(MvdError, match="g \\* views"):
            model(c.sample.cuda(), c.t, c.text.repeat(3, 1, 1).cuda(), source_image_latents=c.lat.cuda(), views=3, **kw)


def _ddim_pipe(params):
    from mvd_amd.config import UNetConfig
    from mvd_amd.mvd_unet import create_mvd_pipeline
    pipe = create_mvd_pipeline(None, dtype=torch.float32, img_ref_scale=0.3, cam_modulation_strength=0.2, cam_output_dim=96,
                               cam_hidden_dim=48, unet_config=UNetConfig.tiny(), init="empty", sampler="ddim")
    missing, unexpected = pipe.unet.load_state_dict(params, strict=False)
    assert not missing and not unexpected
    pipe = pipe.to("cuda")
    pipe.unet.eval()
    return pipe


@pytest.fixture(scope="module")
def ddim_pipe(tiny):
    return _ddim_pipe(tiny[1])


@pytest.mark.parametrize("gs", [1.0, 3.0])
def test_generate_views_matches_the_per_view_loops(tiny, ddim_pipe, gs):
    """``generate_views`` (DDIM, 4 steps, V = 3, explicit latents) against the per-view oracle loop (oracle.mvd forward + the
    fp64 DDIM step of tests/sampler_ref.py, one view at a time) within 4e-2, and against V separate ``pipe(...)`` calls with
    the same latents within twice that."""
    from mvd_amd.utils import orbit_cameras
    from tests import sampler_ref as R
    from tests.parity_util import make_inputs, rel_l2
    cfg, params, _ = tiny
    pipe = ddim_pipe
    V, steps = 3, 4
    inp = make_inputs(cfg, 1, 16, 7, seed=23, cam_dim=96)
    g = torch.Generator().manual_seed(6)
    neg = torch.randn(1, 7, cfg.cross_attention_dim, generator=g)
    lat0 = torch.randn(V, 4, 16, 16, generator=g)
    src = orbit_cameras(1)                                   # (1, 3, 4): infer.py's source position
    tgt = orbit_cameras(V, elevation_deg=15.0, start_deg=40.0)
    sc = pipe.scheduler.config
    ts = R.timesteps("ddim", sc.num_train_timesteps, steps, sc.timestep_spacing, sc.steps_offset)
    want = torch.cat([R.denoise_loop(params, cfg, pipe.scheduler.betas, inp["text"], neg, lat0[v:v + 1], src, tgt[v:v + 1], inp["lat"],
                                     "ddim", ts, gs, [inp["proj"]] * steps, set_alpha_to_one=getattr(sc, "set_alpha_to_one", True),
                                     img_ref_scale=0.3, cam_modulation_strength=0.2) for v in range(V)])
    pipe.unet.fourier_projection = inp["proj"]
    pipe.unet.cache_reference = True
    common = dict(prompt_embeds=inp["text"].cuda(), negative_prompt_embeds=neg.cuda(), num_inference_steps=steps, guidance_scale=gs,
                  source_image_latents=inp["lat"].cuda(), output_type="latent")
    got = pipe.generate_views(source_camera=src[0], target_cameras=tgt, latents=lat0.cuda(), **common)["images"]
    assert pipe.scheduler.timesteps.tolist() == ts.tolist()
    per_view = torch.cat([pipe(source_camera=src, target_camera=tgt[v:v + 1], latents=lat0[v:v + 1].cuda(), **common)["images"]
                          for v in range(V)])
    pipe.unet.cache_reference = False
    assert got.shape == lat0.shape and torch.isfinite(got).all()
    e_oracle, e_calls = rel_l2(got, want), rel_l2(got, per_view.cpu())
    print(f"generate_views gs={gs}: rel-L2 {e_oracle:.3e} to the per-view oracle loops, {e_calls:.3e} to the per-view pipe calls", flush=True)
    assert e_oracle <= 4e-2, e_oracle
    assert e_calls <= 8e-2, e_calls


def test_generate_views_latents_from_a_list_of_generators(ddim_pipe):
    """initial latents from a list of V generators equal the per-view calls' latents (row v = generator v's own draw)"""
    pipe = ddim_pipe
    V = 3
    shape = (pipe.unet.config.sample_size * pipe.vae_scale_factor,) * 2
    mk = lambda: [torch.Generator().manual_seed(100 + v) for v in range(V)]      # noqa: E731
    rows = pipe.prepare_latents(V, 4, *shape, torch.float32, pipe.device, mk())
    for v, gen in enumerate(mk()):
        assert torch.equal(rows[v:v + 1], pipe.prepare_latents(1, 4, *shape, torch.float32, pipe.device, gen))
