"""O objects x V views in one forward (N15, ``MultiViewUNet.forward(..., views=V, objects=O)`` /
``MVDPipeline.generate_views_batch``) on the GPU against the CPU oracle.  The object forward is DEFINED as O V independent forwards
of batch g with a one-row reference (tests/objects_util.py computes exactly that on the oracle), so every comparison here is
against the per-(object, view) calls.

Tolerances: test_views_gpu.py's -- rel-L2 <= 2e-2, max <= 5e-2 max|ref|, every single row <= 4e-2 for one forward; 4e-2 for four
chained forwards, twice that between two GPU results that are each within 4e-2 of the oracle."""
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


def _objects(model, c, **kw):
    model.fourier_projection = c.proj
    with torch.no_grad():
        return model(c.sample.cuda(), c.t, c.text.cuda(), source_camera=c.src.cuda(), target_camera=c.tgt.cuda(),
                     source_image_latents=kw.pop("lat", c.lat.cuda()), views=c.V, objects=c.O, **kw).sample


@pytest.mark.parametrize("O,V,g,hw", [(2, 2, 1, 16), (3, 2, 1, 16), (2, 3, 2, 16), (3, 2, 2, (16, 32))])
def test_object_forward_matches_the_independent_oracle_calls(tiny, O, V, g, hw):
    from tests.parity_util import max_rel, rel_l2
    from tests.objects_util import objects_case
    _, _, model = tiny
    c = objects_case(O, V, g, hw, 0.3)
    got = _objects(model, c)
    assert got.shape == c.want.shape and torch.isfinite(got).all()
    err, emax = rel_l2(got, c.want), max_rel(got, c.want)
    print(f"object forward O={O} V={V} g={g} hw={hw}: rel-L2 {err:.3e} max {emax:.3e}", flush=True)
    per_row = [rel_l2(got[r], c.want[r]) for r in range(g * O * V)]
    print("  per row:", " ".join(f"{e:.2e}" for e in per_row), flush=True)
    assert err <= TOL_L2, (err, emax)
    assert emax <= TOL_MAX, emax
    # row by row (a row answered with another object's reference, camera or text hides in the batch figure)
    assert max(per_row) <= 2 * TOL_L2, per_row


@pytest.mark.parametrize("O,V,g,amp", [(3, 2, 1, 8.0), (2, 3, 2, 1.0)])
def test_object_forward_is_not_a_wrong_batching(tiny_full_scale, O, V, g, amp):
    """img_ref_scale = 1.0, the two cases whose oracle distances tests/test_objects_cpu.py holds: the object forward is closer to
    the independent calls than half the distance of the nearest wrong result (the ordinary batch with the sources repeated
    O V or g O V times -- coupled Q2 statistics, and under guidance Q4 over the wrong rows -- and object o answered from object
    o + 1's reference), closer than each of them, and further than half that distance from each."""
    from tests.parity_util import rel_l2
    from tests.objects_util import objects_case
    _, _, model = tiny_full_scale
    c = objects_case(O, V, g, 16, 1.0, amp, True)
    got = _objects(model, c)
    err = rel_l2(got, c.want)
    wrong = dict(rep_v=c.d_rep_v, rep_gv=c.d_rep_gv, swapped=c.d_swapped)
    print(f"object forward O={O} V={V} g={g} amp={amp} img_ref_scale=1.0: rel-L2 {err:.3e}; wrong results "
          + " / ".join(f"{k} {d:.3e}" for k, d in wrong.items()), flush=True)
    assert torch.isfinite(got).all()
    assert err < 0.5 * min(wrong.values()), (err, wrong)
    for name, d in wrong.items():
        assert err < d, (name, err, d)
        assert rel_l2(got, getattr(c, name)) > 0.5 * d, (name, rel_l2(got, getattr(c, name)), d)


def test_object_forward_reference_cache_is_exact_and_one_row_per_object():
    """Q5 with objects: a second object forward at another timestep is served from the cached reference K/V, bit-identical to
    recomputing them; the engine's reference cache is the ref_batch = O one (one copy of the K/V per object, not per view);
    the shared forward of ONE of the objects on the same tensors' rows is another mode and does not hit."""
    from mvd_amd import _lib as L
    from tests.objects_util import objects_case
    _, _, model = _pair(0.3)                       # a fresh engine: its buffers are sized by this test's forwards alone
    c = objects_case(2, 3, 2, 16, 0.3)
    lat = c.lat.cuda()
    model.cache_reference = False
    a = _objects(model, c, lat=lat)
    eng = model._engine
    model.reset_reference_cache()
    calls = []
    fwd = eng.forward
    eng.forward = lambda *args, **kw: (calls.append(bool(kw.get("reuse_ref"))), fwd(*args, **kw))[1]
    try:
        model.cache_reference = True
        text = c.text.cuda()
        with torch.no_grad():
            kw = dict(source_camera=c.src.cuda(), target_camera=c.tgt.cuda(), source_image_latents=lat, views=c.V, objects=c.O)
            model(c.sample.cuda(), torch.tensor(900), text, **kw)
            b = model(c.sample.cuda(), c.t, text, **kw).sample                 # served from the cache
            b2 = model(c.sample.cuda(), c.t, text, **kw).sample                # and again
            rows = [0, 1, 2, 6, 7, 8]                                            # object 0's rows of both halves
            one = model(c.sample[rows].cuda(), c.t, text[[0, 2]], source_camera=c.src[:3].cuda(), target_camera=c.tgt[:3].cuda(),
                        source_image_latents=lat[:1], views=c.V).sample          # another mode: no hit
    finally:
        eng.forward = fwd
        model.cache_reference = False
    assert calls == [False, True, True, False], calls
    assert torch.equal(a, b) and torch.equal(a, b2)
    # the shared forward of object 0 alone is the same function of object 0's rows (other launch shapes: to tolerance)
    from tests.parity_util import rel_l2
    assert rel_l2(one, c.want[rows]) <= TOL_L2
    two = L.lib().mvd_engine_refcache_bytes(eng._h, 2, 16, 16, 0)
    assert eng._rc.numel() == two and two < L.lib().mvd_engine_refcache_bytes(eng._h, 6, 16, 16, 0)


def test_objects_none_and_one_are_the_shared_forward(tiny):
    from tests.views_util import views_case
    _, _, model = tiny
    c = views_case(3, 2, 16, 0.3)
    model.fourier_projection = c.proj
    kw = dict(source_camera=c.src.cuda(), target_camera=c.tgt.cuda(), source_image_latents=c.lat.cuda())
    with torch.no_grad():
        today = model(c.sample.cuda(), c.t, c.text.cuda(), **kw, views=3).sample
        none = model(c.sample.cuda(), c.t, c.text.cuda(), **kw, views=3, objects=None).sample
        one = model(c.sample.cuda(), c.t, c.text.cuda(), **kw, views=3, objects=1).sample
        x = c.sample[[0, 3]].cuda()
        kw1 = dict(source_camera=c.src[:1].cuda(), target_camera=c.tgt[:1].cuda(), source_image_latents=c.lat.cuda())
        plain = model(x, c.t, c.text.cuda(), **kw1).sample
        plain_one = model(x, c.t, c.text.cuda(), **kw1, objects=1).sample
    assert torch.equal(today, none) and torch.equal(today, one)
    assert torch.equal(plain, plain_one)


def test_object_forward_hip_graph_replay_is_bit_exact(tiny):
    """``use_hip_graph`` with objects: run, capture (both stream branches), replay, replay on refreshed inputs -- bit-identical to
    the plain launches; the graph key carries ``objects``: the shared forward with the same argument block (batch, views,
    ref_batch aside) on the same engine is another graph."""
    from tests.objects_util import objects_case
    _, _, model = tiny
    c = objects_case(2, 3, 2, 16, 0.3)
    model.fourier_projection = c.proj
    xs = [(c.sample * s).cuda() for s in (1.0, 0.5, 0.25, 2.0)]
    text, lat, src, tgt = c.text.cuda(), c.lat.cuda(), c.src.cuda(), c.tgt.cuda()
    rows = [0, 1, 2, 6, 7, 8]

    def fwd(x, t, objects):
        with torch.no_grad():
            if objects:
                return model(x, torch.tensor(t), text, source_image_latents=lat, views=3, objects=objects, source_camera=src,
                             target_camera=tgt).sample.clone()
            return model(x[rows], torch.tensor(t), text[[0, 2]], source_image_latents=lat[:1], views=3, source_camera=src[:3],
                         target_camera=tgt[:3]).sample.clone()

    try:
        model.use_hip_graph = False
        model.cache_reference = False
        want = [fwd(x, 100 + 50 * i, 2) for i, x in enumerate(xs)]
        want_shared = [fwd(x, 100 + 50 * i, None) for i, x in enumerate(xs[:3])]
        model.use_hip_graph = True
        got = [fwd(x, 100 + 50 * i, 2) for i, x in enumerate(xs)]
        got_shared = [fwd(x, 100 + 50 * i, None) for i, x in enumerate(xs[:3])]
    finally:
        model.use_hip_graph = False
    for a, b in zip(got + got_shared, want + want_shared):
        assert torch.equal(a, b)


def test_objects_rejections_in_python(tiny):
    from mvd_amd._lib import MvdError
    from tests.objects_util import objects_case
    _, _, model = tiny
    c = objects_case(2, 3, 2, 16, 0.3)
    kw = dict(source_camera=c.src.cuda(), target_camera=c.tgt.cuda(), views=3, objects=2)
    x, text, lat = c.sample.cuda(), c.text.cuda(), c.lat.cuda()
    with torch.no_grad():
        with pytest.raises(MvdError, match="reference_stats_group"):
            model.reference_stats_group = True
            try:
                model(x, c.t, text, source_image_latents=lat, **kw)
            finally:
                model.reference_stats_group = None
        with pytest.raises(MvdError, match="2 rows of source_image_latents"):        # one source for two objects
            model(x, c.t, text, source_image_latents=lat[:1], **kw)
        with pytest.raises(MvdError, match="2 rows of source_image_latents"):        # one per (object, view)
            model(x, c.t, text, source_image_latents=lat.repeat_interleave(3, 0), **kw)
        with pytest.raises(MvdError, match="g \\* objects \\* views"):               # text per row instead of per (half, object)
            model(x, c.t, text.repeat_interleave(3, 0), source_image_latents=lat, **kw)
        with pytest.raises(MvdError, match="g \\* objects \\* views"):               # one view's rows missing
            model(x[:10], c.t, text, source_image_latents=lat, **kw)
        with pytest.raises(MvdError, match="g \\* objects \\* views"):               # g = 3
            model(torch.cat([x, x[:6]]), c.t, text, source_image_latents=lat, **kw)


# ------------------------------------------------------------------------------------------------ generate_views_batch
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
def test_generate_views_batch_matches_the_per_view_loops(tiny, ddim_pipe, gs):
    """``generate_views_batch`` (DDIM, 4 steps, O = 2, V = 2, explicit latents) against the O V per-view oracle loops (oracle.mvd
    forward + the fp64 DDIM step of tests/sampler_ref.py, one view at a time) within 4e-2, and against O ``generate_views``
    calls with the same latents within twice that."""
    from mvd_amd.utils import orbit_cameras
    from tests import sampler_ref as R
    from tests.parity_util import make_inputs, rel_l2
    cfg, params, _ = tiny
    pipe = ddim_pipe
    O, V, steps = 2, 2, 4
    inp = make_inputs(cfg, O, 16, 7, seed=23, cam_dim=96)
    g = torch.Generator().manual_seed(7)
    neg = torch.randn(O, 7, cfg.cross_attention_dim, generator=g)
    lat0 = torch.randn(O * V, 4, 16, 16, generator=g)
    src = torch.cat([orbit_cameras(1), orbit_cameras(1, elevation_deg=10.0, start_deg=20.0)])          # (O, 3, 4)
    tgt = torch.stack([orbit_cameras(V, elevation_deg=15.0, start_deg=40.0), orbit_cameras(V, elevation_deg=-5.0, start_deg=130.0)])
    sc = pipe.scheduler.config
    ts = R.timesteps("ddim", sc.num_train_timesteps, steps, sc.timestep_spacing, sc.steps_offset)
    want = torch.cat([R.denoise_loop(params, cfg, pipe.scheduler.betas, inp["text"][o:o + 1], neg[o:o + 1], lat0[o * V + v:o * V + v + 1],
                                     src[o:o + 1], tgt[o, v:v + 1], inp["lat"][o:o + 1], "ddim", ts, gs, [inp["proj"]] * steps,
                                     set_alpha_to_one=getattr(sc, "set_alpha_to_one", True), img_ref_scale=0.3,
                                     cam_modulation_strength=0.2) for o in range(O) for v in range(V)])
    pipe.unet.fourier_projection = inp["proj"]
    pipe.unet.cache_reference = True
    common = dict(num_inference_steps=steps, guidance_scale=gs, output_type="latent")
    got = pipe.generate_views_batch(prompt_embeds=inp["text"].cuda(), negative_prompt_embeds=neg.cuda(), source_cameras=src,
                                    target_cameras=tgt, latents=lat0.cuda(), source_image_latents=inp["lat"].cuda(), **common)["images"]
    assert pipe.scheduler.timesteps.tolist() == ts.tolist()
    per_object = torch.cat([pipe.generate_views(prompt_embeds=inp["text"][o:o + 1].cuda(), negative_prompt_embeds=neg[o:o + 1].cuda(),
                                                source_camera=src[o], target_cameras=tgt[o], latents=lat0[o * V:(o + 1) * V].cuda(),
                                                source_image_latents=inp["lat"][o:o + 1].cuda(), **common)["images"] for o in range(O)])
    pipe.unet.cache_reference = False
    assert got.shape == lat0.shape and torch.isfinite(got).all()
    e_oracle, e_calls = rel_l2(got, want), rel_l2(got, per_object.cpu())
    print(f"generate_views_batch gs={gs}: rel-L2 {e_oracle:.3e} to the per-view oracle loops, {e_calls:.3e} to the per-object "
          "generate_views calls", flush=True)
    assert e_oracle <= 4e-2, e_oracle
    assert e_calls <= 8e-2, e_calls


def test_generate_views_batch_latents_from_a_list_of_generators(ddim_pipe, monkeypatch):
    """with a list of O V generators the loop starts from the per-view calls' latents: row o V + v is generator o V + v's own
    draw (what ``pipe(...)`` draws for that view from that generator)"""
    from mvd_amd import pipeline as P
    from mvd_amd._lib import MvdError
    from mvd_amd.utils import orbit_cameras
    pipe = ddim_pipe
    O, V = 2, 2
    shape = (pipe.unet.config.sample_size * pipe.vae_scale_factor,) * 2
    mk = lambda: [torch.Generator().manual_seed(200 + r) for r in range(O * V)]      # noqa: E731
    seen = {}

    class Spy(P.MVDDenoiser):
        def __call__(self, *args, **kw):
            seen["latents"], seen["views"], seen["objects"] = kw["latents"].clone(), kw["views"], kw["objects"]
            raise MvdError("stop before the loop")

    monkeypatch.setattr(P, "MVDDenoiser", Spy)
    from mvd_amd.config import UNetConfig
    xd = UNetConfig.tiny().cross_attention_dim
    with pytest.raises(MvdError, match="stop before the loop"):
        pipe.generate_views_batch(prompt_embeds=torch.zeros(O, 7, xd), source_cameras=orbit_cameras(O), target_cameras=orbit_cameras(V),
                                  source_image_latents=torch.zeros(O, 4, shape[0] // pipe.vae_scale_factor, shape[1] // pipe.vae_scale_factor),
                                  generator=mk(), output_type="latent")
    assert (seen["views"], seen["objects"]) == (V, O) and seen["latents"].shape[0] == O * V
    for r, gen in enumerate(mk()):
        assert torch.equal(seen["latents"][r:r + 1], pipe.prepare_latents(1, 4, *shape, torch.float32, pipe.device, gen))
    with pytest.raises(ValueError, match="list of generators"):
        pipe.generate_views_batch(prompt_embeds=torch.zeros(O, 7, xd), source_cameras=orbit_cameras(O), target_cameras=orbit_cameras(V),
                                  source_image_latents=torch.zeros(O, 4, 2, 2), generator=mk()[:O], output_type="latent")
