"""Ragged turntables -- O objects with V_o views each in one forward (N16, ``MultiViewUNet.forward(..., views=(V_0, ..))`` /
``MVDPipeline.generate_views_batch`` with a list of per-object cameras) on the GPU against the CPU oracle.  The ragged forward is
DEFINED as the R = sum V_o independent forwards of batch g with a one-row reference (tests/ragged_util.py computes exactly that
on the oracle), so every comparison here is against the per-view calls.

Tolerances: test_objects_gpu.py's -- rel-L2 <= 2e-2, max <= 5e-2 max|ref|, every single row <= 4e-2 for one forward; 4e-2 for four
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


def _ragged(model, c, **kw):
    model.fourier_projection = c.proj
    with torch.no_grad():
        return model(c.sample.cuda(), c.t, c.text.cuda(), source_camera=c.src.cuda(), target_camera=c.tgt.cuda(),
                     source_image_latents=kw.pop("lat", c.lat.cuda()), views=kw.pop("views", c.counts), **kw).sample


@pytest.mark.parametrize("counts,g,hw", [((3, 1), 1, 16), ((3, 1), 2, 16), ((3, 2, 1), 1, 16), ((3, 2, 1), 2, 16), ((1, 3), 2, (16, 32))])
def test_ragged_forward_matches_the_independent_oracle_calls(tiny, counts, g, hw):
    from tests.parity_util import max_rel, rel_l2
    from tests.ragged_util import per_row, ragged_case
    _, _, model = tiny
    c = ragged_case(counts, g, hw, 0.3)
    got = _ragged(model, c)
    assert got.shape == c.want.shape and torch.isfinite(got).all()
    err, emax = rel_l2(got, c.want), max_rel(got, c.want)
    print(f"ragged forward counts={counts} g={g} hw={hw}: rel-L2 {err:.3e} max {emax:.3e}", flush=True)
    rows = per_row(got, c.want)
    print("  per row:", " ".join(f"{e:.2e}" for e in rows), flush=True)
    assert err <= TOL_L2, (err, emax)
    assert emax <= TOL_MAX, emax
    # row by row (a row answered with another object's reference, camera or text hides in the batch figure)
    assert max(rows) <= 2 * TOL_L2, rows


def test_ragged_forward_is_not_a_wrong_result(tiny_full_scale):
    """img_ref_scale = 1.0, counts (3, 2, 1), g = 2, the case whose oracle distances tests/test_ragged_cpu.py holds: the ragged forward
    is closer to the independent calls than half the distance of the nearest wrong result -- over the batch (the repeated-source
    batch, the uniform map forced onto the ragged batch) and over the rows of each view that map misroutes -- and further than
    half each distance from each wrong result."""
    from tests.parity_util import rel_l2
    from tests.ragged_util import ragged_case, view_rows
    _, _, model = tiny_full_scale
    c = ragged_case((3, 2, 1), 2, 16, 1.0, 1.0, True)
    got = _ragged(model, c).cpu()
    err = rel_l2(got, c.want)
    wrong = dict(rep=c.d_rep, uniform=c.d_uniform)
    print(f"ragged forward (3, 2, 1) g=2 img_ref_scale=1.0: rel-L2 {err:.3e}; wrong results "
          + " / ".join(f"{k} {d:.3e}" for k, d in wrong.items()), flush=True)
    assert torch.isfinite(got).all()
    assert err < 0.5 * min(wrong.values()), (err, wrong)
    for name, d in wrong.items():
        assert rel_l2(got, getattr(c, name)) > 0.5 * d, (name, rel_l2(got, getattr(c, name)), d)
    for i, d in zip(c.misrouted, c.d_misrouted):
        rows = view_rows(c.R, c.g, i)
        e_right, e_wrong = rel_l2(got[rows], c.want[rows]), rel_l2(got[rows], c.uniform[rows])
        print(f"  view {i}: {e_right:.3e} to its own object's call, {e_wrong:.3e} to the misrouted one ({d:.3e} apart)", flush=True)
        assert e_right < 0.5 * d and e_wrong > 0.5 * d, (i, e_right, e_wrong, d)


@pytest.mark.parametrize("counts,g", [((2, 2), 2), ((3, 3, 3), 1)])
def test_equal_counts_are_the_object_forward_bit_for_bit(tiny, counts, g):
    from tests.objects_util import objects_case
    _, _, model = tiny
    O, V = len(counts), counts[0]
    c = objects_case(O, V, g, 16, 0.3)
    model.fourier_projection = c.proj
    kw = dict(source_camera=c.src.cuda(), target_camera=c.tgt.cuda(), source_image_latents=c.lat.cuda())
    with torch.no_grad():
        want = model(c.sample.cuda(), c.t, c.text.cuda(), **kw, views=V, objects=O).sample
        got = model(c.sample.cuda(), c.t, c.text.cuda(), **kw, views=counts).sample
        got_o = model(c.sample.cuda(), c.t, c.text.cuda(), **kw, views=list(counts), objects=O).sample
    assert torch.equal(got, want) and torch.equal(got_o, want)


def test_one_object_is_the_shared_forward_bit_for_bit(tiny):
    from tests.views_util import views_case
    _, _, model = tiny
    c = views_case(4, 2, 16, 0.3)
    model.fourier_projection = c.proj
    kw = dict(source_camera=c.src.cuda(), target_camera=c.tgt.cuda(), source_image_latents=c.lat.cuda())
    with torch.no_grad():
        want = model(c.sample.cuda(), c.t, c.text.cuda(), **kw, views=4).sample
        got = model(c.sample.cuda(), c.t, c.text.cuda(), **kw, views=(4,)).sample
    assert torch.equal(got, want)


def test_ragged_reference_cache_is_exact_one_row_per_object_and_bound_to_its_layout():
    """Q5 with view counts: a second and a third ragged forward at another timestep are served from the cached reference K/V,
    bit-identical to recomputing them; the engine's reference cache is the ref_batch = O one; a cache filled under another layout
    -- other counts with the same sum, or the objects forward on the same tensors -- is not served (Python recomputes, and the
    engine itself refuses MVD_REUSE_REF)."""
    from mvd_amd import _lib as L
    from tests.ragged_util import ragged_case
    _, _, model = _pair(0.3)                       # a fresh engine: its buffers are sized by this test's forwards alone
    c = ragged_case((3, 2, 1), 2, 16, 0.3)
    lat = c.lat.cuda()
    model.cache_reference = False
    a = _ragged(model, c, lat=lat)
    eng = model._engine
    model.reset_reference_cache()
    calls = []
    fwd = eng.forward
    eng.forward = lambda *args, **kw: (calls.append(bool(kw.get("reuse_ref"))), fwd(*args, **kw))[1]
    x, text = c.sample.cuda(), c.text.cuda()
    kw = dict(source_camera=c.src.cuda(), target_camera=c.tgt.cuda(), source_image_latents=lat)
    try:
        model.cache_reference = True
        with torch.no_grad():
            model(x, torch.tensor(900), text, **kw, views=c.counts)
            b = model(x, c.t, text, **kw, views=c.counts).sample                 # served from the cache
            b2 = model(x, c.t, text, **kw, views=c.counts).sample                # and again
            other = model(x, c.t, text, **kw, views=(1, 2, 3)).sample            # another layout, the same tensors: no hit
            model(x, c.t, text, **kw, views=2, objects=3)                        # the objects forward: another mode, no hit
            back = model(x, c.t, text, **kw, views=c.counts).sample              # and none for the first layout after it
    finally:
        eng.forward = fwd
        model.cache_reference = False
    assert calls == [False, True, True, False, False, False], calls
    assert torch.equal(a, b) and torch.equal(a, b2) and torch.equal(a, back)
    assert not torch.equal(a, other)
    three = L.lib().mvd_engine_refcache_bytes(eng._h, 3, 16, 16, 0)
    assert eng._rc.numel() == three and three < L.lib().mvd_engine_refcache_bytes(eng._h, 6, 16, 16, 0)
    # the engine's own record: its cache now holds layout (3, 2, 1), and MVD_REUSE_REF under (1, 2, 3) is refused by the library.
    # (The workspace is marked as bound for that layout -- same shapes, same sizes -- because binding it anew would drop the cached
    #  reference and the refusal would be for that.)
    assert eng._ws_key == (12, 16, 16, 7, 3, False, 0, (3, 2, 1))
    eng._ws_key = (12, 16, 16, 7, 3, False, 0, (1, 2, 3))
    with torch.no_grad(), pytest.raises(L.MvdError, match="without a matching cached reference"):
        eng.forward(x, torch.full((12,), 321.0, device="cuda"), text, reuse_ref=True, views=(1, 2, 3))
    eng._ws_key = None


def test_ragged_hip_graph_replay_is_bit_exact_with_layouts_alternated(tiny):
    """``use_hip_graph`` with view counts: two layouts alternated on one engine, a uniform ``objects=`` forward in between -- run,
    capture, replay, replay on refreshed inputs, all bit-identical to the plain launches.  A replayed graph reads its layout's
    table slot: no slot may have been rewritten by the other layout's forwards (the slot-lifetime rule)."""
    from tests.ragged_util import ragged_case
    _, _, model = tiny
    ca, cb = ragged_case((3, 2, 1), 2, 16, 0.3), ragged_case((1, 2, 3), 2, 16, 0.3)
    model.fourier_projection = ca.proj
    xs = [(ca.sample * s).cuda() for s in (1.0, 0.5, 0.25, 2.0)]
    text, lat, src, tgt = ca.text.cuda(), ca.lat.cuda(), ca.src.cuda(), ca.tgt.cuda()
    src_b = cb.src.cuda()

    def fwd(x, t, mode):
        with torch.no_grad():
            kw = dict(source_image_latents=lat, target_camera=tgt)
            if mode == "a":
                return model(x, torch.tensor(t), text, views=(3, 2, 1), source_camera=src, **kw).sample.clone()
            if mode == "b":
                return model(x, torch.tensor(t), text, views=(1, 2, 3), source_camera=src_b, **kw).sample.clone()
            return model(x, torch.tensor(t), text, views=2, objects=3, source_camera=src, **kw).sample.clone()

    order = ["a", "b", "o", "a", "b", "a", "o", "b", "b", "a", "a", "b"]
    try:
        model.use_hip_graph = False
        model.cache_reference = False
        want = [fwd(xs[i % 4], 100 + 50 * (i % 4), m) for i, m in enumerate(order)]
        model.use_hip_graph = True
        got = [fwd(xs[i % 4], 100 + 50 * (i % 4), m) for i, m in enumerate(order)]
    finally:
        model.use_hip_graph = False
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), (i, order[i])
    assert not torch.equal(want[0], want[1])               # the two layouts compute different things on the same rows


def test_ragged_rejections_in_python(tiny):
    from mvd_amd._lib import MvdError
    from tests.ragged_util import ragged_case
    _, _, model = tiny
    c = ragged_case((3, 2, 1), 2, 16, 0.3)
    kw = dict(source_camera=c.src.cuda(), target_camera=c.tgt.cuda())
    x, text, lat = c.sample.cuda(), c.text.cuda(), c.lat.cuda()
    with torch.no_grad():
        with pytest.raises(MvdError, match="reference_stats_group"):
            model.reference_stats_group = True
            try:
                model(x, c.t, text, source_image_latents=lat, views=(3, 2, 1), **kw)
            finally:
                model.reference_stats_group = None
        with pytest.raises(MvdError, match="at least one view"):
            model(x, c.t, text, source_image_latents=lat, views=(3, 3, 0), **kw)
        with pytest.raises(MvdError, match="at least one view"):
            model(x, c.t, text, source_image_latents=lat, views=(), **kw)
        with pytest.raises(MvdError, match="objects must be None or 3"):
            model(x, c.t, text, source_image_latents=lat, views=(3, 2, 1), objects=2, **kw)
        with pytest.raises(MvdError, match="3 rows of source_image_latents"):        # one source for three objects
            model(x, c.t, text, source_image_latents=lat[:1], views=(3, 2, 1), **kw)
        with pytest.raises(MvdError, match="3 rows of source_image_latents"):        # one per view
            model(x, c.t, text, source_image_latents=lat[[0, 0, 0, 1, 1, 2]], views=(3, 2, 1), **kw)
        with pytest.raises(MvdError, match="g \\* 6 rows"):                          # text per row instead of per (half, object)
            model(x, c.t, text[[0, 0, 0, 1, 1, 2, 3, 3, 3, 4, 4, 5]], source_image_latents=lat, views=(3, 2, 1), **kw)
        with pytest.raises(MvdError, match="g \\* 6 rows"):                          # one view's rows missing
            model(x[:10], c.t, text, source_image_latents=lat, views=(3, 2, 1), **kw)
        with pytest.raises(MvdError, match="g \\* 6 rows"):                          # g = 3
            model(torch.cat([x, x[:6]]), c.t, text, source_image_latents=lat, views=(3, 2, 1), **kw)
        with pytest.raises(MvdError, match="cameras must hold 1 or sum of the view counts = 6"):      # one camera per object
            model(x, c.t, text, source_image_latents=lat, views=(3, 2, 1), source_camera=c.src[:3].cuda(), target_camera=c.tgt[:3].cuda())


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
def test_ragged_generate_views_batch_matches_the_per_view_loops(tiny, ddim_pipe, gs):
    """``generate_views_batch`` with a ragged camera list (DDIM, 4 steps, counts (2, 1), explicit latents) against the three
    per-view oracle loops (oracle.mvd forward + the fp64 DDIM step of tests/sampler_ref.py, one view at a time) within 4e-2, and
    against the per-object ``generate_views`` calls with the same latents within twice that."""
    from mvd_amd.utils import orbit_cameras
    from tests import sampler_ref as R
    from tests.parity_util import make_inputs, rel_l2
    cfg, params, _ = tiny
    pipe = ddim_pipe
    counts, steps = (2, 1), 4
    O, Rn = len(counts), sum(counts)
    offs = [0, 2]
    inp = make_inputs(cfg, O, 16, 7, seed=23, cam_dim=96)
    g = torch.Generator().manual_seed(7)
    neg = torch.randn(O, 7, cfg.cross_attention_dim, generator=g)
    lat0 = torch.randn(Rn, 4, 16, 16, generator=g)
    src = torch.cat([orbit_cameras(1), orbit_cameras(1, elevation_deg=10.0, start_deg=20.0)])          # (O, 3, 4)
    tgt = [orbit_cameras(2, elevation_deg=15.0, start_deg=40.0), orbit_cameras(1, elevation_deg=-5.0, start_deg=130.0)]
    sc = pipe.scheduler.config
    ts = R.timesteps("ddim", sc.num_train_timesteps, steps, sc.timestep_spacing, sc.steps_offset)
    want = torch.cat([R.denoise_loop(params, cfg, pipe.scheduler.betas, inp["text"][o:o + 1], neg[o:o + 1], lat0[offs[o] + v:offs[o] + v + 1],
                                     src[o:o + 1], tgt[o][v:v + 1], inp["lat"][o:o + 1], "ddim", ts, gs, [inp["proj"]] * steps,
                                     set_alpha_to_one=getattr(sc, "set_alpha_to_one", True), img_ref_scale=0.3,
                                     cam_modulation_strength=0.2) for o in range(O) for v in range(counts[o])])
    pipe.unet.fourier_projection = inp["proj"]
    pipe.unet.cache_reference = True
    common = dict(num_inference_steps=steps, guidance_scale=gs, output_type="latent")
    got = pipe.generate_views_batch(prompt_embeds=inp["text"].cuda(), negative_prompt_embeds=neg.cuda(), source_cameras=src,
                                    target_cameras=tgt, latents=lat0.cuda(), source_image_latents=inp["lat"].cuda(), **common)["images"]
    assert pipe.scheduler.timesteps.tolist() == ts.tolist()
    per_object = torch.cat([pipe.generate_views(prompt_embeds=inp["text"][o:o + 1].cuda(), negative_prompt_embeds=neg[o:o + 1].cuda(),
                                                source_camera=src[o], target_cameras=tgt[o], latents=lat0[offs[o]:offs[o] + counts[o]].cuda(),
                                                source_image_latents=inp["lat"][o:o + 1].cuda(), **common)["images"] for o in range(O)])
    pipe.unet.cache_reference = False
    assert got.shape == lat0.shape and torch.isfinite(got).all()
    e_oracle, e_calls = rel_l2(got, want), rel_l2(got, per_object.cpu())
    print(f"ragged generate_views_batch gs={gs}: rel-L2 {e_oracle:.3e} to the per-view oracle loops, {e_calls:.3e} to the per-object "
          "generate_views calls", flush=True)
    assert e_oracle <= 4e-2, e_oracle
    assert e_calls <= 8e-2, e_calls


def test_ragged_generate_views_batch_latents_from_a_list_of_generators(ddim_pipe, monkeypatch):
    """with a list of R generators the loop starts from the per-view calls' latents: row c is generator c's own draw"""
    from mvd_amd import pipeline as P
    from mvd_amd._lib import MvdError
    from mvd_amd.config import UNetConfig
    from mvd_amd.utils import orbit_cameras
    pipe = ddim_pipe
    counts = (2, 1)
    Rn = sum(counts)
    shape = (pipe.unet.config.sample_size * pipe.vae_scale_factor,) * 2
    mk = lambda: [torch.Generator().manual_seed(300 + r) for r in range(Rn)]      # noqa: E731
    seen = {}

    class Spy(P.MVDDenoiser):
        def __call__(self, *args, **kw):
            seen["latents"], seen["views"], seen["cams"] = kw["latents"].clone(), kw["views"], (kw["source_camera"], kw["target_camera"])
            raise MvdError("stop before the loop")

    monkeypatch.setattr(P, "MVDDenoiser", Spy)
    xd = UNetConfig.tiny().cross_attention_dim
    src, tgt = orbit_cameras(2), [orbit_cameras(2, start_deg=30.0), orbit_cameras(1, start_deg=200.0)]
    lat = torch.zeros(2, 4, shape[0] // pipe.vae_scale_factor, shape[1] // pipe.vae_scale_factor)
    with pytest.raises(MvdError, match="stop before the loop"):
        pipe.generate_views_batch(prompt_embeds=torch.zeros(2, 7, xd), source_cameras=src, target_cameras=tgt, source_image_latents=lat,
                                  generator=mk(), output_type="latent")
    assert seen["views"] == counts and seen["latents"].shape[0] == Rn
    for r, gen in enumerate(mk()):
        assert torch.equal(seen["latents"][r:r + 1], pipe.prepare_latents(1, 4, *shape, torch.float32, pipe.device, gen))
    # the source camera of an object on each of its views' rows, the target cameras in object-major order
    assert torch.equal(seen["cams"][0].cpu(), src[[0, 0, 1]]) and torch.equal(seen["cams"][1].cpu(), torch.cat(tgt))
    with pytest.raises(ValueError, match="list of generators"):
        pipe.generate_views_batch(prompt_embeds=torch.zeros(2, 7, xd), source_cameras=src, target_cameras=tgt, source_image_latents=lat,
                                  generator=mk()[:2], output_type="latent")
