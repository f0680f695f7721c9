"""DeepCache in the engine (``mvd_engine_set_deepcache``) on the MI355X: tiny topology, 16 x 16 latents,
batch 2, text length 7.  The definition makes the feature testable bit for bit: a shallow forward is the full forward with ONE
tensor -- the hidden input of ``up_blocks.{n-1}.resnets.{Lb-1-branch}`` -- replaced by the stored one, so on unchanged inputs it
must reproduce the refresh forward exactly, and on changed inputs it must follow the oracle's record -> replay
(tests/deepcache_ref.py), which tests/test_deepcache_cpu.py shows to be far from both the full forward and the old output.

The parity bounds are measured, not fixed: 1.5 x the rel-L2 of the plain engine forward (loop) against the plain oracle on the
same inputs -- the stored feature carries the first step's bf16 error unchanged into a forward that re-reads it, the margin the
FreeU tests took -- and never more than 3e-2 for a forward (``freeu_ref.PARITY_BOUND_MAX``) / 4e-2 for a loop
(tests/test_samplers_gpu.py).

Measured on one MI355X (rel-L2):
  forward, second step's inputs: plain engine vs plain oracle 1.398e-2 -> bound 2.098e-2; shallow vs the replayed oracle 1.342e-2
  (branch 0) / 1.400e-2 (branch 1); shallow vs the FULL oracle 0.870 / 0.475, vs the first step's oracle output 0.762 / 1.011;
  6-step CFG-3 DDIM loop, interval 3: DeepCache off 1.855e-2 -> bound 2.783e-2, on 1.986e-2 (0.339 to the plain oracle loop);
  generate_views, 2 views, 4 steps: off 2.342e-2 -> bound 3.513e-2, on 2.058e-2 (0.624 to the plain oracle loops)."""
import contextlib
import ctypes as C

import pytest
import torch

from tests import deepcache_ref as DR
from tests import freeu_ref as FR

pytestmark = pytest.mark.gpu

LOOP_BOUND_MAX = 4e-2          # the loop bound of tests/test_samplers_gpu.py


def _pair():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tests.parity_util import build_pair
    return build_pair("tiny", 0, 96, 48)


@pytest.fixture(scope="module")
def tiny():
    return _pair()


@pytest.fixture(scope="module")
def two_steps(tiny):
    """the CPU file's inputs: first step seed 0 at t = 500, second step the same with the ``sample`` of seed 1 at t = 100; on the device
    as ONE set of tensors (the wrapper recognises the reference by tensor identity), with the plain oracle's outputs"""
    from tests.parity_util import make_inputs
    cfg, params, _ = tiny
    a = make_inputs(cfg, 2, 16, 7, 0, 96)
    b = dict(a, sample=make_inputs(cfg, 2, 16, 7, 1, 96)["sample"])
    dev = {k: a[k].cuda() for k in ("text", "src", "tgt", "lat")}
    dev["sample_a"], dev["sample_b"] = a["sample"].cuda(), b["sample"].cuda()
    return dict(a=a, b=b, dev=dev, first=_oracle(params, cfg, a, 500), full=_oracle(params, cfg, b, 100))


def _oracle(params, cfg, inp, t):
    from oracle import mvd as OM
    with torch.no_grad():
        return OM.multiview_unet_forward(params, cfg, inp["sample"], torch.tensor(t), inp["text"], inp["src"], inp["tgt"], inp["lat"],
                                         fourier_proj=inp["proj"], img_ref_scale=0.3, cam_modulation_strength=0.2)


def _fwd(model, d, sample, t, deep=None, image=True, camera=True, **layout):
    """one wrapper forward on the device tensors ``d`` (the same objects every call)"""
    kw = dict(deep_cache=deep) if deep is not None else {}
    if camera:
        kw.update(source_camera=d["src"], target_camera=d["tgt"])
    if image:
        kw.update(source_image_latents=d["lat"])
    with torch.no_grad():
        return model(sample, torch.as_tensor(t), d["text"], **kw, **layout).sample.clone()


@pytest.fixture()
def clean(tiny):
    """every test leaves the shared model as it found it"""
    model = tiny[2]
    yield model
    model.disable_deepcache()
    model.disable_freeu()
    model.cache_reference = False
    model.use_hip_graph = False
    model.reset_reference_cache()
    if model._engine is not None:
        model._engine.set_profiling(False)


# ------------------------------------------------------------------------------------------------ 1. bit identity
@pytest.mark.parametrize("branch", [0, 1])
@pytest.mark.parametrize("case", ["camera+image", "no-image", "ragged(2,1)g2", "freeu"])
def test_shallow_forward_on_the_same_inputs_is_the_refresh_forward_bit_for_bit(tiny, two_steps, clean, case, branch):
    """a cold forward, then a refresh forward with the reference reused (A), then a shallow forward on the same inputs (B):
    ``torch.equal(A, B)``.  Both reuse the reference, so both run single-stream and every executed kernel gets the launch plan its
    shape alone decides (no kernel's split or tile choice was found to depend on more: the identity holds as stated).  Without
    image conditioning there is no reference and both forwards are single-stream anyway."""
    model = clean
    model.enable_deepcache(3, branch)
    model.cache_reference = True
    if case == "ragged(2,1)g2":
        from tests.ragged_util import ragged_case
        c = ragged_case((2, 1), 2, 16, 0.3)
        model.fourier_projection = c.proj
        d = dict(text=c.text.cuda(), src=c.src.cuda(), tgt=c.tgt.cuda(), lat=c.lat.cuda())
        x, t, kw = c.sample.cuda(), c.t, dict(views=c.counts)
    else:
        model.fourier_projection = two_steps["a"]["proj"]
        d, x, t, kw = two_steps["dev"], two_steps["dev"]["sample_a"], 500, {}
        if case == "no-image":
            kw = dict(image=False)
        if case == "freeu":
            model.enable_freeu(**FR.SD21)
    eng_calls = []
    plain = _fwd(model, d, x, t, **kw)                                   # cold: fills the reference cache
    fwd = model._engine.forward
    model._engine.forward = lambda *a, **k: (eng_calls.append((bool(k.get("reuse_ref")), k.get("deep_cache"))), fwd(*a, **k))[1]
    try:
        A = _fwd(model, d, x, t, "refresh", **kw)
        B = _fwd(model, d, x, t, "reuse", **kw)
    finally:
        model._engine.forward = fwd
    img = case != "no-image"
    assert eng_calls == [(img, "refresh"), (img, "reuse")], eng_calls
    assert torch.isfinite(A).all() and A.shape == x.shape
    assert torch.equal(A, plain)                                          # (a refresh forward is the forward)
    assert torch.equal(A, B)
    # and the shallow forward does read the stored feature: on another sample it is neither A nor that sample's full forward
    x2 = x.flip(0).contiguous()
    B2, full2 = _fwd(model, d, x2, t, "reuse", **kw), _fwd(model, d, x2, t, **kw)
    assert not torch.equal(B2, A) and not torch.equal(B2, full2)


# ------------------------------------------------------------------------------------------------ 2. refresh changes nothing
def test_refresh_forward_is_the_plain_forward_bit_for_bit(two_steps, clean):
    """cold and with the reference reused, against a FRESH engine that has never heard of DeepCache"""
    model = clean
    _, _, fresh = _pair()
    d = two_steps["dev"]
    model.fourier_projection = fresh.fourier_projection = two_steps["a"]["proj"]
    want = _fwd(fresh, d, d["sample_a"], 500)
    for branch in (0, 1):
        model.enable_deepcache(2, branch)
        model.cache_reference = False
        assert torch.equal(_fwd(model, d, d["sample_a"], 500, "refresh"), want)              # cold: the two-stream forward
        model.cache_reference = True
        _fwd(model, d, d["sample_a"], 900)
        assert torch.equal(_fwd(model, d, d["sample_a"], 500, "refresh"), want)              # reference reused
    assert fresh._engine.deepcache is None and model._engine.deepcache == 1


def _tiny_pipe(params):
    from mvd_amd.config import UNetConfig
    from mvd_amd.mvd_unet import create_mvd_pipeline
    pipe = create_mvd_pipeline(None, dtype=torch.float32, img_ref_scale=0.3, cam_modulation_strength=0.2, cam_output_dim=96,
                               cam_hidden_dim=48, unet_config=UNetConfig.tiny(), init="empty", sampler="ddim")
    missing, unexpected = pipe.unet.load_state_dict(params, strict=False)
    assert not missing and not unexpected
    pipe = pipe.to("cuda")
    pipe.unet.eval()
    return pipe


def _loop_inputs(cfg):
    from mvd_amd.utils import orbit_cameras
    from tests.parity_util import make_inputs
    inp = make_inputs(cfg, 2, 16, 7, seed=31, cam_dim=96)
    g = torch.Generator().manual_seed(5)
    neg = torch.randn(2, 7, cfg.cross_attention_dim, generator=g)
    lat0 = torch.randn(2, 4, 16, 16, generator=g)
    return inp, orbit_cameras(1), orbit_cameras(1, elevation_deg=15.0, start_deg=40.0), neg, lat0


def _run_loop(pipe, inp, src, tgt, neg, lat0, steps, gs):
    pipe.unet.fourier_projection = inp["proj"]
    pipe.unet.cache_reference = True
    return pipe(prompt_embeds=inp["text"].cuda(), negative_prompt_embeds=neg.cuda(), num_inference_steps=steps, guidance_scale=gs,
                latents=lat0.cuda(), source_camera=src.cuda(), target_camera=tgt.cuda(), source_image_latents=inp["lat"].cuda(),
                output_type="latent")["images"].clone()


@pytest.fixture(scope="module")
def pipe(tiny):
    return _tiny_pipe(tiny[1])


def test_interval_one_and_disable_after_enable_are_the_plain_loop_bit_for_bit(tiny, pipe):
    """3-step guided DDIM loop: a fresh pipeline's result == ``enable_deepcache(1)`` == enable(3) then disable; interval 3 differs"""
    cfg, params, _ = tiny
    args = _loop_inputs(cfg)
    want = _run_loop(_tiny_pipe(params), *args, 3, 3.0)
    try:
        pipe.enable_deepcache(cache_interval=1)
        one = _run_loop(pipe, *args, 3, 3.0)
        pipe.enable_deepcache(cache_interval=3)
        three = _run_loop(pipe, *args, 3, 3.0)
        assert pipe.unet._engine.deepcache == 0
        pipe.disable_deepcache()
        off = _run_loop(pipe, *args, 3, 3.0)
        assert pipe.unet._engine.deepcache is None
    finally:
        pipe.disable_deepcache()
    assert torch.equal(one, want) and torch.equal(off, want)
    assert not torch.equal(three, want)


# ------------------------------------------------------------------------------------------------ 3. parity with the oracle
@pytest.mark.parametrize("branch", [0, 1])
def test_shallow_forward_matches_the_replayed_oracle(tiny, two_steps, clean, branch):
    """refresh at the first step's inputs (t = 500), shallow at the second step's (another sample, t = 100), against the oracle's
    record -> replay.  Bound: 1.5 x the plain engine forward's rel-L2 against the plain oracle at the second step's inputs (measured
    here), at most 3e-2; and the shallow output is at least 4 x the bound from the FULL oracle output at the second step's inputs.

    Measured on one MI355X (rel-L2): plain forward at the second step 1.398e-2 -> bound 2.098e-2; refresh at the first step 1.314e-2;
    shallow vs the replayed oracle 1.342e-2 (branch 0) / 1.400e-2 (branch 1); shallow vs the full oracle 0.870 / 0.475."""
    from tests.parity_util import rel_l2
    cfg, params, _ = tiny
    model, d = clean, two_steps["dev"]
    model.fourier_projection = two_steps["a"]["proj"]
    store = {}
    with DR.deepcache_oracle("record", store, branch):
        first = _oracle(params, cfg, two_steps["a"], 500)
    assert torch.equal(first, two_steps["first"])
    with DR.deepcache_oracle("replay", store, branch):
        want = _oracle(params, cfg, two_steps["b"], 100)
    model.cache_reference = False
    plain = rel_l2(_fwd(model, d, d["sample_b"], 100), two_steps["full"])
    bound = min(1.5 * plain, FR.PARITY_BOUND_MAX)
    model.enable_deepcache(3, branch)
    e_refresh = rel_l2(_fwd(model, d, d["sample_a"], 500, "refresh"), first)
    got = _fwd(model, d, d["sample_b"], 100, "reuse")
    err, e_full, e_first = rel_l2(got, want), rel_l2(got, two_steps["full"]), rel_l2(got, first)
    print(f"deepcache parity branch {branch}: plain forward at the second step {plain:.3e} -> bound {bound:.3e}; refresh at the first step "
          f"{e_refresh:.3e}; shallow vs replayed oracle {err:.3e}; shallow vs full oracle {e_full:.3e}, vs first-step oracle {e_first:.3e}", flush=True)
    assert torch.isfinite(got).all() and got.shape == want.shape
    assert err <= bound, (err, bound, plain)
    assert e_full >= 4 * bound, (e_full, bound)


# ------------------------------------------------------------------------------------------------ 4. the work is really skipped
def _attention_launches(eng):
    return sum(v["launches"] for k, v in eng.profile_summary().items() if k.startswith("attn_"))          # classes 8-11


@pytest.mark.parametrize("branch", [0, 1])
def test_shallow_forward_launches_only_its_own_attentions(two_steps, clean, branch):
    """per transformer block two attention launches: a full main pass has 16 blocks -> 32, a shallow pass (branch + 1) down and
    (branch + 2) up blocks -> 2 (2 branch + 3); the encoder pass (16 more blocks) appears in neither"""
    model, d = clean, two_steps["dev"]
    model.fourier_projection = two_steps["a"]["proj"]
    model.enable_deepcache(3, branch)
    model.cache_reference = True
    _fwd(model, d, d["sample_a"], 500)                                   # cold, un-profiled
    eng = model._engine
    eng.set_profiling(True)
    try:
        A = _fwd(model, d, d["sample_a"], 500, "refresh")
        full = _attention_launches(eng)
        B = _fwd(model, d, d["sample_a"], 500, "reuse")
        shallow = _attention_launches(eng)
    finally:
        eng.set_profiling(False)
    assert full == 32 and shallow == 2 * (2 * branch + 3), (full, shallow)
    assert torch.equal(A, B)


# ------------------------------------------------------------------------------------------------ 5. rejections
def _raw_args(eng, d, sample, t, out, flags, image=True):
    """the argument block ``MVDEngine.forward`` builds for the two-step inputs, for calls straight into the C ABI"""
    from mvd_amd import _lib as L
    B, _, H, W = sample.shape
    a = L.mvd_forward_args_t()
    a.batch, a.height, a.width, a.text_len = B, H, W, d["text"].shape[1]
    a.sample, a.timesteps, a.text = sample.data_ptr(), t.data_ptr(), d["text"].data_ptr()
    a.source_camera, a.target_camera, a.cam_rows, a.cam_batch = d["src"].data_ptr(), d["tgt"].data_ptr(), d["src"].shape[1], B
    a.fourier_proj = d["proj"].data_ptr()
    a.ref_batch = B if image else 0
    a.flags = L.MVD_USE_CAMERA | (L.MVD_USE_IMAGE | L.MVD_REUSE_REF if image else 0) | flags
    a.out = out.data_ptr()
    return a


def test_rejections_come_before_any_launch_and_leave_the_next_forward_alone(two_steps, clean):
    """every mismatch between the stored feature's record and a shallow forward's arguments is an error that names it, nothing is
    launched (the output buffer keeps its sentinel), and the next valid shallow forward gives what it gave before"""
    from mvd_amd import _lib as L
    model = clean
    d = dict(two_steps["dev"], proj=two_steps["a"]["proj"].cuda().contiguous())
    model.fourier_projection = two_steps["a"]["proj"]
    model.enable_deepcache(3, 0)
    model.cache_reference = True
    x, t = d["sample_a"], torch.full((2,), 500.0, device="cuda")
    _fwd(model, d, x, 500)                                               # cold
    eng, lib = model._engine, L.lib()
    out = torch.empty_like(x)

    def call(a):
        out.fill_(7.0)
        rc = lib.mvd_unet_forward(eng._h, C.byref(a), L.stream())
        torch.cuda.synchronize()
        return rc, L.last_error() if rc else ""

    def rejected(a, words):
        rc, msg = call(a)
        assert rc == -1 and words in msg, (rc, msg)
        assert bool((out == 7.0).all()), f"something was launched: {msg}"

    def valid(want):
        rc, msg = call(_raw_args(eng, d, x, t, out, L.MVD_DEEPCACHE_SHALLOW))
        assert rc == 0, msg
        assert torch.equal(out, want)

    # no stored feature yet
    rejected(_raw_args(eng, d, x, t, out, L.MVD_DEEPCACHE_SHALLOW), "without a stored deep feature")
    A = _fwd(model, d, x, 500, "refresh")
    valid(A)
    # both bits
    rejected(_raw_args(eng, d, x, t, out, L.MVD_DEEPCACHE_SHALLOW | L.MVD_DEEPCACHE_REFRESH), "one or the other")
    valid(A)
    # batch
    a = _raw_args(eng, d, x[:1], t, out, L.MVD_DEEPCACHE_SHALLOW)
    a.ref_batch = 1
    rejected(a, "is of batch 2, this forward of batch 1")
    valid(A)
    # size
    a = _raw_args(eng, d, x[:, :, :8, :8], t, out, L.MVD_DEEPCACHE_SHALLOW)
    rejected(a, "is of latent size 16x16, this forward of 8x8")
    valid(A)
    # layout: the two rows as two views of one object
    a = _raw_args(eng, d, x, t, out, L.MVD_DEEPCACHE_SHALLOW | L.MVD_SHARE_REF)
    a.views, a.ref_batch = 2, 1
    rejected(a, "another batch layout")
    valid(A)
    # conditioning bits
    rejected(_raw_args(eng, d, x, t, out, L.MVD_DEEPCACHE_SHALLOW, image=False), "image conditioning on")
    valid(A)
    # image conditioning without MVD_REUSE_REF
    a = _raw_args(eng, d, x, t, out, L.MVD_DEEPCACHE_SHALLOW)
    a.flags &= ~L.MVD_REUSE_REF
    rejected(a, "needs MVD_REUSE_REF")
    valid(A)
    # the encoder pass alone takes neither bit
    stats = torch.empty(1 << 16, device="cuda")
    rc = lib.mvd_engine_reference_encode(eng._h, C.byref(_raw_args(eng, d, x, t, out, L.MVD_DEEPCACHE_REFRESH)), C.c_void_p(stats.data_ptr()), L.stream())
    assert rc == -1 and "DeepCache bits" in L.last_error()
    valid(A)
    # a weight registered since: the same tensor again is a new generation
    slot = "conv_in.b"
    eng._register(0, {slot: eng._weights[0][slot]})
    rejected(_raw_args(eng, d, x, t, out, L.MVD_DEEPCACHE_SHALLOW), "weights were registered or cleared")
    assert torch.equal(_fwd(model, d, x, 500, "refresh"), A)
    valid(A)
    # the branch toggled (and back): the stored feature is gone
    eng.set_deepcache(1)
    rejected(_raw_args(eng, d, x, t, out, L.MVD_DEEPCACHE_SHALLOW), "without a stored deep feature")
    eng.set_deepcache(0)
    rejected(_raw_args(eng, d, x, t, out, L.MVD_DEEPCACHE_SHALLOW), "without a stored deep feature")
    assert torch.equal(_fwd(model, d, x, 500, "refresh"), A)
    valid(A)
    # image conditioning but no valid reference cache (the buffers bound again drop it; the stored feature stays)
    L.call("mvd_engine_bind_workspace", eng._h, C.c_void_p(eng._ws.data_ptr()), eng._ws.numel(), C.c_void_p(eng._rc.data_ptr()), eng._rc.numel())
    eng._ref_valid = None
    rejected(_raw_args(eng, d, x, t, out, L.MVD_DEEPCACHE_SHALLOW), "MVD_REUSE_REF without a matching cached reference")
    with pytest.raises(L.MvdError, match="no valid reference K/V"):
        _fwd(model, d, x, 500, "reuse")
    # ... and the wrapper's own: other tensors than the refresh call's, and a reset
    assert torch.equal(_fwd(model, d, x, 500, "refresh"), A)              # (cold: the engine's reference was dropped)
    assert torch.equal(_fwd(model, d, x, 500, "reuse"), A)
    with pytest.raises(L.MvdError, match="not those of the preceding"):
        _fwd(model, dict(d, lat=d["lat"].clone()), x, 500, "reuse")
    model.reset_reference_cache()
    with pytest.raises(L.MvdError, match="without a preceding"):
        _fwd(model, d, x, 500, "reuse")
    # without the setting
    model.disable_deepcache()
    model._sync_engine()
    rejected(_raw_args(eng, d, x, t, out, L.MVD_DEEPCACHE_SHALLOW), "without mvd_engine_set_deepcache")
    rejected(_raw_args(eng, d, x, t, out, L.MVD_DEEPCACHE_REFRESH), "without mvd_engine_set_deepcache")
    assert torch.equal(_fwd(model, d, x, 500), A)


def test_hip_graph_replay_of_refresh_and_shallow_forwards(two_steps, clean):
    """the bits are part of the graph key: refresh and shallow forwards replayed as graphs give what plain launches give, in the
    loop's order (refresh, reuse, reuse) three times over -- first use, capture, replay"""
    model, d = clean, two_steps["dev"]
    model.fourier_projection = two_steps["a"]["proj"]
    model.enable_deepcache(3, 0)
    model.cache_reference = True
    seq = [("refresh", d["sample_a"], 500), ("reuse", d["sample_b"], 300), ("reuse", d["sample_a"], 100)]
    _fwd(model, d, d["sample_a"], 900)
    want = [_fwd(model, d, x, t, mode) for mode, x, t in seq]
    assert not torch.equal(want[0], want[2])
    model.use_hip_graph = True
    for rnd in range(3):
        for i, (mode, x, t) in enumerate(seq):
            assert torch.equal(_fwd(model, d, x, t, mode), want[i]), (rnd, i)


# ------------------------------------------------------------------------------------------------ 6. the loop
def test_pipeline_loop_matches_the_oracle_loop(tiny, pipe):
    """the tiny 6-step CFG-3 DDIM loop with interval 3 (refresh, reuse, reuse, refresh, reuse, reuse) against the oracle loop run
    through ``deepcache_ref.deepcache_loop`` + tests/sampler_ref.py.  Bound: 1.5 x the same loop's rel-L2 with DeepCache off against the
    plain oracle loop (measured here), at most 4e-2.  Then ``generate_views`` with 2 views (4 steps: refresh, reuse, reuse, refresh)
    against the per-view oracle loops, under the bound measured the same way.

    Measured on one MI355X (rel-L2): loop off 1.855e-2 -> bound 2.783e-2, on 1.986e-2 (0.339 between the two oracle loops);
    generate_views off 2.342e-2 -> bound 3.513e-2, on 2.058e-2 (0.624 to the plain oracle loops)."""
    from mvd_amd.utils import orbit_cameras
    from tests import sampler_ref as R
    from tests.parity_util import make_inputs, rel_l2
    cfg, params, _ = tiny
    sc = pipe.scheduler.config
    kw = dict(set_alpha_to_one=getattr(sc, "set_alpha_to_one", True), img_ref_scale=0.3, cam_modulation_strength=0.2)
    try:
        # ---- __call__
        steps, gs = 6, 3.0
        inp, src, tgt, neg, lat0 = _loop_inputs(cfg)
        ts = R.timesteps("ddim", sc.num_train_timesteps, steps, sc.timestep_spacing, sc.steps_offset)

        def oracle_loop():
            return R.denoise_loop(params, cfg, pipe.scheduler.betas, inp["text"], neg, lat0, src, tgt, inp["lat"], "ddim", ts, gs,
                                  [inp["proj"]] * steps, **kw)
        want_off = oracle_loop()
        with DR.deepcache_loop(3, 0):
            want_on = oracle_loop()
        pipe.disable_deepcache()
        off = rel_l2(_run_loop(pipe, inp, src, tgt, neg, lat0, steps, gs), want_off)
        bound = min(1.5 * off, LOOP_BOUND_MAX)
        pipe.enable_deepcache(cache_interval=3, cache_branch_id=0)
        got = _run_loop(pipe, inp, src, tgt, neg, lat0, steps, gs)
        err, e_plain = rel_l2(got, want_on), rel_l2(got, want_off)
        print(f"deepcache loop (6 steps, CFG 3, DDIM, interval 3): DeepCache off {off:.3e} -> bound {bound:.3e}; on {err:.3e} to the DeepCache "
              f"oracle loop, {e_plain:.3e} to the plain oracle loop ({rel_l2(want_on, want_off):.3e} between the two oracle loops)", flush=True)
        assert torch.isfinite(got).all() and got.shape == lat0.shape
        assert err <= bound, (err, bound, off)
        # ---- generate_views, 2 views
        V, steps = 2, 4
        one = make_inputs(cfg, 1, 16, 7, seed=23, cam_dim=96)
        g = torch.Generator().manual_seed(6)
        neg1 = torch.randn(1, 7, cfg.cross_attention_dim, generator=g)
        latv = torch.randn(V, 4, 16, 16, generator=g)
        srcv, tgtv = orbit_cameras(1), orbit_cameras(V, elevation_deg=15.0, start_deg=40.0)
        ts = R.timesteps("ddim", sc.num_train_timesteps, steps, sc.timestep_spacing, sc.steps_offset)

        def view_loops(deep):
            rows = []
            for v in range(V):
                with (DR.deepcache_loop(3, 0) if deep else contextlib.nullcontext()):
                    rows.append(R.denoise_loop(params, cfg, pipe.scheduler.betas, one["text"], neg1, latv[v:v + 1], srcv, tgtv[v:v + 1], one["lat"],
                                               "ddim", ts, gs, [one["proj"]] * steps, **kw))
            return torch.cat(rows)

        def views():
            pipe.unet.fourier_projection = one["proj"]
            pipe.unet.cache_reference = True
            return pipe.generate_views(source_camera=srcv[0], target_cameras=tgtv, latents=latv.cuda(), prompt_embeds=one["text"].cuda(),
                                       negative_prompt_embeds=neg1.cuda(), num_inference_steps=steps, guidance_scale=gs,
                                       source_image_latents=one["lat"].cuda(), output_type="latent")["images"].clone()
        want_off, want_on = view_loops(False), view_loops(True)
        pipe.disable_deepcache()
        off = rel_l2(views(), want_off)
        bound = min(1.5 * off, LOOP_BOUND_MAX)
        pipe.enable_deepcache(cache_interval=3, cache_branch_id=0)
        got = views()
        err, e_plain = rel_l2(got, want_on), rel_l2(got, want_off)
        print(f"deepcache generate_views (2 views, 4 steps, CFG 3, DDIM, interval 3): DeepCache off {off:.3e} -> bound {bound:.3e}; on {err:.3e} to "
              f"the DeepCache oracle loops, {e_plain:.3e} to the plain oracle loops", flush=True)
        assert torch.isfinite(got).all() and got.shape == latv.shape
        assert err <= bound, (err, bound, off)
    finally:
        pipe.disable_deepcache()
