"""Token merging in the engine's main pass (``mvd_engine_set_tome``) on the MI355X, tiny topology, against
the ToMe oracle of tests/tome_ref.py run under the ENGINE's own merge decisions (``MVDEngine.tome_tables()``): the same function
under the same decisions.  Decisions themselves are judged at operator level (tests/test_tome_ops_gpu.py): upstream bf16 error
legitimately flips near-ties, so the share of tokens whose slot differs from the oracle's own decisions is printed, not asserted.

The parity bound is measured, not fixed: the rel-L2 of the SAME inputs with ToMe off against the plain oracle (the parent's
figure for that case), times 1.5 (FreeU's precedent for a change that re-rounds bf16 intermediates), and never more than
``tome_ref.PARITY_BOUND_MAX`` = 3e-2, which tests/test_tome_cpu.py shows to be a quarter or less of the distance to every wrong
variant.  Every parity case also has to be at least four bounds away from the forward without ToMe.

Measured on one MI355X (rel-L2; off = ToMe off vs the plain oracle -> bound; on = ToMe on vs the oracle under the engine's tables;
share of slots that differ from the oracle's own decisions -- one flipped src moves the row of every kept src behind it):
  16 x 16: off 1.314e-2 -> 1.970e-2, on 1.303e-2, 12.4 %;  16 x 32: off 1.313e-2 -> 1.970e-2, on 1.360e-2, 13.1 %;
  48 x 48: off 1.255e-2 -> 1.882e-2, on 1.273e-2, 23.9 %;  batch 1: off 1.227e-2 -> 1.840e-2, on 1.281e-2, 13.8 %;
  max_downsample 2: off 1.314e-2 -> 1.970e-2, on 1.316e-2, 15.7 %;  ragged (2, 1), g = 2: off 1.263e-2 -> 1.894e-2, on 1.280e-2;
  every ToMe result 1.5e-1 .. 2.0e-1 from the plain oracle.

What this bound cannot judge: a fault in ONE eligible block.  Every wrong variant priced in tests/test_tome_cpu.py is wrong in all
five blocks at once; a stale or another image's table, ``attn2`` merged as well or an un-merge through the neighbouring row in one
block alone moves the output by 6.6e-2 .. 1.2e-1 on the oracle, and milder faults of one block stay inside 2e-2 (the ``also_ref``
variant of tests/test_todo_engine_gpu.py does).  tests/test_block_parity_options_gpu.py holds every block of a ToMe forward to the
oracle's function of that block on the engine's own input and tables (a single-block fault is 7 bounds away and more there:
tests/test_block_parity_options_cpu.py), also at the SD-2.1 topology, batch 1 and 8, which no test here runs.

The pipeline: ``generate_views`` adds nothing to a forward but the samplers' fused steps, which never see the setting, and the
oracle loop under forced tables would need the tables of every step's forward; the wrapper path it uses
(``MultiViewUNet._ensure_engine``, the cached reference, hipGraph replay) is what the forward tests below exercise, and
tests/test_tome_host_cpu.py checks that the pipeline hands the setting down."""
import pytest
import torch

from tests import tome_ref as T

pytestmark = pytest.mark.gpu


def _pair():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tests.parity_util import build_pair
    return build_pair("tiny", 0, 96, 48, img_ref_scale=0.3)


@pytest.fixture(scope="module")
def tiny():
    return _pair()


@pytest.fixture()
def clean(tiny):
    model = tiny[2]
    model.disable_tome()
    model.tome_keep_tables = False
    yield model
    model.disable_tome()
    model.tome_keep_tables = False
    model.disable_deepcache()
    model.cache_reference = False
    model.use_hip_graph = False
    model.reset_reference_cache()


def _oracle(params, cfg, inp, t=500, rows=slice(None)):
    from oracle import mvd as OM
    with torch.no_grad():
        return OM.multiview_unet_forward(params, cfg, inp["sample"][rows], torch.tensor(t), inp["text"][rows], inp["src"][rows], inp["tgt"][rows],
                                         inp["lat"][rows], fourier_proj=inp["proj"], img_ref_scale=0.3, cam_modulation_strength=0.2)


def _engine(model, inp, t=500, rows=slice(None), **kw):
    model.fourier_projection = inp["proj"]
    with torch.no_grad():
        return model(inp["sample"][rows].cuda(), torch.tensor(t), inp["text"][rows].cuda(), source_camera=inp["src"][rows].cuda(),
                     target_camera=inp["tgt"][rows].cuda(), source_image_latents=inp["lat"][rows].cuda(), **kw).sample.clone()


def _tables(model, batch):
    return {k: v.cpu().reshape(batch, -1) for k, v in model._engine.tome_tables().items()}


def _bound(off_err):
    return min(1.5 * off_err, T.PARITY_BOUND_MAX)


def _flipped(tables, own):
    n = sum(t.numel() for t in tables.values())
    return sum(int((tables[k].long() != own[k]).sum()) for k in tables) / max(n, 1)


@pytest.mark.parametrize("hw,rows,setting", [(16, 2, T.PARITY_SETTING), ((16, 32), 2, T.PARITY_SETTING), (48, 2, T.PARITY_SETTING),
                                             (16, 1, T.PARITY_SETTING), (16, 2, dict(ratio=0.5, max_downsample=2))],
                         ids=["16x16", "16x32", "48x48", "batch1", "max_downsample2"])
def test_tome_forward_matches_the_oracle_under_the_same_decisions(tiny, clean, hw, rows, setting):
    from mvd_amd.unet_params import tome_blocks
    from tests.parity_util import make_inputs, max_rel, rel_l2
    cfg, params, model = tiny
    inp = make_inputs(cfg, 2, hw, 7, 0, 96)
    sl = slice(0, rows)
    plain = _oracle(params, cfg, inp, rows=sl)
    off_out = _engine(model, inp, rows=sl)
    off = rel_l2(off_out, plain)
    bound = _bound(off)
    model.enable_tome(**setting)
    model.tome_keep_tables = True
    got = _engine(model, inp, rows=sl)
    tables = _tables(model, rows)
    h, w = (hw, hw) if isinstance(hw, int) else hw
    expect = tome_blocks(model.unet_config, h, w, **setting)
    assert sorted(tables) == sorted(expect), (sorted(tables), sorted(expect))
    for name, (H, W, r) in expect.items():                       # a valid map with exactly r merged src per image
        nd = (H // 2) * (W // 2)
        dst, src = T.geometry(H, W)
        s = tables[name].long()
        assert ((s >= 0) & (s < H * W - r)).all() and (s[:, dst] == torch.arange(nd)).all() and ((s[:, src] < nd).sum(dim=1) == r).all(), name
    own = {}
    with T.tome_oracle(**setting, record=own):
        _oracle(params, cfg, inp, rows=sl)
    with T.tome_oracle(**setting, tables=tables):
        want = _oracle(params, cfg, inp, rows=sl)
    err = rel_l2(got, want)
    print(f"tome forward hw={hw} rows={rows} {setting}: ToMe off {off:.3e}, bound {bound:.3e}, ToMe on rel-L2 {err:.3e} max {max_rel(got, want):.3e}; "
          f"{100 * _flipped(tables, own):.2f} % of the slots differ from the oracle's own decisions; {rel_l2(got, plain):.3e} to the plain oracle", flush=True)
    assert got.shape == want.shape and torch.isfinite(got).all()
    assert err <= bound, (err, bound, off)
    assert rel_l2(got, off_out.cpu()) >= 4 * bound and rel_l2(got, plain) >= 4 * bound


def test_tome_ragged_forward_under_guidance(tiny, clean):
    """views = (2, 1), g = 2: the ragged forward with ToMe is the three independent ToMe oracle calls, each under its rows' tables"""
    from oracle import mvd as OM
    from tests.parity_util import rel_l2
    from tests.ragged_util import per_row, ragged_case
    _, _, model = tiny
    c = ragged_case((2, 1), 2, 16, 0.3)

    def fwd():
        model.fourier_projection = c.proj
        with torch.no_grad():
            return model(c.sample.cuda(), c.t, c.text.cuda(), source_camera=c.src.cuda(), target_camera=c.tgt.cuda(),
                         source_image_latents=c.lat.cuda(), views=c.counts).sample.clone()
    off_out = fwd()
    off = rel_l2(off_out, c.want)
    bound = _bound(off)
    model.enable_tome(**T.PARITY_SETTING)
    model.tome_keep_tables = True
    got = fwd()
    tables = _tables(model, c.g * c.R)
    obj = [o for o, n in enumerate(c.counts) for _ in range(n)]
    want = torch.empty_like(c.sample)
    for v in range(c.R):
        rows = [j * c.R + v for j in range(c.g)]
        with T.tome_oracle(**T.PARITY_SETTING, tables={k: t[rows] for k, t in tables.items()}), torch.no_grad():
            want[rows] = OM.multiview_unet_forward(c.params, c.cfg, c.sample[rows], c.t, c.text[[j * c.O + obj[v] for j in range(c.g)]], c.src[v:v + 1],
                                                   c.tgt[v:v + 1], c.lat[obj[v]:obj[v] + 1], fourier_proj=c.proj, img_ref_scale=0.3,
                                                   cam_modulation_strength=0.2)
    err, rows_err = rel_l2(got, want), per_row(got, want)
    print(f"tome ragged (2, 1) g=2: ToMe off {off:.3e}, bound {bound:.3e}, ToMe on {err:.3e}; per row " + " ".join(f"{e:.2e}" for e in rows_err), flush=True)
    assert err <= bound, (err, bound)
    assert max(rows_err) <= 2 * bound, rows_err
    assert rel_l2(got, off_out.cpu()) >= 4 * bound


def test_off_settings_are_the_plain_forward_bit_for_bit(tiny, clean):
    """disable_tome() after enable_tome, ratio 0, and a latent at which no block is eligible == a fresh engine's forward"""
    from tests.parity_util import make_inputs
    cfg, _, model = tiny
    inp = make_inputs(cfg, 2, 16, 7, 3, 96)
    _, _, fresh = _pair()
    want = _engine(fresh, inp)
    assert fresh._engine.tome is None
    model.enable_tome(0.5)
    on = _engine(model, inp)
    assert model._engine.tome == (0.5, 1) and not torch.equal(on, want)
    model.disable_tome()
    assert torch.equal(_engine(model, inp), want) and model._engine.tome is None
    model.enable_tome(0.0)
    assert torch.equal(_engine(model, inp), want)
    model.enable_tome(0.01)                 # int(256 * 0.01) = 2 merged src at 16 x 16, but int(64 * 0.01) = 0: with the level-0
    small = make_inputs(cfg, 2, 8, 7, 3, 96)   # maps at 8 x 8 no block merges anything
    got_small = _engine(model, small)
    assert torch.equal(got_small, _engine(fresh, small))


def test_turning_it_off_on_an_engine_sized_with_it_on():
    """a FRESH engine whose first forward runs with token merging on binds the (smaller) workspace of that forward; turning it off
    must size the workspace again -- the next forward runs and equals another fresh engine's, bit for bit; on again likewise"""
    from tests.parity_util import make_inputs
    cfg, _, model = _pair()
    inp = make_inputs(cfg, 2, 16, 7, 3, 96)
    model.enable_tome(0.75)
    on = _engine(model, inp)
    eng = model._engine
    sized_on = eng._ws.numel()
    model.disable_tome()
    off = _engine(model, inp)
    assert eng._ws.numel() > sized_on, (eng._ws.numel(), sized_on)        # (were they equal, this test would show nothing)
    _, _, fresh = _pair()
    assert torch.equal(off, _engine(fresh, inp)) and not torch.equal(on, off)
    model.enable_tome(0.75)
    assert torch.equal(_engine(model, inp), on)
    model.disable_tome()


def test_determinism_deepcache_and_graph_replay(tiny, clean):
    from tests.parity_util import make_inputs
    cfg, _, model = tiny
    inp = make_inputs(cfg, 2, 16, 7, 5, 96)
    dev = {k: inp[k].cuda() for k in ("sample", "text", "src", "tgt", "lat")}
    model.fourier_projection = inp["proj"]

    def fwd(**kw):
        with torch.no_grad():
            return model(dev["sample"], torch.tensor(500), dev["text"], source_camera=dev["src"], target_camera=dev["tgt"],
                         source_image_latents=dev["lat"], **kw).sample.clone()
    off = fwd()
    model.enable_tome(**T.PARITY_SETTING)
    a, b = fwd(), fwd()
    assert torch.equal(a, b) and not torch.equal(a, off)
    # DeepCache: refresh == the ToMe forward, a reuse on unchanged inputs reproduces it (all three with the reference reused)
    model.enable_deepcache(3, 0)
    model.cache_reference = True
    fwd()
    warm = fwd()
    refresh = fwd(deep_cache="refresh")
    reuse = fwd(deep_cache="reuse")
    assert torch.equal(refresh, warm) and torch.equal(reuse, refresh)
    model.disable_deepcache()
    model.cache_reference = False
    # hipGraph: run, capture, replay, replay; a changed setting drops the graph
    model.use_hip_graph = True
    for i, g in enumerate([fwd() for _ in range(4)]):
        assert torch.equal(g, a), i
    model.enable_tome(0.25)
    quarter = [fwd() for _ in range(3)]
    model.disable_tome()
    plain = [fwd() for _ in range(3)]
    model.use_hip_graph = False
    model.enable_tome(0.25)
    want_quarter = fwd()
    assert not torch.equal(want_quarter, a) and not torch.equal(want_quarter, off)
    for i, g in enumerate(quarter):
        assert torch.equal(g, want_quarter), i
    for i, g in enumerate(plain):
        assert torch.equal(g, off), i


def test_a_map_above_the_limit_fails_the_forward_before_any_launch(tiny, clean):
    from mvd_amd._lib import MvdError
    from tests.parity_util import make_inputs
    cfg, _, model = tiny
    inp = make_inputs(cfg, 1, (96, 104), 7, 7, 96)
    model.enable_tome(0.5)
    with pytest.raises(MvdError, match="at most 9216 tokens"):
        _engine(model, inp, rows=slice(0, 1))
