"""Token downsampling of the self-attention keys in the engine's main pass (``mvd_engine_set_todo``) on
the MI355X, tiny topology, against the ToDo oracle of tests/todo_ref.py.

The parity bound is measured, not fixed: the rel-L2 of the SAME inputs with the switch off against the plain oracle, times 1.5
(FreeU's and token merging's precedent for a change that re-rounds bf16 intermediates), and never more than
``todo_ref.PARITY_BOUND_MAX`` = 3e-2, which tests/test_todo_cpu.py shows to be a quarter or less of the distance to the wrong
variants it can judge.  Every parity case also has to be at least four bounds away from the forward with the switch off and from
the plain oracle, ``todo_keys()`` has to name exactly the blocks of ``todo_blocks`` with their key counts, and at 16 x 16 the
result has to lie closer to the right oracle than to the one that downsamples the reference K/V as well (``also_ref``, which the
bound cannot judge).

Measured on one MI355X (rel-L2; off = switch off vs the plain oracle -> bound; on = ToDo on vs the ToDo oracle; then the distance to
the switch-off forward / to the plain oracle):
  16 x 16 (2, 1, nearest): off 1.314e-2 -> 1.970e-2, on 1.301e-2; 1.886e-1 / 1.891e-1; to the ``also_ref`` oracle 2.167e-2
  16 x 32 (2, 1, nearest): off 1.313e-2 -> 1.970e-2, on 1.314e-2; 1.489e-1 / 1.486e-1
  48 x 48 (2, 1, nearest), sample with the period-2 component: off 1.273e-2 -> 1.910e-2, on 1.262e-2; 2.735e-1 / 2.732e-1
  16 x 16 (2, 2, area):    off 1.314e-2 -> 1.970e-2, on 1.232e-2; 2.181e-1 / 2.186e-1; to the ``also_ref`` oracle 3.985e-2
  16 x 16 (4, 1, nearest), 16 keys: off 1.314e-2 -> 1.970e-2, on 1.431e-2; 3.719e-1 / 3.720e-1; to the ``also_ref`` oracle 4.567e-2
  batch 1 (2, 1, nearest): off 1.227e-2 -> 1.840e-2, on 1.284e-2; 1.901e-1 / 1.910e-1
  ragged (2, 1), g = 2:    off 1.263e-2 -> 1.894e-2, on 1.266e-2 (rows 1.13e-2 .. 1.52e-2); 1.877e-1 / 1.879e-1
  FreeU (SD-2.1 setting) + (2, 2, area): off 1.293e-2 -> 1.940e-2, on 1.226e-2; 2.176e-1 / 2.178e-1

What this bound cannot judge is judged block by block in tests/test_block_parity_options_gpu.py: every block of a ToDo forward
against the ToDo oracle's function of that block on the engine's own input.  ``also_ref`` is the example -- 2.17e-2 from the
engine's result here, beside a bound of 1.97e-2, and in ONE block it moves the oracle's output by 1.3e-2 .. 1.4e-2, inside the
bound; at the block it is 2.8e-2 of the branch and more, two block bounds away and more (tests/test_block_parity_options_cpu.py),
so an engine that pooled the reference K/V in one block would fail there.  The same file runs ToDo at the SD-2.1 topology (5 and
10 heads, batch 1 and 8), which no test here does.

The inputs are ``parity_util.make_inputs``' at seed 0, as in the token-merging engine test, with one exception that
``todo_ref.parity_inputs`` states and tests/test_todo_cpu.py justifies on the ORACLE alone: under white noise the distance between
downsampling on and off falls like 1 / sqrt(keys) -- the oracle's own two results are 5.6e-2 apart at 48 x 48 (576 keys), the engine's
were 5.7e-2 apart, less than four parity bounds (7.5e-2), so there the test could not have told a forward that ignores the switch
from one that honours it.  The 48 x 48 sample therefore carries a zero-mean component of period 2 (what ``nearest`` keeps differs
from what it drops); the bound is measured on those same inputs with the switch off."""
import pytest
import torch

from tests import todo_ref as T

pytestmark = pytest.mark.gpu

NEAREST = T.PARITY_SETTING
AREA22 = dict(factor=2, factor_level_2=2, method="area")
NEAREST4 = dict(factor=4, factor_level_2=1, method="nearest")


def _pair():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tests.parity_util import build_pair
    return build_pair("tiny", 0, 96, 48, img_ref_scale=0.3)


@pytest.fixture(scope="module")
def tiny():
    return _pair()


def _reset(model):
    model.disable_todo()
    model.disable_tome()
    model.disable_freeu()
    model.disable_deepcache()
    model.cache_reference = False
    model.use_hip_graph = False
    model.reset_reference_cache()


@pytest.fixture()
def clean(tiny):
    _reset(tiny[2])
    yield tiny[2]
    _reset(tiny[2])


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


def _bound(off_err):
    return min(1.5 * off_err, T.PARITY_BOUND_MAX)


def _expected_keys(model, hw, setting):
    from mvd_amd.unet_params import todo_blocks
    h, w = (hw, hw) if isinstance(hw, int) else hw
    return {name: v[3] for name, v in todo_blocks(model.unet_config, h, w, setting["factor"], setting["factor_level_2"]).items()}


@pytest.mark.parametrize("hw,rows,setting", [(16, 2, NEAREST), ((16, 32), 2, NEAREST), (48, 2, NEAREST), (16, 2, AREA22), (16, 2, NEAREST4), (16, 1, NEAREST)],
                         ids=["16x16", "16x32", "48x48", "2_2_area", "4_1_nearest_16_keys", "batch1"])
def test_todo_forward_matches_the_todo_oracle(tiny, clean, hw, rows, setting):
    from tests.parity_util import max_rel, rel_l2
    cfg, params, model = tiny
    inp = T.parity_inputs(cfg, 2, hw)          # (make_inputs' seed 0; at 48 x 48 plus a period-2 component: see todo_ref.parity_inputs)
    sl = slice(0, rows)
    plain = _oracle(params, cfg, inp, rows=sl)
    off_out = _engine(model, inp, rows=sl)
    assert model._engine.todo_keys() == {}
    off = rel_l2(off_out, plain)
    bound = _bound(off)
    model.enable_todo(**setting)
    got = _engine(model, inp, rows=sl)
    keys = model._engine.todo_keys()
    assert keys == _expected_keys(model, hw, setting) and keys, keys
    rec = {}
    with T.todo_oracle(**setting, record=rec):
        want = _oracle(params, cfg, inp, rows=sl)
    assert rec == keys
    err = rel_l2(got, want)
    print(f"todo forward hw={hw} rows={rows} {setting}: off {off:.3e}, bound {bound:.3e}, on rel-L2 {err:.3e} max {max_rel(got, want):.3e}; "
          f"{rel_l2(got, off_out.cpu()):.3e} to the switch-off forward, {rel_l2(got, plain):.3e} to the plain oracle", flush=True)
    assert got.shape == want.shape and torch.isfinite(got).all()
    assert err <= bound, (err, bound, off)
    assert rel_l2(got, off_out.cpu()) >= 4 * bound and rel_l2(got, plain) >= 4 * bound
    if hw == 16 and rows == 2:
        with T.todo_oracle(**setting, also_ref=True):
            wrong = rel_l2(got, _oracle(params, cfg, inp, rows=sl))
        print(f"    to the oracle that downsamples the reference K/V too: {wrong:.3e}", flush=True)
        assert err < wrong, (err, wrong)


def test_todo_ragged_forward_under_guidance(tiny, clean):
    """views = (2, 1), g = 2: the ragged forward with ToDo is the three independent ToDo oracle calls"""
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
    model.enable_todo(**NEAREST)
    got = fwd()
    assert model._engine.todo_keys() == _expected_keys(model, 16, NEAREST)
    obj = [o for o, n in enumerate(c.counts) for _ in range(n)]
    want = torch.empty_like(c.sample)
    for v in range(c.R):
        rows = [j * c.R + v for j in range(c.g)]
        with T.todo_oracle(**NEAREST), torch.no_grad():
            want[rows] = OM.multiview_unet_forward(c.params, c.cfg, c.sample[rows], c.t, c.text[[j * c.O + obj[v] for j in range(c.g)]], c.src[v:v + 1],
                                                   c.tgt[v:v + 1], c.lat[obj[v]:obj[v] + 1], fourier_proj=c.proj, img_ref_scale=0.3,
                                                   cam_modulation_strength=0.2)
    err, rows_err = rel_l2(got, want), per_row(got, want)
    print(f"todo ragged (2, 1) g=2: off {off:.3e}, bound {bound:.3e}, on {err:.3e}; per row " + " ".join(f"{e:.2e}" for e in rows_err) +
          f"; {rel_l2(got, off_out.cpu()):.3e} to the switch-off forward, {rel_l2(got, c.want):.3e} to the plain oracle", flush=True)
    assert err <= bound, (err, bound)
    assert max(rows_err) <= 2 * bound, rows_err
    assert rel_l2(got, off_out.cpu()) >= 4 * bound and rel_l2(got, c.want) >= 4 * bound


def test_parity_with_freeu_on(tiny, clean):
    from tests import freeu_ref as FR
    from tests.parity_util import make_inputs, rel_l2
    cfg, params, model = tiny
    inp = make_inputs(cfg, 2, 16, 7, 0, 96)
    model.enable_freeu(**FR.SD21)
    with FR.freeu_oracle(**FR.SD21):
        plain = _oracle(params, cfg, inp)
        with T.todo_oracle(**AREA22):
            want = _oracle(params, cfg, inp)
    off_out = _engine(model, inp)
    off = rel_l2(off_out, plain)
    bound = _bound(off)
    model.enable_todo(**AREA22)
    got = _engine(model, inp)
    err = rel_l2(got, want)
    print(f"todo with FreeU {AREA22}: off {off:.3e}, bound {bound:.3e}, on {err:.3e}; {rel_l2(got, off_out.cpu()):.3e} to the switch-off forward, "
          f"{rel_l2(got, plain):.3e} to the FreeU oracle without ToDo", flush=True)
    assert err <= bound, (err, bound)
    assert rel_l2(got, off_out.cpu()) >= 4 * bound and rel_l2(got, plain) >= 4 * bound


def test_off_settings_are_the_plain_forward_bit_for_bit(tiny, clean):
    """disable_todo() after enable_todo and factors (1, 1) == a fresh engine's forward; the smallest maps"""
    from tests.parity_util import make_inputs
    cfg, _, model = tiny
    inp = make_inputs(cfg, 2, 16, 7, 3, 96)
    _, _, fresh = _pair()
    want = _engine(fresh, inp)
    assert fresh._engine.todo is None and fresh._engine.todo_keys() == {}
    model.enable_todo(2, 2, "area")
    on = _engine(model, inp)
    assert model._engine.todo == (2, 2, "area") and not torch.equal(on, want)
    model.disable_todo()
    assert torch.equal(_engine(model, inp), want) and model._engine.todo is None and model._engine.todo_keys() == {}
    model.enable_todo(1, 1, "area")
    assert torch.equal(_engine(model, inp), want) and model._engine.todo_keys() == {}
    # the engine's own (1, 1): set, not cleared
    model._engine.set_todo(1, 1, "nearest")
    assert torch.equal(_engine(model, inp), want)
    model._engine.clear_todo()
    # the smallest maps the engine meets: a latent is a multiple of 8 per side, so a level-1 map has at least 4 rows and columns and
    # H // f >= 1 holds for every f <= 4 -- "a map too small for the factor" cannot arise in a forward of this topology; the rule is
    # pinned where it can be met, by the operator's refusal (tests/test_todo_ops_gpu.py).  What can be met: ONE key per image
    # (4 x 4 under 4), one row of keys (4 x 12 under 4), and level 0 untouched while level 1 is downsampled
    narrow = make_inputs(cfg, 2, (8, 24), 7, 3, 96)
    model.enable_todo(1, 4)
    got = _engine(model, narrow)
    assert model._engine.todo_keys() == _expected_keys(model, (8, 24), dict(factor=1, factor_level_2=4)) and set(model._engine.todo_keys().values()) == {3}
    assert torch.isfinite(got).all() and not torch.equal(got, _engine(fresh, narrow))
    small = make_inputs(cfg, 2, 8, 7, 3, 96)
    model.enable_todo(4, 4)
    got = _engine(model, small)
    assert sorted(set(model._engine.todo_keys().values())) == [1, 4] and torch.isfinite(got).all()
    model.disable_todo()
    assert torch.equal(_engine(model, small), _engine(fresh, small))


def test_determinism_graph_replay_deepcache_and_the_mutual_refusal(tiny, clean):
    from mvd_amd._lib import MvdError
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
    model.enable_todo(**NEAREST)
    a, b = fwd(), fwd()
    assert torch.equal(a, b) and not torch.equal(a, off)
    # DeepCache: refresh == the ToDo forward, a reuse on unchanged inputs reproduces it (all three with the reference reused)
    model.enable_deepcache(3, 0)
    model.cache_reference = True
    fwd()
    warm = fwd()
    refresh = fwd(deep_cache="refresh")
    reuse = fwd(deep_cache="reuse")
    assert torch.equal(refresh, warm) and torch.equal(reuse, refresh)
    # a deep feature stored under another setting is stale: the wrapper forgets it ...
    model.enable_todo(**AREA22)
    with pytest.raises(MvdError, match="without a preceding"):
        fwd(deep_cache="reuse")
    refresh22 = fwd(deep_cache="refresh")
    assert not torch.equal(refresh22, refresh) and torch.equal(fwd(deep_cache="reuse"), refresh22)
    # ... and the engine itself refuses before any launch when only IT was told (same values: the wrapper sees no change)
    model._engine.set_todo(*model.todo)
    with pytest.raises(MvdError, match="without a stored deep feature"):
        fwd(deep_cache="reuse")
    model._engine.clear_todo()
    model._engine.set_todo(*model.todo)
    assert torch.equal(fwd(deep_cache="refresh"), refresh22)
    model.disable_deepcache()
    model.cache_reference = False
    model.reset_reference_cache()
    model.enable_todo(**NEAREST)
    # hipGraph: run, capture, replay, replay; a changed setting drops the graph
    model.use_hip_graph = True
    for i, g in enumerate([fwd() for _ in range(4)]):
        assert torch.equal(g, a), i
        assert model._engine.todo_keys() == _expected_keys(model, 16, NEAREST)
    model.enable_todo(**NEAREST4)
    four = [fwd() for _ in range(3)]
    model.disable_todo()
    plain = [fwd() for _ in range(3)]
    model.use_hip_graph = False
    model.enable_todo(**NEAREST4)
    want_four = fwd()
    assert not torch.equal(want_four, a) and not torch.equal(want_four, off)
    for i, g in enumerate(four):
        assert torch.equal(g, want_four), i
    for i, g in enumerate(plain):
        assert torch.equal(g, off), i
    # ToDo and ToMe are alternatives, on the wrapper and on the engine
    with pytest.raises(ValueError, match="alternatives"):
        model.enable_tome(0.5)
    with pytest.raises(MvdError, match="alternatives"):
        model._engine.set_tome(0.5)
    assert torch.equal(fwd(), want_four)                           # the refusals changed nothing
    model.disable_todo()
    model.enable_tome(0.5)
    merged = fwd()
    with pytest.raises(ValueError, match="alternatives"):
        model.enable_todo()
    with pytest.raises(MvdError, match="alternatives"):
        model._engine.set_todo(2, 1, "nearest")
    assert torch.equal(fwd(), merged) and model._engine.todo is None
    model.disable_tome()
    model.enable_todo(**NEAREST4)                                  # one off, the other on, in one step of the wrapper
    assert torch.equal(fwd(), want_four)


def test_a_workspace_sized_with_the_switch_off():
    """the wrapper sizes the workspace again when the setting changes; an engine told behind the wrapper's back either still fits
    or is refused by the dry run in front of every forward -- nothing is launched into a workspace that is too small"""
    from mvd_amd import _lib as L
    from tests.parity_util import make_inputs
    cfg, _, model = _pair()
    inp = make_inputs(cfg, 2, 16, 7, 3, 96)
    off = _engine(model, inp)
    eng = model._engine
    sized_off = eng._ws.numel()
    model.enable_todo(**AREA22)
    on = _engine(model, inp)
    print(f"workspace, tiny at 16 x 16, batch 2: off {sized_off} bytes, (2, 2, area) {eng._ws.numel()} bytes", flush=True)
    assert eng._ws.numel() >= sized_off and not torch.equal(on, off)
    _, _, other = _pair()
    assert torch.equal(_engine(other, inp), off)
    L.call("mvd_engine_set_todo", other._engine._h, 2, 2, 1)       # behind the wrapper's back: its workspace is the switch-off one
    try:
        got = _engine(other, inp)
    except L.MvdError as e:
        assert "workspace too small" in str(e), str(e)
        print("    behind the wrapper's back: refused, " + str(e), flush=True)
    else:
        assert torch.equal(got, on)
        print("    behind the wrapper's back: the switch-off workspace still fits", flush=True)
    L.call("mvd_engine_clear_todo", other._engine._h)
    assert torch.equal(_engine(other, inp), off)
