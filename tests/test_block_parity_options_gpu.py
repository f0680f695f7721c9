"""Block-by-block parity of the engine's main pass under token merging (N21), token downsampling (N22) and DeepCache (N20) on the
MI355X, through the main-pass taps -- the form, the fixtures and the bound of tests/test_block_parity_gpu.py:

    || got - want ||  <=  tol * || want - x ||  +  1.25 * || bf16(want) - want ||

``want`` of an eligible transformer block is the OPTION ORACLE's function of the engine's own block input (tests/block_ref.py):
token merging under the engine's own slot tables (``MVDEngine.tome_tables()``), token downsampling by its definition.  The
end-to-end tests (tests/test_tome_engine_gpu.py, tests/test_todo_engine_gpu.py) bound the output at 2e-2 rel-L2 on the tiny
topology; tests/test_block_parity_options_cpu.py prices what that is worth for a fault in ONE block.

Cases (tiny topology, the weights of block_ref.tiny_params; every block through ``check_taps``, so that a workspace the option adds
cannot overwrite a neighbour's tensor unnoticed):
  tome_b2 / tome_b2_md2 / tome_wide_b2       batch 2, 16 x 16 | max_downsample 2: level 1, two heads | 8 x 24
  todo_b2 / todo_b2_area22 / todo_wide_b2    (2, 1, nearest) | (2, 2, area): level 1 | 8 x 24
  tome_views_v2_g2, todo_objects_o2_v2_g2    the Groups of the layout cases
  todo_freeu_b2                              (2, 2, area) under FreeU at the SD-2.1 setting
DeepCache, interval 3, branches 0 and 1, plain and with each option: a refresh forward (every block), then a reuse forward on
the next timestep and a perturbed sample -- every block the shallow forward taps on its own inputs, the first re-run up-block
resnet on the REFRESH forward's tap that tests/deepcache_ref.py defines as the stored feature and the shallow forward's own skip.
Full SD-2.1 size, 64 x 64, camera + image: the eligible transformer blocks and the blocks that read them, batch 1 (ToMe 0.5 |
ToDo (2, 2, area)) and batch 8, rows 0 and 7 (ToMe 0.5 | ToDo (2, 1, nearest)) -- 5 and 10 heads, the packed twins and the .wx
routes, none of which a merged or pooled launch had run under a parity test.
Row independence, bit for bit, with each option on: rows 0 and 2 of every tap, of the output and of the kept slot tables.

THE ROUTES at batch 1 (split-KV from 2048 keys on a nearly empty chip).  The profile's per-shape table shows
what the engine launched; ``mvd_attention_pick_split``, which the engine asks for every attention launch, is then asked through
``ops.attention_pair(nsplit=0)`` on the same arguments and ``ops.last_attention_plan()`` read: a ToMe block at ratio 0.5 launches
2048 queries on (2048 merged keys | 4096 reference keys) x 5 heads -- 640 waves, three key ranges, 480 workgroups; a ToDo block
4096 queries on (1024 pooled keys | 4096) -- the fewest keys are below 2048: unsplit, 320 workgroups.

THE BOUND.  ``block_ref.TOL["attention"]`` = 1e-2 and slack 1.25, untouched.  Nearest single-block wrong variant on the CPU
(tests/test_block_parity_options_cpu.py, distance / ||branch||): token merging 9.4e-2 (un-merge into the neighbouring row at level
1; attn2 merged as well 9.8e-2, the stale table 1.1e-1, another image's table 1.2e-1, merged src left out 3.1e-1); token
downsampling 2.8e-2 (``also_ref``, the one variant below three bounds; f + 1 4.2e-2, the other method 1.3e-1, the corner 1.8e-1).
A third of the nearest caps any raised tolerance: 3.1e-2 for token merging, 9.3e-3 for token downsampling -- BELOW the 1e-2 in
force, so a token-downsampling block has no room to rise at all: had it needed more than 1e-2 that would have been a finding.
What the blocks need is in MEASURED below.
"""
import copy

import pytest
import torch

from tests import test_block_parity_gpu as B
from tests.test_block_parity_gpu import tiny      # noqa: F401  (the fixture: the tiny model with block_ref.tiny_params)

pytestmark = pytest.mark.gpu

# MEASURED on the MI355X: the tolerance the worst block of a kind needs, (|| got - want || - 1.25 || bf16(want) - want ||) / || branch ||
# (worst case of the group; its block)
MEASURED = """
case                          changed blocks: tol needed  error    (block)                     | every other kind
tome_b2                       2.89e-3                      5.16e-3  down_blocks.0.attentions.0   | as the plain tiny cases: attention 3.7e-3
tome_b2_md2                   2.98e-3                      5.29e-3  down_blocks.1.attentions.0   |   (mid_block.attentions.0, never changed),
tome_wide_b2                  2.87e-3                      5.14e-3  down_blocks.0.attentions.0   |   resnet 2.2e-3, resnet_sc 1.5e-3,
tome_views_v2_g2              2.39e-3                      5.04e-3  down_blocks.0.attentions.0   |   conv_in 8.2e-4, samplers 4.5e-4,
todo_b2                       2.91e-3                      5.18e-3  down_blocks.0.attentions.0   |   tail 1.7e-4, FiLM below its rounding term
todo_b2_area22                2.87e-3                      5.19e-3  down_blocks.1.attentions.0   |
todo_wide_b2                  2.83e-3                      5.11e-3  down_blocks.0.attentions.0   |
todo_objects_o2_v2_g2         2.48e-3                      5.13e-3  down_blocks.0.attentions.0   |
todo_freeu_b2                 2.53e-3                      5.26e-3  down_blocks.0.attentions.0   |
deepcache b0 + ToMe           2.89e-3 refresh, 2.88e-3 reuse        down_blocks.0.attentions.0   | reuse: resnet_sc 7.3e-4 (the re-run up-block
deepcache b1 + ToDo           2.91e-3 refresh, 2.83e-3 reuse        down_blocks.0.attentions.0   |   resnets), attention 2.9e-3, resnet 2.0e-3
SD-2.1 64 x 64, ToMe, b1      2.96e-3                      5.26e-3  down_blocks.0.attentions.0   | readers: resnet 3.8e-4, resnet_sc 7.8e-4
SD-2.1 64 x 64, ToDo, b1      2.87e-3                      5.21e-3  down_blocks.1.attentions.0   | readers: resnet 3.7e-4, resnet_sc 7.7e-4
SD-2.1 64 x 64, ToMe, b8      3.09e-3                      5.39e-3  down_blocks.0.attentions.0   | readers: resnet 3.9e-4, resnet_sc 7.3e-4
SD-2.1 64 x 64, ToDo, b8      2.92e-3                      5.21e-3  down_blocks.0.attentions.0   | readers: resnet 2.9e-4, resnet_sc 7.4e-4
A merged block needs 3.1e-3 at most, a pooled one 2.9e-3: less than the plain transformer blocks of the parent file (4.1e-3).  The
bf16 means that merging re-rounds cost nothing that shows at the block; tol = 1e-2 stays for every kind.
Routes at batch 1 (profile): ToMe 5 launches of 2048 queries x (2048 | 4096) keys x 5 heads -> the rule gives 3 key ranges, 480
workgroups; ToDo 5 launches of 4096 x (1024 | 4096) x 5 heads and 5 of 1024 x (256 | 1024) x 10 -> unsplit, 320 workgroups.
"""

TINY_CASES = ("tome_b2", "tome_b2_md2", "tome_wide_b2", "todo_b2", "todo_b2_area22", "todo_wide_b2", "tome_views_v2_g2",
              "todo_objects_o2_v2_g2", "todo_freeu_b2")


def _reset(model):
    model.disable_tome()
    model.disable_todo()
    model.disable_freeu()
    model.disable_deepcache()
    model.tome_keep_tables = model.keep_taps = model.keep_reference_features = False
    model.cache_reference = model.use_hip_graph = False
    model.fourier_projection = None
    model.reset_reference_cache()


def _options_on(model, c):
    if c.freeu is not None:
        model.enable_freeu(**c.freeu)
    if c.tome is not None:
        model.enable_tome(**c.tome)
        model.tome_keep_tables = True
    if c.todo is not None:
        model.enable_todo(**c.todo)


@pytest.fixture()
def clean(tiny):      # noqa: F811
    _reset(tiny[2])
    yield tiny[2]
    _reset(tiny[2])


def _tables(model, c):
    return {k: v.cpu().reshape(c.B, -1) for k, v in model._engine.tome_tables().items()} if c.tome is not None else None


def _option_ran(model, c, cond, tables, executed=None):
    """the engine merged / pooled exactly the blocks ``tome_blocks`` / ``todo_blocks`` name (of ``executed``, a shallow forward)"""
    if c.tome is not None:
        expect = sorted(n for n in cond.merging if executed is None or n in executed)
        assert expect and set(expect) <= set(tables) and (executed is not None or sorted(tables) == expect), (sorted(tables), expect)
    if c.todo is not None:
        keys = model._engine.todo_keys()
        expect = {n: v[3] for n, v in cond.pooling.items() if executed is None or n in executed}
        # (a shallow forward: the counts of the blocks it does not run are not this test's subject)
        assert expect and (keys == expect if executed is None else expect.items() <= keys.items()), (keys, expect)


def _check(model, c, what, rows=None, readers_only=False):
    """one forward of case ``c`` under its options; every block (``readers_only``: the eligible transformer blocks and the blocks
    that read them) against block_ref on the engine's own inputs"""
    from tests import block_ref as R
    _options_on(model, c)
    out, taps, feats = B._forward(model, c)
    tables = _tables(model, c)
    cond = R.case_cond(c, feats, tome_tables=tables)
    _option_ran(model, c, cond, tables)
    inputs = R.input_names(c.cfg, c.cams is not None)
    sliced = rows is not None
    pick = (lambda x: x[rows].cpu()) if sliced else (lambda x: x.cpu())
    taps = {n: pick(x) for n, x in taps.items()}
    only = None
    if readers_only:
        only = R.eligible_and_readers(cond, inputs)
        assert len(only) > len(cond.merging) + len(cond.pooling)
    need = {}
    worst = R.check_taps(cond, taps, inputs, c.sample[rows] if sliced else c.sample, out[rows] if sliced else out, rows=rows, what=what,
                         sliced=sliced, only=only, need=need)
    R.report(what, worst, need)
    assert "attention" in worst
    return worst


@pytest.mark.parametrize("name", TINY_CASES)
def test_every_block_under_the_option(tiny, clean, name):      # noqa: F811
    from tests import block_ref as R
    cfg, params, model, _ = tiny
    cases = R.option_cases(cfg, params)
    assert tuple(cases) == TINY_CASES
    _check(model, cases[name], name)


@pytest.mark.parametrize("branch,option", [(0, None), (1, None), (0, "tome"), (1, "todo")])
def test_deepcache_refresh_and_shallow_forward(tiny, clean, branch, option):      # noqa: F811
    from tests import block_ref as R
    from tests.todo_ref import PARITY_SETTING as TODO
    from tests.tome_ref import PARITY_SETTING as TOME
    cfg, params, model, _ = tiny
    what = f"deepcache_b{branch}_{option or 'plain'}"
    c = R.make_case(what, cfg, params, 2, 16, 7, tome=dict(TOME) if option == "tome" else None, todo=dict(TODO) if option == "todo" else None)
    c2 = copy.copy(c)
    g = torch.Generator().manual_seed(9)
    c2.sample = c.sample + 0.3 * torch.randn(c.sample.shape, generator=g)        # (the next step's latent: near, not equal)
    c2.t = c.t - 20.0
    model.enable_deepcache(3, branch)
    _options_on(model, c)
    lat, text = c.lat.cuda(), c.text.cuda()             # (the same two tensors in both calls: the wrapper's test for "reuse")

    def run(case, mode):
        model.keep_taps = model.keep_reference_features = True
        model.fourier_projection = case.cams[2]
        with torch.no_grad():
            out = model(case.sample.cuda(), case.t.cuda(), text, source_camera=case.cams[0].cuda(), target_camera=case.cams[1].cuda(),
                        source_image_latents=lat, deep_cache=mode).sample.float().cpu()
        return out, {n: x.cpu() for n, x in model.taps().items()}, _tables(model, case)

    inputs = R.input_names(cfg, True)
    out1, taps1, tables1 = run(c, "refresh")
    feats = {n: x.cpu() for n, x in model._engine.features().items()}
    cond1 = R.case_cond(c, feats, tome_tables=tables1)
    _option_ran(model, c, cond1, tables1)
    need = {}
    R.report(what + " refresh", R.check_taps(cond1, taps1, inputs, c.sample, out1, what=what + " refresh", need=need), need)

    out2, taps2, tables2 = run(c2, "reuse")
    names, deep = R.shallow_blocks(cfg, inputs, branch)
    assert list(taps2) + ["conv_out"] == names, (list(taps2), names)
    assert deep not in taps2 and not torch.equal(out2, out1)
    cond2 = R.case_cond(c2, feats, tome_tables=tables2)
    _option_ran(model, c2, cond2, tables2, executed={R.feature_of(n) for n in names if ".attentions." in n})
    need = {}
    worst = R.check_taps(cond2, taps2, {n: inputs[n] for n in names}, c2.sample, out2, what=what + " reuse", extra={deep: taps1[deep]},
                         need=need)
    R.report(what + " reuse", worst, need)
    assert {"conv_in", "attention", "resnet_sc", "tail"} <= set(worst)


def _attention_launches(shapes):
    """[(nq, nk of problem 0, heads, problems, launches)] of the attention rows of ``profile_shapes()``"""
    rows = []
    for line in shapes.splitlines():
        f = dict(kv.split("=") for kv in line.split())
        if 1001 <= int(f["tag"]) <= 1002:
            rows.append((int(f["M"]), int(f["N"]), int(f["K"]), int(f["tag"]) - 1000, int(f["launches"])))
    return rows


def _engine_split(nq, nk, nk_ref, heads):
    """workgroups of ONE two-problem launch of these sizes under the split the engine's rule picks (``nsplit = 0``)"""
    from mvd_amd import ops
    from mvd_amd.packing import QSCALE
    gen = torch.Generator().manual_seed(64)
    rnd = lambda n, s=1.0: (torch.randn(1, n, heads * 64, generator=gen) * s).to(torch.bfloat16).cuda()      # noqa: E731
    ops.attention_pair(dict(q=rnd(nq, QSCALE), k=rnd(nk), v=rnd(nk)), dict(q=rnd(nq, QSCALE), k=rnd(nk_ref), v=rnd(nk_ref)), heads,
                       scale=0.0, nsplit=0)
    plan = ops.last_attention_plan()
    assert plan["waves"] == 4, plan
    return plan["workgroups"]


FULL = [("tome", 1, dict(ratio=0.5, max_downsample=1)), ("todo", 1, dict(factor=2, factor_level_2=2, method="area")),
        ("tome", 8, dict(ratio=0.5, max_downsample=1)), ("todo", 8, dict(factor=2, factor_level_2=1, method="nearest"))]


@pytest.mark.parametrize("option,batch,setting", FULL, ids=[f"{o}_b{b}" for o, b, _ in FULL])
def test_eligible_blocks_and_their_readers_full_size(option, batch, setting):
    """the full SD-2.1 topology at 64 x 64: the eligible transformer blocks and the blocks that read their outputs (everything else
    is held by cases 8 and 9 of tests/test_block_parity_gpu.py)"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import oracle
    from tests import block_ref as R
    from tests import todo_ref as D
    from tests.parity_util import shared_pair
    torch.set_num_threads(oracle.host_threads())
    cfg, params, model = shared_pair("sd21")
    c = R.make_case(f"sd21_{option}_b{batch}", cfg, params, batch, 64, 77, seed=51, cam_dim=1024, **{option: dict(setting)})
    if option == "todo":          # (1024 keys: white noise leaves pooled and full keys too close -- todo_ref.parity_inputs' component)
        even = ((torch.arange(64)[:, None] % 2 == 0) & (torch.arange(64)[None, :] % 2 == 0)).float()
        c.sample = c.sample + D.PERIOD2_AMPLITUDE * (even - (1.0 - even) / 3.0)
    _reset(model)
    eng = model._sync_engine()
    eng.set_profiling(2)            # (records the launches, keeps the forward's own two-stream schedule)
    try:
        _check(model, c, c.name, [0, batch - 1] if batch > 1 else None, readers_only=True)
        launches = _attention_launches(eng.profile_shapes())
        print(f"{c.name}: attention launches (queries, keys, heads, problems, launches): {launches}", flush=True)
        print(f"{c.name}: routes taken (both passes): {B._routes(eng)}", flush=True)
    finally:
        eng.set_profiling(0)
        _reset(model)
    if batch == 1 and option == "tome":
        # five blocks at 64 x 64 merge 4096 tokens into 2048: self + reference in one launch, 5 heads
        assert (2048, 2048, 5, 2, 5) in launches, launches
        assert _engine_split(2048, 2048, 4096, 5) == 16 * 5 * 2 * 3          # 640 waves < 1024, 2048 keys or more: three key ranges
    if batch == 1 and option == "todo":
        assert (4096, 1024, 5, 2, 5) in launches and (1024, 256, 10, 2, 5) in launches, launches
        assert _engine_split(4096, 1024, 4096, 5) == 32 * 5 * 2              # 1024 pooled keys: below 2048, unsplit


@pytest.mark.parametrize("option", ["tome", "todo"])
def test_rows_do_not_depend_on_another_row_under_the_option(tiny, clean, option):      # noqa: F811
    """tests/test_block_parity_gpu.py's test on ``uniform_b3_cam_img`` with the option on: row 1's sample, text, camera, timestep
    changed in turn -- rows 0 and 2 of every tap, of the output and of the kept slot tables keep their bits"""
    from tests.todo_ref import PARITY_SETTING as TODO
    from tests.tome_ref import PARITY_SETTING as TOME
    _cfg, _params, model, cases = tiny
    c = cases["uniform_b3_cam_img"]
    if option == "tome":
        model.enable_tome(**TOME)
        model.tome_keep_tables = True
    else:
        model.enable_todo(**TODO)
    g = torch.Generator().manual_seed(5)
    model.keep_taps = True
    eng = model._sync_engine()
    enc_text = c.text.cuda().contiguous()

    def run(sample=None, text=None, t=None, tgt=None):
        out = eng.forward((c.sample if sample is None else sample).cuda(), (c.t if t is None else t).cuda(),
                          (c.text if text is None else text).cuda(), source_latents=c.lat.cuda(), encoder_text=enc_text,
                          source_camera=c.cams[0].cuda(), target_camera=(c.cams[1] if tgt is None else tgt).cuda(), fourier_proj=c.cams[2].cuda())
        taps = {n: x.cpu() for n, x in eng.taps().items()}
        taps["conv_out"] = out.cpu()
        if option == "tome":
            tables = {f"table {k}": v.cpu().reshape(c.B, -1).float() for k, v in eng.tome_tables().items()}
            assert len(tables) == 5
            taps.update(tables)
        else:
            assert len(eng.todo_keys()) == 5
        return taps

    base = run()
    B._same_rows(base, run(), [0, 1, 2], f"{option}: the same forward again")
    sample, text, t, tgt = c.sample.clone(), c.text.clone(), c.t.clone(), c.cams[1].clone()
    sample[1] = torch.randn(sample[1].shape, generator=g)
    text[1] = torch.randn(text[1].shape, generator=g)
    t[1] = 777.0
    tgt[1] = c.cams[1][0] @ torch.diag(torch.tensor([1.0, -1.0, -1.0, 1.0]))
    for what, v in dict(sample=sample, text=text, t=t, tgt=tgt).items():
        got = run(**{what: v})
        assert not torch.equal(got["conv_out"][1], base["conv_out"][1]), f"{option}: changing row 1's {what} changed nothing"
        B._same_rows(base, got, [0, 2], f"{option}: row 1's {what} changed")
