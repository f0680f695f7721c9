"""Block-by-block parity of the engine's main pass on the MI355X, through the main-pass taps (``mvd_engine_set_taps``).

One forward per case with taps on; every tapped block is held to the ORACLE's function of that block, run on the engine's own
input tensors of the block (tests/block_ref.py: "teacher forcing"), in the form of tests/branch_check.py:

    || got - want ||  <=  tol * || want - x ||  +  1.25 * || bf16(want) - want ||

x: the residual input where the block has one of the output's shape, else 0.  The end-to-end tests bound the output at rel-L2
2e-2 against ~1.3e-2 already present; half of 102 single-site wiring faults (one adapter branch dropped or fed another row's
reference, one FiLM modulator dropped or fed another row's camera, one attn2 reading another row's text) move the output by
less than 1.5e-2.  At the block the same faults are 5 % of the branch and more.

Cases (tiny topology unless stated; the seeded weights with the adapter's out-projections scaled up, block_ref.tiny_params):
 1 uniform batch 1 and 3, 16 x 16, text 7, one timestep per row: camera + image, each alone, neither
 2 batch 3, 8 x 24 latents, text 77, camera + image: ragged tiles at every level, non-square maps
 3 guidance form, sample batch 4 on reference batch 2, image: Q4 re-chunking, the encoder-text selection
 4 shared views V = 2, g = 2;  5 objects O = 2, V = 2, g = 2;  6 ragged counts (2, 1), g = 2 -- image; the reference of each is
   the independent per-row oracle block calls of the layout's definition (helpers of objects_util / ragged_util)
 7 FreeU (the published SD-2.1 setting), image: the up-block resnets read the re-weighted pair, the taps hold the plain one
 8 full SD-2.1 size, 64 x 64, batch 1, camera + image: the packed twins of the batch-1 routes (.ws, .wf/.cf, tail.w, ...)
 9 full SD-2.1 size, 64 x 64, batch 8, camera + image: the tiled and X-stationary routes (.wx, .w4); rows 0 and 7 are compared,
   the adapter's Q2 statistics run over all eight rows of the engine's kept features
Cases 1 and 2 are the smallest shapes at which every level still has a map of 2 x 2 or more.

Row independence is exact (no tolerance): batch 3, row 1's sample, text, camera and timestep changed in turn -- rows 0 and 2 of
every tap and of the output keep their bits; the same in the guidance form (6 rows on 3).  The reference latents are left alone:
Q2 couples the rows by definition.

The taps themselves: the output with taps on is the output with taps off (torch.equal) -- also under use_hip_graph, under
cache_reference and in a DeepCache shallow forward, which taps the blocks it executes; with taps off the workspace size is what
it was, and taps on adds no launch.

THE BOUND.  slack 1.25 and tol 1e-2 are branch_check.py's defaults.  Nearest wrong variant per block kind over all cases, on the
CPU (tests/test_block_parity_cpu.py, distance / ||branch||, worst block): attention 5.4e-2 (the two adapter processors exchanged;
to_out_ref bias left out 9.7e-2, another row's reference 6.8e-2, a branch dropped 2.0e-1, another row's text 1.9e-1), resnet
4.8e-2 (another row's time projection; the neighbouring slice 5.9e-2, hidden / skip swapped 4.7e-1, the skip after FiLM 2.9e-1,
FreeU left out 2.0e-1), FiLM 7.0e-2 (another row's camera; the neighbouring modulator 1.9e-1); a third of the nearest caps any
tolerance of its kind.  Measured on the MI355X: the table MEASURED below (every kind fits 1e-2: attention, the
largest, needs 4.1e-3).
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

# MEASURED on the MI355X, worst block of all cases of a size, per block kind: the tolerance the block needs, (|| got - want || -
# 1.25 || bf16(want) - want ||) / || branch ||; its error / || branch ||; the largest fraction of the bound (tol 1e-2) a test printed
MEASURED = """
kind          tiny: tol needed  error    of bound | SD-2.1 64 x 64, batch 1 and 8: tol needed  error
attention     4.1e-3            6.3e-3   0.52     | 3.0e-3   5.3e-3     (mid_block.attentions.0)
resnet        2.1e-3            4.4e-3   0.54     | 2.1e-3   4.4e-3     (down_blocks.0.resnets.0; of the bound: mid_block.resnets.1)
resnet_sc     1.6e-3            3.6e-3   0.30     | 1.7e-3   3.7e-3     (down_blocks.1.resnets.0)
conv_in       8.2e-4            2.9e-3   0.24     | 6.9e-4   2.8e-3
downsampler   3.7e-4            2.4e-3   0.20     | 3.1e-4   2.4e-3
upsampler     3.3e-4            2.4e-3   0.20     | 3.0e-4   2.4e-3
tail          2.2e-4            2.2e-3   0.19     | 1.8e-4   2.2e-3
film          < 0               1.7e-3   0.14     | < 0      1.7e-3     (below its own rounding term)
Every kind fits tol = 1e-2 (block_ref.TOL), which therefore stays; the nearest wrong variants (the docstring above) are 4.8e-2 and up.
"""


@pytest.fixture(scope="module")
def tiny():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import oracle
    from mvd_amd.config import UNetConfig
    from mvd_amd.mvd_unet import MultiViewUNet
    from tests import block_ref as R
    torch.set_num_threads(oracle.host_threads())
    cfg, params = R.tiny_params()
    model = MultiViewUNet(None, unet_config=UNetConfig.tiny(), init="empty", img_ref_scale=0.3, cam_modulation_strength=0.2,
                          cam_output_dim=96, cam_hidden_dim=48)
    missing, unexpected = model.load_state_dict(params, strict=False)
    assert not missing and not unexpected, (missing[:5], unexpected[:5])
    model = model.to("cuda").eval()
    return cfg, params, model, R.tiny_cases(cfg, params)


def _forward(model, c, taps=True, sample=None, text=None, t=None, tgt=None, **kw):
    """one forward of case ``c`` (inputs optionally replaced); (out, taps, feats) on the CPU, taps / feats None when not kept"""
    model.keep_taps = taps
    model.keep_reference_features = taps and c.lat is not None
    args = {}
    if c.cams is not None:
        model.fourier_projection = c.cams[2]
        args.update(source_camera=c.cams[0].cuda(), target_camera=(c.cams[1] if tgt is None else tgt).cuda())
    if c.lat is not None:
        args.update(source_image_latents=c.lat.cuda())
    try:
        with torch.no_grad():
            out = model((c.sample if sample is None else sample).cuda(), (c.t if t is None else t).cuda(),
                        (c.text if text is None else text).cuda(), **args, **c.kw, **kw).sample
        tp = fe = None
        if taps:
            tp = model.taps()
            if c.lat is not None:
                fe = {n: x.cpu() for n, x in model._engine.features().items()}
        return out.float().cpu(), tp, fe
    finally:
        model.fourier_projection = None
        model.keep_taps = model.keep_reference_features = False


def _check(model, c, what, rows=None):
    from tests import block_ref as R
    if c.freeu is not None:
        model.enable_freeu(**c.freeu)
    try:
        out, taps, feats = _forward(model, c)
    finally:
        if c.freeu is not None:
            model.disable_freeu()
    sliced = rows is not None
    pick = (lambda x: x[rows].cpu()) if sliced else (lambda x: x.cpu())
    taps = {n: pick(x) for n, x in taps.items()}
    cond = R.case_cond(c, feats)
    worst = R.check_taps(cond, taps, R.input_names(c.cfg, c.cams is not None), c.sample[rows] if sliced else c.sample,
                         out[rows] if sliced else out, rows=rows, what=what, sliced=sliced)
    R.report(what, worst)
    return worst


TINY_CASES = ("uniform_b1_cam_img", "uniform_b3_cam_img", "uniform_b3_cam", "uniform_b3_img", "uniform_b3_plain", "wide_b3_cam_img",
              "guidance_4_on_2", "views_v2_g2", "objects_o2_v2_g2", "ragged_2_1_g2", "freeu_b2_img")


@pytest.mark.parametrize("name", TINY_CASES)
def test_every_block_on_its_own_inputs(tiny, name):
    _cfg, _params, model, cases = tiny
    assert tuple(cases) == TINY_CASES
    _check(model, cases[name], name)


def _routes(eng):
    s = eng.profile_summary()
    return ", ".join(f"{k} x{v['launches']}" for k, v in sorted(s.items()))


@pytest.mark.parametrize("batch,rows", [(1, None), (8, [0, 7])])
def test_every_block_full_size(batch, rows):
    """cases 8 and 9: the full SD-2.1 topology at 64 x 64 -- the slots and routes the tiny configuration never reads"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import oracle
    from tests import block_ref as R
    from tests.parity_util import shared_pair
    torch.set_num_threads(oracle.host_threads())
    cfg, params, model = shared_pair("sd21")
    c = R.make_case(f"sd21_b{batch}", cfg, params, batch, 64, 77, seed=51, cam_dim=1024)
    eng = model._sync_engine()
    eng.set_profiling(2)            # (records the launches, keeps the forward's own two-stream schedule)
    try:
        _check(model, c, c.name, rows)
        print(f"{c.name}: routes taken (both passes): {_routes(eng)}", flush=True)
    finally:
        eng.set_profiling(0)


def _same_rows(a, b, rows, what):
    from tests.exact_util import assert_same_bits
    for n in a:
        assert_same_bits(b[n][rows], a[n][rows], f"{what}: first tap that differs: {n}")


# taps that may depend on another row, by name, with the reason (none: every kernel of the main pass is row-wise)
ROW_COUPLED = {}


@pytest.mark.parametrize("name,others", [("uniform_b3_cam_img", [0, 2]), ("guidance_6_on_3", [0, 2, 3, 4, 5])])
def test_rows_do_not_depend_on_another_row(tiny, name, others):
    """row 1's sample, text, camera, timestep changed in turn: every other row of every tap and of the output keeps its bits"""
    from tests import block_ref as R
    cfg, params, model, cases = tiny
    c = cases[name] if name in cases else R.make_case(name, cfg, params, 6, 16, 7, cam=False, ref_batch=3)
    g = torch.Generator().manual_seed(5)
    model.keep_taps = True
    eng = model._sync_engine()
    # the encoder pass's inputs stay as they are (the rows of the reference are coupled by Q2): the engine's own entry, whose
    # encoder text is an argument of its own -- the rows MultiViewUNet.forward selects from the unchanged text
    enc_text = (c.text if c.text.shape[0] == c.lat.shape[0] else c.text[c.lat.shape[0]:]).cuda().contiguous()

    def run(sample=None, text=None, t=None, tgt=None):
        cam = {}
        if c.cams is not None:
            cam = dict(source_camera=c.cams[0].cuda(), target_camera=(c.cams[1] if tgt is None else tgt).cuda(), fourier_proj=c.cams[2].cuda())
        out = eng.forward((c.sample if sample is None else sample).cuda(), (c.t if t is None else t).cuda(),
                          (c.text if text is None else text).cuda(), source_latents=c.lat.cuda(), encoder_text=enc_text, **cam)
        taps = {n: x.cpu() for n, x in eng.taps().items() if n not in ROW_COUPLED}
        taps["conv_out"] = out.cpu()
        return taps

    base = run()
    _same_rows(base, run(), list(range(c.B)), f"{name}: the same forward again")
    sample = c.sample.clone()
    sample[1] = torch.randn(sample[1].shape, generator=g)
    text = c.text.clone()
    text[1] = torch.randn(text[1].shape, generator=g)
    t = c.t.clone()
    t[1] = 777.0
    changes = dict(sample=sample, text=text, t=t)
    if c.cams is not None:
        tgt = c.cams[1].clone()
        tgt[1] = c.cams[1][0] @ torch.diag(torch.tensor([1.0, -1.0, -1.0, 1.0]))
        changes["tgt"] = tgt
    try:
        for what, v in changes.items():
            got = run(**{what: v})
            assert not torch.equal(got["conv_out"][1], base["conv_out"][1]), f"{name}: changing row 1's {what} changed nothing"
            _same_rows(base, got, others, f"{name}: row 1's {what} changed")
    finally:
        model.keep_taps = False
        model.reset_reference_cache()


def _launches(eng):
    return sum(v["launches"] for v in eng.profile_summary().values())


def test_taps_change_nothing(tiny):
    """taps off: the workspace size and the launches of a forward are what they were; taps on: the same output bit for bit, the
    same number of launches, the FiLM outputs counted in the workspace"""
    from mvd_amd import _lib as L
    _cfg, _params, model, cases = tiny
    c = cases["uniform_b3_cam_img"]
    off, _, _ = _forward(model, c, taps=False)
    eng = model._engine
    size = lambda: L.lib().mvd_engine_workspace_bytes(eng._h, 3, 16, 16, 7, 3)      # noqa: E731
    ws_off = size()
    assert L.lib().mvd_engine_num_taps(eng._h) == -1 and "not kept" in L.last_error()
    on, taps, _ = _forward(model, c)
    assert torch.equal(on, off)
    eng.set_taps(True)
    ws_on = size()
    assert L.lib().mvd_engine_num_taps(eng._h) == 0          # switching drops the records of the forward before
    eng.set_taps(False)
    # mid_0 is the identity; up_0 .. up_3 get an output of their own: B H W C bf16 each, 256-byte granules
    extra = sum(3 * (16 >> lv) ** 2 * ch * 2 for lv, ch in ((2, 128), (1, 128), (0, 128), (0, 64)))
    assert ws_off > 0 and size() == ws_off and extra <= ws_on - ws_off <= extra + 4 * 256, (ws_off, ws_on, extra)
    assert torch.equal(_forward(model, c, taps=False)[0], off)
    # no launch is added (profiling mode 1 counts the launches of both passes)
    counts = []
    for keep in (False, True):
        eng.set_profiling(1)
        try:
            _forward(model, c, taps=keep)
            counts.append(_launches(eng))
        finally:
            eng.set_profiling(0)
    assert counts[0] == counts[1] > 100, counts
    assert list(taps)[:3] == ["conv_in", "down_blocks.0.resnets.0", "down_blocks.0.attentions.0"] and tuple(taps["conv_in"].shape) == (3, 64, 16, 16)


def test_taps_under_graph_replay_and_cached_reference(tiny):
    _cfg, _params, model, cases = tiny
    c = cases["uniform_b3_cam_img"]
    plain, taps0, _ = _forward(model, c)
    taps0 = {n: x.cpu() for n, x in taps0.items()}
    for flag in ("use_hip_graph", "cache_reference"):
        setattr(model, flag, True)
        try:
            # (graph: first use, capture, replay; cache: the encoder pass, then two forwards on the cached reference)
            lat, text = c.lat.cuda(), c.text.cuda()

            def run(keep):
                model.keep_taps = keep
                model.fourier_projection = c.cams[2]
                with torch.no_grad():
                    out = model(c.sample.cuda(), c.t.cuda(), text, source_camera=c.cams[0].cuda(), target_camera=c.cams[1].cuda(),
                                source_image_latents=lat).sample.float().cpu()
                return out, ({n: x.cpu() for n, x in model.taps().items()} if keep else None)

            offs = [run(False)[0] for _ in range(3)]
            model.reset_reference_cache()
            ons = [run(True) for _ in range(3)]
            for i in range(3):
                assert torch.equal(ons[i][0], offs[i]), (flag, i)
                assert list(ons[i][1]) == list(taps0), (flag, i)
            # the replayed / cached forwards hold the records of their own run
            for n in taps0:
                assert torch.equal(ons[2][1][n], ons[1][1][n]), (flag, n)
            if flag == "use_hip_graph":
                assert torch.equal(offs[0], plain)
                for n in taps0:
                    assert torch.equal(ons[2][1][n], taps0[n]), (flag, n)
        finally:
            setattr(model, flag, False)
            model.keep_taps = False
            model.fourier_projection = None
            model.reset_reference_cache()


def test_shallow_forward_taps_the_blocks_it_runs(tiny):
    _cfg, _params, model, cases = tiny
    c = cases["uniform_b3_cam_img"]
    model.enable_deepcache(3, 0)
    try:
        lat, text = c.lat.cuda(), c.text.cuda()

        def run(keep, mode):
            model.keep_taps = keep
            model.fourier_projection = c.cams[2]
            with torch.no_grad():
                out = model(c.sample.cuda(), c.t.cuda(), text, source_camera=c.cams[0].cuda(), target_camera=c.cams[1].cuda(),
                            source_image_latents=lat, deep_cache=mode).sample.float().cpu()
            return out, (model.taps() if keep else None)

        full_off, _ = run(False, "refresh")
        shallow_off, _ = run(False, "reuse")
        full_on, full_taps = run(True, "refresh")
        shallow_on, taps = run(True, "reuse")
        assert torch.equal(full_on, full_off) and torch.equal(shallow_on, shallow_off)
        assert len(full_taps) == 1 + 22 + 16 + 6 + 8 + 1
        assert list(taps) == ["conv_in", "down_blocks.0.resnets.0", "down_blocks.0.attentions.0", "up_blocks.3.resnets.1",
                              "up_blocks.3.attentions.1", "up_blocks.3.resnets.2", "up_blocks.3.attentions.2", "film.up_3", "conv_norm_out.in"]
        # the executed blocks of the shallow forward read what the full forward's read up to the stored feature
        for n in ("conv_in", "down_blocks.0.resnets.0", "down_blocks.0.attentions.0"):
            assert torch.equal(taps[n], full_taps[n]), n
    finally:
        model.disable_deepcache()
        model.keep_taps = False
        model.fourier_projection = None
        model.reset_reference_cache()
