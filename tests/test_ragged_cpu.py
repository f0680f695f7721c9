"""CPU-side checks of the ragged forward (N16: O objects with V_o views each in one forward).

* the C ABI: header, ``_lib._SIGS`` and the library agree on the new symbols; ``mvd_forward_args_t`` is as it was;
* the engine's table builder against the maps of tests/ragged_util.py; equal counts give the N15 arithmetic map;
* every shape ``mvd_unet_forward_ragged`` does not take is rejected on the host, before any launch, with its message (an engine
  without a workspace: nothing could launch), and so are the Python-side arguments that need no GPU;
* on the ORACLE alone: the repeated-source batch and the uniform map forced onto a ragged batch stay away from the R independent
  calls by at least half of what was measured when the feature was written -- the yardstick tests/test_ragged_gpu.py leans on;
* the bit-exact attention test's data can see a wrong table.
"""
import ctypes as C
import os
import re

import pytest
import torch

from mvd_amd import _lib as L
from mvd_amd.config import UNetConfig
from tests.ragged_util import adapter_table, object_of, offsets, ragged_case, ragged_views, row, text_table, uniform_object_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mvd_unet_forward_ragged", "mvd_engine_workspace_bytes_ragged", "mvd_op_attention_mapped")
LAYOUTS = [(3, 1), (1, 3), (3, 2, 1), (1, 1, 4), (2, 2), (3, 3, 3), (4,), (1,), (5, 1, 1, 2)]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.lib()


def _header():
    return open(os.path.join(ROOT, "include", "mvd_hip.h")).read()


# ------------------------------------------------------------------------------------------------ ABI
def test_new_symbols_in_header_sigs_and_library(lib):
    hdr = _header()
    S = L._SIGS
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in L.EXPORTED_SYMBOLS and name in S and hasattr(lib, name), name
        params = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr, re.S).group(1)
        assert len(params.split(",")) == len(S[name][1]), (name, params)
    # the counts and their number come beside the unchanged argument block, in front of the stream where there is one
    fwd, fwd_r = S["mvd_unet_forward"], S["mvd_unet_forward_ragged"]
    assert fwd_r == (fwd[0], fwd[1][:-1] + [C.POINTER(C.c_int), C.c_int] + fwd[1][-1:])
    ws, ws_r = S["mvd_engine_workspace_bytes_args"], S["mvd_engine_workspace_bytes_ragged"]
    assert ws_r == (ws[0], ws[1] + [C.POINTER(C.c_int), C.c_int])
    att, mapped = S["mvd_op_attention"], S["mvd_op_attention_mapped"]
    assert mapped == (att[0], att[1][:-1] + [C.POINTER(C.c_int), C.c_int] + att[1][-1:])
    assert L.mvd_forward_args_t._fields_[-1] == ("views", C.c_int)


# ------------------------------------------------------------------------------------------------ the tables
def _engine_tables(lib, counts, g):
    n = g * sum(counts)
    a, t = (C.c_int * n)(), (C.c_int * n)()
    assert lib.mvd_debug_ragged_tables((C.c_int * len(counts))(*counts), len(counts), g, a, t) == n, L.last_error()
    return list(a), list(t)


@pytest.mark.parametrize("g", [1, 2])
@pytest.mark.parametrize("counts", LAYOUTS)
def test_engine_tables_are_the_row_maps(lib, counts, g):
    a, t = _engine_tables(lib, counts, g)
    O = len(counts)
    _, R = offsets(counts)
    assert a == adapter_table(counts, g) and t == text_table(counts, g)
    assert all(0 <= x < g * O for x in a + t)
    for j in range(g):
        for o, V in enumerate(counts):
            for v in range(V):
                r = row(counts, j, o, v)
                assert a[r] == o * g + j and t[r] == j * O + o
    if len(set(counts)) == 1:                      # equal counts: the arithmetic map of MvdAttnArgs::kv_objects, the text in batch order
        from tests.objects_util import element_of
        V = counts[0]
        assert a == [element_of(r // V, O, g) for r in range(g * R)]
        assert t == [r // V for r in range(g * R)]


def test_a_ragged_layout_is_not_the_uniform_map():
    assert object_of((3, 2, 1)) == [0, 0, 0, 1, 1, 2] and uniform_object_of((3, 2, 1)) == [0, 0, 1, 1, 2, 2]
    assert object_of((3, 1)) == [0, 0, 0, 1] and uniform_object_of((3, 1)) == [0, 0, 1, 1]


@pytest.mark.parametrize("counts,g", [((3, 0), 1), ((0,), 1), ((2, -1, 2), 2), ((2, 2), 3), ((2, 2), 0), ((), 1)])
def test_table_builder_rejects(lib, counts, g):
    n = 64
    a, t = (C.c_int * n)(), (C.c_int * n)()
    assert lib.mvd_debug_ragged_tables((C.c_int * max(len(counts), 1))(*counts), len(counts), g, a, t) < 0
    assert L.last_error()


# ------------------------------------------------------------------------------------------------ host-side rejections
def _tiny_engine(lib):
    cfg = UNetConfig.tiny()
    c = L.mvd_config_t()
    c.in_channels, c.out_channels, c.num_levels = cfg.in_channels, cfg.out_channels, cfg.num_levels
    for i in range(cfg.num_levels):
        c.block_out_channels[i] = cfg.block_out_channels[i]
        c.num_heads[i] = cfg.num_heads[i]
    c.layers_per_block, c.cross_attention_dim = cfg.layers_per_block, cfg.cross_attention_dim
    c.norm_num_groups, c.norm_eps = cfg.norm_num_groups, cfg.norm_eps
    c.cam_output_dim, c.cam_hidden_dim, c.simple_cam_encoder, c.cam_modulation_strength = 96, 48, 0, 0.2
    h = C.c_void_p()
    assert lib.mvd_engine_create(C.byref(c), C.byref(h)) == 0, L.last_error()
    return h


def _args(batch, views=0, hw=16, ref_batch=1, flags=None, cam_batch=0):
    a = L.mvd_forward_args_t()
    a.batch, a.height, a.width, a.text_len, a.ref_batch, a.views = batch, hw, hw, 7, ref_batch, views
    a.cam_rows, a.cam_batch = 4, cam_batch
    a.flags = (L.MVD_USE_IMAGE | L.MVD_SHARE_REF) if flags is None else flags
    return a


def _counts(counts):
    return (C.c_int * max(len(counts), 1))(*counts)


CAM = L.MVD_USE_IMAGE | L.MVD_USE_CAMERA | L.MVD_SHARE_REF
RAGGED_REJECTED = [
    # counts, batch, args.views, hw, ref_batch, flags, cam_batch, message -- one per rule of include/mvd_hip.h
    ((3, 1), 4, 0, 16, 2, L.MVD_USE_IMAGE, 0, "need MVD_SHARE_REF with MVD_USE_IMAGE"),      # counts without the flag
    ((3, 1), 4, 0, 16, 2, L.MVD_SHARE_REF, 0, "need MVD_SHARE_REF with MVD_USE_IMAGE"),      # ... without image conditioning
    ((3, 1), 4, 0, 16, 1, None, 0, "ref_batch == objects"),                                  # one reference row for two objects
    ((3, 1), 4, 0, 16, 4, None, 0, "ref_batch == objects"),                                  # one per view
    ((3, 0), 3, 0, 16, 2, None, 0, "at least one view"),
    ((3, -1), 2, 0, 16, 2, None, 0, "at least one view"),
    ((3, 1), 5, 0, 16, 2, None, 0, "is not 1 or 2"),                                         # not a multiple of R
    ((3, 1), 12, 0, 16, 2, None, 0, "is not 1 or 2"),                                        # g = 3
    ((3, 1), 8, 2, 16, 2, None, 0, "args->views must be 0"),
    ((3, 1), 8, 0, 16, 2, CAM, 2, "cameras must hold 1 or sum of the view counts = 4"),      # one camera per object
    ((3, 1), 8, 0, 16, 2, CAM, 8, "cameras must hold 1 or sum of the view counts = 4"),      # one per row
    ((3, 1), 8, 0, 8, 2, None, 0, "do not divide"),                                          # hw % g != 0 at the 1x1 level
]


@pytest.mark.parametrize("counts,batch,views,hw,ref_batch,flags,cam_batch,msg", RAGGED_REJECTED)
def test_ragged_forward_rejections_on_the_host(lib, counts, batch, views, hw, ref_batch, flags, cam_batch, msg):
    h = _tiny_engine(lib)
    try:
        a = _args(batch, views, hw, ref_batch, flags, cam_batch)
        assert lib.mvd_unet_forward_ragged(h, C.byref(a), _counts(counts), len(counts), None) != 0
        assert msg in L.last_error(), L.last_error()
        assert lib.mvd_engine_workspace_bytes_ragged(h, C.byref(a), _counts(counts), len(counts)) < 0
        assert msg in L.last_error(), L.last_error()
    finally:
        lib.mvd_engine_destroy(h)


def test_null_counts_and_no_objects_are_rejected(lib):
    h = _tiny_engine(lib)
    try:
        a = _args(4, ref_batch=2)
        assert lib.mvd_unet_forward_ragged(h, C.byref(a), None, 2, None) != 0 and "null" in L.last_error()
        assert lib.mvd_unet_forward_ragged(h, C.byref(a), _counts((3, 1)), 0, None) != 0 and "0 objects" in L.last_error()
        assert lib.mvd_engine_workspace_bytes_ragged(h, C.byref(a), None, 2) < 0
    finally:
        lib.mvd_engine_destroy(h)


def test_view_counts_do_not_open_the_global_statistics_path(lib):
    """the flag on mvd_engine_reference_encode stays rejected (the entry takes no counts)"""
    h = _tiny_engine(lib)
    try:
        stats = (C.c_float * 4)()          # never written: the call is refused before it sizes anything
        a = _args(8, 0, ref_batch=2)
        assert lib.mvd_engine_reference_encode(h, C.byref(a), stats, None) != 0
        assert "global-statistics" in L.last_error(), L.last_error()
    finally:
        lib.mvd_engine_destroy(h)


def test_ragged_forward_sizing(lib):
    h = _tiny_engine(lib)
    try:
        def ragged(counts, g):
            R = sum(counts)
            return lib.mvd_engine_workspace_bytes_ragged(h, C.byref(_args(g * R, 0, ref_batch=len(counts), flags=CAM, cam_batch=R)),
                                                         _counts(counts), len(counts))

        def objects(O, V, g):
            return lib.mvd_engine_workspace_bytes_objects(h, C.byref(_args(g * O * V, V, ref_batch=O, flags=CAM, cam_batch=O * V)), O)

        # equal counts ARE the objects forward (one object: the views forward)
        assert ragged((2, 2), 2) == objects(2, 2, 2) > 0
        assert ragged((3, 3, 3), 1) == objects(3, 3, 1) > 0
        assert ragged((4,), 2) == lib.mvd_engine_workspace_bytes_args(h, C.byref(_args(8, 4, flags=CAM, cam_batch=4))) > 0
        # a ragged layout: more than the same objects with fewer rows, less than the layout padded to V = 3
        ws = ragged((3, 2, 1), 2)
        assert ws > 0, L.last_error()
        assert objects(3, 1, 2) < ws < objects(3, 3, 2)
        assert ragged((3, 2, 1), 1) < ws
        # a valid ragged forward gets as far as the missing workspace: no table is built for a call that cannot run
        a = _args(12, 0, ref_batch=3)
        assert lib.mvd_unet_forward_ragged(h, C.byref(a), _counts((3, 2, 1)), 3, None) != 0
        assert "workspace" in L.last_error(), L.last_error()
    finally:
        lib.mvd_engine_destroy(h)


# ------------------------------------------------------------------------------------------------ Python, no GPU
def test_reference_cache_key_carries_the_counts():
    from mvd_amd.engine import MVDEngine
    key = MVDEngine._ref_key
    assert key(12, 16, 16, 7, 3, (3, 2, 1)) == key(12, 16, 16, 7, 3, [3, 2, 1])
    assert key(12, 16, 16, 7, 3, (3, 2, 1)) != key(12, 16, 16, 7, 3, (1, 2, 3))
    assert key(12, 16, 16, 7, 3, (2, 2, 2)) != key(12, 16, 16, 7, 3, 2, 3)          # a ragged call's record is not the objects call's
    # the int forms are what they were
    assert key(8, 16, 16, 7, 1, 4) == (8, 16, 16, 7, 1, 4)
    assert key(8, 16, 16, 7, 2, 2, 2) == (8, 16, 16, 7, 2, 2, 2)
    assert key(2, 16, 16, 7, 2) == key(2, 16, 16, 7, 2, 0, 0) == key(2, 16, 16, 7, 2, 0, 1) == (2, 16, 16, 7, 2)


class _StubUNet:
    """enough of MultiViewUNet for generate_views_batch to reach its argument checks"""
    use_camera_conditioning = use_image_conditioning = True
    img_ref_scale = 0.3

    class config:
        sample_size = 2

    def _exec_device(self):
        return torch.device("cpu")


def _stub_pipeline():
    from mvd_amd.pipeline import MVDPipeline
    from mvd_amd.scheduler import DDIMScheduler
    return MVDPipeline(_StubUNet(), DDIMScheduler())


def _cam(n):
    return torch.eye(4).repeat(n, 1, 1)


RAGGED_PIPELINE_REJECTED = [
    # target camera list, source cameras, latents rows, source latents rows, message
    ([_cam(2)], _cam(2), 2, 2, "target_cameras for 1 objects, prompts for 2"),
    ([_cam(2), _cam(0)], _cam(2), 2, 2, "one (V_o, 3|4, 4) tensor per object"),
    ([_cam(2), torch.eye(4)], _cam(2), 3, 2, "one (V_o, 3|4, 4) tensor per object"),
    ([_cam(2), _cam(1)[:, :3]], _cam(2), 3, 2, "one (V_o, 3|4, 4) tensor per object"),
    ([_cam(2), _cam(1)], _cam(3), 3, 2, "source_cameras must be (2, 4, 4)"),
    ([_cam(2), _cam(1)], _cam(2), 4, 2, "4 rows of latents for the 3 views of counts (2, 1)"),
    ([_cam(2), _cam(1)], _cam(2), 3, 3, "one source image per object"),
]


@pytest.mark.parametrize("cams,src,lat_rows,ref_rows,msg", RAGGED_PIPELINE_REJECTED)
def test_generate_views_batch_rejects_a_bad_ragged_call(cams, src, lat_rows, ref_rows, msg):
    pipe = _stub_pipeline()
    with pytest.raises(L.MvdError) as ei:
        pipe.generate_views_batch(prompt_embeds=torch.zeros(2, 7, 32), source_cameras=src, target_cameras=cams, height=16, width=16,
                                  latents=torch.zeros(lat_rows, 4, 2, 2), source_image_latents=torch.zeros(ref_rows, 4, 2, 2),
                                  output_type="latent", guidance_scale=1.0)
    assert msg in str(ei.value), ei.value


def test_denoiser_rejects_counts_against_objects_or_prompts():
    from mvd_amd.pipeline import MVDDenoiser
    from mvd_amd.scheduler import DDIMScheduler
    den = MVDDenoiser(_StubUNet(), DDIMScheduler())
    with pytest.raises(L.MvdError, match="objects must be None or 2"):
        den(torch.zeros(2, 7, 32), 2, 1.0, views=(2, 1), objects=3)
    with pytest.raises(L.MvdError, match="one prompt per object"):
        den(torch.zeros(3, 7, 32), 2, 1.0, views=(2, 1))


# ------------------------------------------------------------------------------------------------ separation on the oracle
def test_wrong_results_stay_away_at_3_2_1_under_guidance():
    """counts (3, 2, 1), g = 2, sources as drawn, img_ref_scale 1.0 (tiny topology, 16x16).  Measured when the feature was written:
    the repeated-source batch 2.83e-1 from the R independent calls; the uniform kv_group = 2 map forced onto the batch books
    views 2 and 4 to the next object's reference: 1.61e-1 and 1.23e-1 over their rows, 8.2e-2 over the batch.  Held at half."""
    c = ragged_case((3, 2, 1), 2, 16, 1.0, 1.0, True)
    print(f"(3, 2, 1) g 2: repeated sources {c.d_rep:.3e}, uniform map {c.d_uniform:.3e}, misrouted views {c.misrouted} "
          f"{['%.3e' % d for d in c.d_misrouted]}", flush=True)
    assert torch.isfinite(c.want).all()
    assert c.misrouted == [2, 4]
    assert c.d_misrouted[0] >= 6e-2 and c.d_misrouted[1] >= 5e-2, c.d_misrouted
    assert c.d_rep >= 1.4e-1, c.d_rep
    assert c.d_uniform >= 4e-2, c.d_uniform


def test_wrong_results_stay_away_at_3_1_under_guidance():
    """counts (3, 1), g = 2: the misrouted view 1.58e-1, the repeated-source batch 1.97e-1 (measured); held at half"""
    c = ragged_case((3, 1), 2, 16, 1.0, 1.0, True)
    print(f"(3, 1) g 2: repeated sources {c.d_rep:.3e}, uniform map {c.d_uniform:.3e}, misrouted {['%.3e' % d for d in c.d_misrouted]}", flush=True)
    assert c.misrouted == [2]
    assert c.d_misrouted[0] >= 8e-2 and c.d_rep >= 1e-1, (c.d_misrouted, c.d_rep)


def test_wrong_results_stay_away_at_3_2_1_without_guidance():
    """counts (3, 2, 1), g = 1, the sources of objects 1.. scaled by 8: views 2 and 4 at 2.43e-1 and 1.02e-1, the repeated-source
    batch (coupled statistics alone) 6.1e-2 (measured); held at half"""
    c = ragged_case((3, 2, 1), 1, 16, 1.0, 8.0, True)
    print(f"(3, 2, 1) g 1 amp 8: repeated sources {c.d_rep:.3e}, misrouted {['%.3e' % d for d in c.d_misrouted]}", flush=True)
    assert c.d_misrouted[0] >= 1.2e-1 and c.d_misrouted[1] >= 5e-2 and c.d_rep >= 3e-2, (c.d_misrouted, c.d_rep)


# ------------------------------------------------------------------------------------------------ the attention test's data
def test_routing_data_sees_a_wrong_table():
    """counts (3, 2, 1), g = 2: batch row 2 (object 0, view 2) wants element 0's values; the uniform map would read element 2
    (object 1), whose V rows differ at the same keys"""
    import exact_util as X
    counts, g, heads, nq, nk = (3, 2, 1), 2, 2, 33, 65
    p = X.routing_problem(len(counts) * g, heads, max(counts) * nq, nk, X.LAZY, True)
    q, k, v, want = ragged_views(p, counts, g, nq)
    R = sum(counts)
    assert q.shape == (g * R, nq, heads * 64) and k.shape[0] == len(counts) * g
    tab = adapter_table(counts, g)
    b, e, wrong_e = 2, tab[2], 1 * g + 0
    assert e == 0 and not torch.equal(p.v[e], p.v[wrong_e])
    pi = p.pi[e].reshape(heads, max(counts), nq)[:, 2]                                # (heads, nq): view 2 of element e
    for elem, same in ((e, True), (wrong_e, False)):
        vals = p.v[elem].reshape(nk, heads, 64)
        rows = torch.stack([vals[pi[h], h] for h in range(heads)], 1).reshape(nq, heads * 64)
        assert torch.equal(rows, want[b]) == same
