"""CPU-side checks of the object forward (N15: O objects x V views in one forward).

* the C ABI: header, ``_lib._SIGS`` and ``EXPORTED_SYMBOLS`` agree on the four new symbols; ``mvd_forward_args_t`` still ends
  in ``views`` (the object count travels beside the block);
* every shape ``mvd_unet_forward_objects`` does not take is rejected on the host, before any launch, with its message (an
  engine without a workspace: nothing could launch); ``objects`` of 0 or 1 is ``mvd_unet_forward``, rejections included;
* on the ORACLE alone: the O V independent calls differ from the ordinary batch with repeated sources and from the
  object-swapped result by far more than the engine's tolerance -- so the GPU test that holds the object forward to the
  independent calls (tests/test_objects_gpu.py) cannot be passed by any of them;
* the bit-exact attention test's data can see a wrong K/V element map.
"""
import ctypes as C
import os
import re

import pytest
import torch

from mvd_amd import _lib as L
from mvd_amd.config import UNetConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_L2 = 2e-2            # tests/test_engine_gpu.py: the engine's bound against the oracle
NEW = ("mvd_unet_forward_objects", "mvd_engine_workspace_bytes_objects", "mvd_op_attention_objects", "mvd_op_refnorm_grouped")


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
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in L.EXPORTED_SYMBOLS and name in L._SIGS and hasattr(lib, name), name
    S = L._SIGS
    # each new entry is its N14 counterpart plus the count, in front of the stream where there is one
    fwd, fwd_o = S["mvd_unet_forward"], S["mvd_unet_forward_objects"]
    assert fwd_o == (fwd[0], fwd[1][:-1] + [C.c_int] + fwd[1][-1:])
    ws, ws_o = S["mvd_engine_workspace_bytes_args"], S["mvd_engine_workspace_bytes_objects"]
    assert ws_o == (ws[0], ws[1] + [C.c_int])
    grp, obj = S["mvd_op_attention_grouped"], S["mvd_op_attention_objects"]
    assert obj == (grp[0], grp[1][:-1] + [C.c_int] + grp[1][-1:])
    rn, rng = S["mvd_op_refnorm"], S["mvd_op_refnorm_grouped"]
    assert rng == (rn[0], rn[1][:2] + [C.c_int] + rn[1][2:])          # (x, batch, GROUP, hw, c, y, stream)
    # and the header's parameter lists have as many parameters
    for name in NEW:
        params = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr, re.S).group(1)
        assert len(params.split(",")) == len(S[name][1]), (name, params)


def test_forward_args_struct_still_ends_in_views():
    body = re.search(r"typedef struct \{((?:(?!typedef).)*?)\} mvd_forward_args_t;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    last = [d.strip() for d in body.split(";") if d.strip()][-1]
    assert last == "int views", last
    assert L.mvd_forward_args_t._fields_[-1] == ("views", C.c_int)
    assert "objects" not in [f[0] for f in L.mvd_forward_args_t._fields_]


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


def _args(batch, views, hw=16, ref_batch=1, flags=None, cam_batch=0):
    a = L.mvd_forward_args_t()
    a.batch, a.height, a.width, a.text_len, a.ref_batch, a.views = batch, hw, hw, 7, ref_batch, views
    a.cam_rows, a.cam_batch = 4, cam_batch
    a.flags = (L.MVD_USE_IMAGE | L.MVD_SHARE_REF) if flags is None else flags
    return a


CAM = L.MVD_USE_IMAGE | L.MVD_USE_CAMERA | L.MVD_SHARE_REF
OBJECTS_REJECTED = [
    # objects, batch, views, hw, ref_batch, flags, cam_batch, message -- one per rule of include/mvd_hip.h
    (2, 8, 0, 16, 2, L.MVD_USE_IMAGE, 0, "needs MVD_SHARE_REF with MVD_USE_IMAGE"),        # objects without the flag
    (2, 8, 2, 16, 2, L.MVD_SHARE_REF, 0, "needs MVD_SHARE_REF with MVD_USE_IMAGE"),        # ... without image conditioning
    (2, 8, 2, 16, 1, None, 0, "ref_batch == objects"),                                     # one reference row for two objects
    (2, 8, 2, 16, 4, None, 0, "ref_batch == objects"),                                     # one per (object, view)
    (2, 10, 2, 16, 2, None, 0, "not a multiple of objects 2 x views 2"),
    (3, 8, 2, 16, 3, None, 0, "not a multiple of objects 3 x views 2"),
    (2, 8, 0, 16, 2, None, 0, "not a multiple of objects"),                                # views missing
    (2, 12, 2, 16, 2, None, 0, "rows per view"),                                           # g = 3
    (2, 8, 2, 16, 2, CAM, 2, "cameras must hold 1 or objects x views = 4"),                # one camera per object
    (2, 8, 2, 16, 2, CAM, 8, "cameras must hold 1 or objects x views = 4"),                # one per row
    (2, 8, 2, 8, 2, None, 0, "do not divide"),                                             # hw % g != 0 at the 1x1 level
]


@pytest.mark.parametrize("objects,batch,views,hw,ref_batch,flags,cam_batch,msg", OBJECTS_REJECTED)
def test_object_forward_rejections_on_the_host(lib, objects, batch, views, hw, ref_batch, flags, cam_batch, msg):
    h = _tiny_engine(lib)
    try:
        a = _args(batch, views, hw, ref_batch, flags, cam_batch)
        assert lib.mvd_unet_forward_objects(h, C.byref(a), objects, None) != 0
        assert msg in L.last_error(), L.last_error()
        assert lib.mvd_engine_workspace_bytes_objects(h, C.byref(a), objects) < 0
        assert msg in L.last_error(), L.last_error()
    finally:
        lib.mvd_engine_destroy(h)


def test_object_count_does_not_open_the_global_statistics_path(lib):
    """the flag on mvd_engine_reference_encode stays rejected (the entry takes no object count)"""
    h = _tiny_engine(lib)
    try:
        stats = (C.c_float * 4)()          # never written: the call is refused before it sizes anything
        a = _args(8, 2, ref_batch=2)
        assert lib.mvd_engine_reference_encode(h, C.byref(a), stats, None) != 0
        assert "global-statistics" in L.last_error(), L.last_error()
    finally:
        lib.mvd_engine_destroy(h)


# test_views_cpu.REJECTED, rebuilt here (batch, views, hw, ref_batch, flags, cam_batch, message)
VIEWS_REJECTED = [
    (4, 2, 8, 1, None, 0, "do not divide"),
    (6, 3, 16, 2, None, 0, "ref_batch == 1"),
    (6, 3, 16, 6, None, 0, "ref_batch == 1"),
    (6, 2, 16, 1, None, 0, "rows per view"),
    (5, 2, 16, 1, None, 0, "not a multiple of views"),
    (6, 0, 16, 1, None, 0, "not a multiple of views"),
    (6, 3, 16, 1, L.MVD_SHARE_REF, 0, "needs MVD_USE_IMAGE"),
    (6, 3, 16, 1, L.MVD_USE_IMAGE | L.MVD_USE_CAMERA | L.MVD_SHARE_REF, 2, "cameras must hold"),
    (6, 3, 16, 1, L.MVD_USE_IMAGE, 0, "needs MVD_SHARE_REF"),
]


@pytest.mark.parametrize("objects", [0, 1])
@pytest.mark.parametrize("batch,views,hw,ref_batch,flags,cam_batch,msg", VIEWS_REJECTED)
def test_objects_of_zero_or_one_reject_like_the_shared_forward(lib, objects, batch, views, hw, ref_batch, flags, cam_batch, msg):
    h = _tiny_engine(lib)
    try:
        a = _args(batch, views, hw, ref_batch, flags, cam_batch)
        rc = lib.mvd_unet_forward(h, C.byref(a), None)
        want = L.last_error()
        assert rc != 0 and msg in want, want
        assert lib.mvd_unet_forward_objects(h, C.byref(a), objects, None) == rc
        assert L.last_error() == want
        ws = lib.mvd_engine_workspace_bytes_args(h, C.byref(a))
        assert ws < 0 and lib.mvd_engine_workspace_bytes_objects(h, C.byref(a), objects) == ws
        assert L.last_error() == want
    finally:
        lib.mvd_engine_destroy(h)


def test_object_forward_sizing(lib):
    h = _tiny_engine(lib)
    try:
        # objects <= 1: the argument-block entry, for a shared forward and for a plain one
        for a in (_args(8, 4, flags=CAM, cam_batch=4), _args(2, 0, flags=L.MVD_USE_CAMERA | L.MVD_USE_IMAGE)):
            for objects in (0, 1):
                assert lib.mvd_engine_workspace_bytes_objects(h, C.byref(a), objects) == lib.mvd_engine_workspace_bytes_args(h, C.byref(a)) > 0
        ws = {}
        for O, V, g in ((2, 2, 1), (2, 2, 2), (3, 2, 2), (2, 3, 2)):
            ws[O, V, g] = lib.mvd_engine_workspace_bytes_objects(h, C.byref(_args(g * O * V, V, ref_batch=O, flags=CAM, cam_batch=O * V)), O)
            assert ws[O, V, g] > 0, L.last_error()
        assert ws[2, 2, 1] < ws[2, 2, 2] < ws[3, 2, 2]
        # less than the sources repeated per row: the encoder pass at batch 3 instead of batch 12
        assert ws[3, 2, 2] < lib.mvd_engine_workspace_bytes(h, 12, 16, 16, 7, 12)
        # a valid object forward gets as far as the missing workspace
        a = _args(12, 3, ref_batch=2)
        assert lib.mvd_unet_forward_objects(h, C.byref(a), 2, None) != 0
        assert "workspace" in L.last_error(), L.last_error()
    finally:
        lib.mvd_engine_destroy(h)


# ------------------------------------------------------------------------------------------------ separation on the oracle
def test_coupled_statistics_are_far_from_the_independent_calls():
    """(O, V, g) = (3, 2, 1), objects 1 and 2 with sources 8 x as large, img_ref_scale 1.0: no guidance, so Q4 is out of the
    picture and what separates the ordinary batch (every row with its own object's source) from the independent calls is the
    Q2 statistics over the batch alone.  At least 2 x TOL_L2 = 4e-2."""
    from tests.objects_util import objects_case
    c = objects_case(3, 2, 1, 16, 1.0, 8.0, True)
    print(f"(3, 2, 1) amp 8: ordinary batch {c.d_rep_v:.3e}, swapped objects {c.d_swapped:.3e} from the independent calls", flush=True)
    assert torch.isfinite(c.want).all()
    assert torch.equal(c.rep_v, c.rep_gv)                  # g = 1: one and the same batch
    assert c.d_rep_v >= 2 * TOL_L2, c.d_rep_v


def test_wrong_batchings_are_far_from_the_independent_calls():
    """(O, V, g) = (2, 3, 2), sources as drawn, img_ref_scale 1.0: under guidance Q4 hands the rows of an ordinary batch other
    objects' tokens.  Both repeated batches and the object-swapped result are at least 4 x TOL_L2 = 8e-2 from the independent
    calls."""
    from tests.objects_util import objects_case
    c = objects_case(2, 3, 2, 16, 1.0, 1.0, True)
    print(f"(2, 3, 2): sources repeated O V times {c.d_rep_v:.3e}, g O V times {c.d_rep_gv:.3e}, swapped objects {c.d_swapped:.3e} "
          "from the independent calls", flush=True)
    assert torch.isfinite(c.want).all()
    assert c.d_rep_v >= 4 * TOL_L2, c.d_rep_v
    assert c.d_rep_gv >= 4 * TOL_L2, c.d_rep_gv
    assert c.d_swapped >= 4 * TOL_L2, c.d_swapped


# ------------------------------------------------------------------------------------------------ the attention test's data
def test_routing_data_sees_a_wrong_element_map():
    """O = 2, g = 2: the identity map (K/V element q = b // V) and the correct map (q % O) * g + q // O pick different elements
    for q = 1 and 2, and those elements' V rows differ -- a kernel that ignores kv_objects returns other bits."""
    import exact_util as X
    from tests.objects_util import element_of, object_views
    O, V, g, heads, nq, nk = 2, 3, 2, 2, 33, 65
    maps = [element_of(q, O, g) for q in range(O * g)]
    assert maps == [0, 2, 1, 3] and sorted(maps) == list(range(O * g))
    p = X.routing_problem(O * g, heads, V * nq, nk, X.LAZY, True)
    q, k, v, want = object_views(p, O, V, g)
    assert q.shape == (g * O * V, nq, heads * 64) and k.shape[0] == O * g
    for qq in (1, 2):
        assert not torch.equal(p.v[qq], p.v[maps[qq]])
        # rows of group qq (batch rows qq V .. qq V + V - 1) want element maps[qq]'s values at their own keys ...
        b = qq * V
        e = maps[qq]
        pi = p.pi[e].reshape(heads, V, nq)[:, 0]                                      # (heads, nq): view 0 of element e
        vals = p.v[e].reshape(nk, heads, 64)
        right = torch.stack([vals[pi[h], h] for h in range(heads)], 1).reshape(nq, heads * 64)
        assert torch.equal(right, want[b])
        # ... and the identity map's element gives other bits at the same keys
        other = p.v[qq].reshape(nk, heads, 64)
        wrong = torch.stack([other[pi[h], h] for h in range(heads)], 1).reshape(nq, heads * 64)
        assert not torch.equal(wrong, want[b])
