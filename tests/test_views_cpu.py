"""CPU-side checks of the shared-reference forward (N14: V views of one object in one batch).

* the C ABI: header, ``_lib.mvd_forward_args_t`` (field ``views``), ``MVD_SHARE_REF`` and the new symbols agree;
* ``mvd_amd.utils.orbit_cameras`` is ``create_camera_matrix`` row by row;
* every shape the mode does not take is rejected on the host, before any launch, with its message (an engine without a
  workspace: nothing could launch);
* on the ORACLE alone: the V independent batch-2 calls differ from both ways of batching them through today's interface (the
  source repeated V or 2V times) by far more than the engine's tolerance -- so the GPU test that holds the shared forward
  to the independent calls (tests/test_views_gpu.py) cannot be passed by either of them.
"""
import ctypes as C
import math
import os
import re

import pytest
import torch

from mvd_amd import _lib as L
from mvd_amd.config import UNetConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_L2 = 2e-2            # tests/test_engine_gpu.py: the engine's bound against the oracle


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.lib()


def _header():
    return open(os.path.join(ROOT, "include", "mvd_hip.h")).read()


# ------------------------------------------------------------------------------------------------ ABI
def test_forward_args_struct_matches_header():
    body = re.search(r"typedef struct \{((?:(?!typedef).)*?)\} mvd_forward_args_t;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names, kinds = [], []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ptr = "*" in decl
        typ = "ptr" if ptr else decl.split()[0]
        for n in decl.replace("*", " ").split(",") if not ptr else [decl]:
            names.append(n.replace("*", " ").split()[-1])
            kinds.append(typ)
    fields = L.mvd_forward_args_t._fields_
    assert names == [f[0] for f in fields]
    assert names[-1] == "views" and fields[-1] == ("views", C.c_int)
    want = {"ptr": C.c_void_p, "int": C.c_int}
    assert [want[k] for k in kinds] == [f[1] for f in fields]


def test_share_ref_flag_and_symbols(lib):
    hdr = _header()
    flags = dict(re.findall(r"\b(MVD_(?:USE_CAMERA|USE_IMAGE|REUSE_REF|KEEP_FEATURES|SHARE_REF)) = (\d+)", hdr))
    assert {k: int(v) for k, v in flags.items()} == dict(MVD_USE_CAMERA=L.MVD_USE_CAMERA, MVD_USE_IMAGE=L.MVD_USE_IMAGE,
                                                         MVD_REUSE_REF=L.MVD_REUSE_REF, MVD_KEEP_FEATURES=L.MVD_KEEP_FEATURES,
                                                         MVD_SHARE_REF=L.MVD_SHARE_REF)
    assert L.MVD_SHARE_REF == 16
    for name in ("mvd_engine_workspace_bytes_args", "mvd_op_attention_grouped"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name)
    # mvd_op_attention's signature plus kv_group in front of the stream
    base, grouped = L._SIGS["mvd_op_attention"], L._SIGS["mvd_op_attention_grouped"]
    assert grouped == (base[0], base[1][:-1] + [C.c_int] + base[1][-1:])


# ------------------------------------------------------------------------------------------------ orbit_cameras
@pytest.mark.parametrize("n,elev,radius,start", [(1, 0.0, 2.0, 0.0), (4, 0.0, 2.0, 0.0), (5, 20.0, 1.5, 30.0), (8, -35.0, 3.0, 350.0)])
def test_orbit_cameras_rows_are_create_camera_matrix(n, elev, radius, start):
    from mvd_amd.utils import create_camera_matrix, orbit_cameras
    cams = orbit_cameras(n, elevation_deg=elev, radius=radius, start_deg=start)
    assert cams.shape == (n, 3, 4) and cams.dtype == torch.float32
    e = math.radians(elev)
    for i in range(n):
        a = math.radians(start + 360.0 * i / n)
        pos = [radius * math.cos(e) * math.sin(a), radius * math.sin(e), radius * math.cos(e) * math.cos(a)]
        assert torch.equal(cams[i], create_camera_matrix(pos, [0, 0, 0])), i
        assert abs(float(cams[i, :, 3].norm()) - radius) < 1e-5
    if elev == 0.0 and start == 0.0:
        assert torch.equal(cams[0], create_camera_matrix([0, 0, radius], [0, 0, 0]))      # infer.py's source position
    import importlib.util
    spec = importlib.util.spec_from_file_location("_shim_utils", os.path.join(ROOT, "integration", "src", "utils.py"))
    shim = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(shim)
    assert shim.orbit_cameras is orbit_cameras


def test_orbit_cameras_defaults_and_bad_count():
    from mvd_amd.utils import orbit_cameras
    assert torch.equal(orbit_cameras(3), orbit_cameras(3, elevation_deg=0.0, radius=2.0, start_deg=0.0))
    with pytest.raises(ValueError):
        orbit_cameras(0)


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


REJECTED = [
    # batch, views, hw, ref_batch, flags, cam_batch, message
    (4, 2, 8, 1, None, 0, "do not divide"),                        # hw % g != 0 at the 1x1 level
    (6, 3, 16, 2, None, 0, "ref_batch == 1"),
    (6, 3, 16, 6, None, 0, "ref_batch == 1"),
    (6, 2, 16, 1, None, 0, "rows per view"),                       # g = 3
    (5, 2, 16, 1, None, 0, "not a multiple of views"),
    (6, 0, 16, 1, None, 0, "not a multiple of views"),
    (6, 3, 16, 1, L.MVD_SHARE_REF, 0, "needs MVD_USE_IMAGE"),
    (6, 3, 16, 1, L.MVD_USE_IMAGE | L.MVD_USE_CAMERA | L.MVD_SHARE_REF, 2, "cameras must hold"),
    (6, 3, 16, 1, L.MVD_USE_IMAGE, 0, "needs MVD_SHARE_REF"),      # views without the flag
]


@pytest.mark.parametrize("batch,views,hw,ref_batch,flags,cam_batch,msg", REJECTED)
def test_shared_forward_rejections_on_the_host(lib, batch, views, hw, ref_batch, flags, cam_batch, msg):
    h = _tiny_engine(lib)
    try:
        a = _args(batch, views, hw, ref_batch, flags, cam_batch)
        assert lib.mvd_unet_forward(h, C.byref(a), None) != 0
        assert msg in L.last_error(), L.last_error()
        assert lib.mvd_engine_workspace_bytes_args(h, C.byref(a)) < 0
        assert msg in L.last_error(), L.last_error()
    finally:
        lib.mvd_engine_destroy(h)


def test_shared_forward_rejected_on_the_global_statistics_path(lib):
    h = _tiny_engine(lib)
    try:
        stats = (C.c_float * 4)()          # never written: the call is refused before it sizes anything
        a = _args(6, 3)
        assert lib.mvd_engine_reference_encode(h, C.byref(a), stats, None) != 0
        assert "global-statistics" in L.last_error(), L.last_error()
    finally:
        lib.mvd_engine_destroy(h)


def test_shared_forward_sizing(lib):
    """The argument-block sizing entry sizes what the positional one cannot express (V = 3 does not divide the reference
    tokens), a valid shared forward gets as far as the missing workspace, and the flag-less block sizes like the positional
    entry."""
    h = _tiny_engine(lib)
    try:
        cam = L.MVD_USE_CAMERA | L.MVD_USE_IMAGE
        assert lib.mvd_engine_workspace_bytes(h, 6, 16, 16, 7, 1) < 0 and "divisible" in L.last_error()
        ws = {}
        for V, g in ((3, 1), (3, 2), (4, 2), (5, 2)):
            ws[V, g] = lib.mvd_engine_workspace_bytes_args(h, C.byref(_args(g * V, V, flags=cam | L.MVD_SHARE_REF, cam_batch=V)))
            assert ws[V, g] > 0, L.last_error()
        assert ws[3, 1] < ws[3, 2] < ws[4, 2] < ws[5, 2]
        # less than the source repeated per row: one encoder pass at batch 1 instead of batch 8
        assert ws[4, 2] < lib.mvd_engine_workspace_bytes(h, 8, 16, 16, 7, 8)
        plain = _args(2, 0, flags=cam, cam_batch=0)
        assert lib.mvd_engine_workspace_bytes_args(h, C.byref(plain)) == lib.mvd_engine_workspace_bytes(h, 2, 16, 16, 7, 1)
        a = _args(6, 3)
        assert lib.mvd_unet_forward(h, C.byref(a), None) != 0
        assert "workspace" in L.last_error(), L.last_error()
    finally:
        lib.mvd_engine_destroy(h)


# ------------------------------------------------------------------------------------------------ separation on the oracle
@pytest.mark.parametrize("V", [3, 5])
def test_wrong_batchings_are_far_from_the_independent_calls(V):
    """V in {3, 5}, g = 2, 16x16 latents, img_ref_scale 1.0.  Under guidance a batch-2 call gives its uncond row the first half
    of the reference tokens and its cond row the second half (Q4); a batch-2V call with a repeated source re-chunks V (or 2V)
    copies over 2V rows instead, and the replicated batch moves the Q2 statistics.  Both must be at least 4 x TOL_L2 = 8e-2
    from the independent calls.  On these inputs (make_inputs' default seed): 8.2e-2 / 2.37e-1 at V = 3, 8.9e-2 / 2.31e-1 at
    V = 5.  The V-times distance moves with the inputs -- 7.7e-2 to 1.3e-1 over seeds 0..5 -- so the bound sits near its low end;
    the 2V-times distance is 2.2e-1 to 2.6e-1 throughout."""
    from tests.views_util import views_case
    c = views_case(V, 2, 16, 1.0, True)
    print(f"V={V}: source repeated V times {c.d_rep_v:.3e}, 2V times {c.d_rep_gv:.3e} from the independent calls", flush=True)
    assert torch.isfinite(c.want).all()
    assert c.d_rep_v >= 4 * TOL_L2, c.d_rep_v
    assert c.d_rep_gv >= 4 * TOL_L2, c.d_rep_gv
