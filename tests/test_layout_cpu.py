"""The batch layout as ONE value (mvd_amd/layout.py, csrc/ragged.h): what the three Python layers and the three C entries used to
work out each for themselves.

* ``ViewLayout.parse`` over a table of inputs: the expected values are written out by hand and are what the denoiser,
  ``MultiViewUNet.forward`` (``who="forward"``) and ``MVDEngine`` (``who="engine"``) computed before they shared the value;
* every layer takes an integral NumPy scalar for a view count (the denoiser used to take it for a sequence);
* the C entries: a bad call through ``mvd_unet_forward_ragged`` with equal counts is rejected with the message -- byte for byte -- of
  ``mvd_unet_forward_objects`` (one object: of ``mvd_unet_forward``), one case per rule that such a call can reach.  The batch rules
  are not among them: the ragged entry checks its counts against the batch, in its own words, before it looks whether they are
  equal (tests/test_ragged_cpu.py pins that).  ``objects`` of 0 / 1 against ``mvd_unet_forward`` is tests/test_objects_cpu.py's."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from mvd_amd import _lib as L
from mvd_amd.config import UNetConfig
from mvd_amd.layout import ViewLayout


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.lib()


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


def _args(batch, views, hw, ref_batch, flags, cam_batch):
    a = L.mvd_forward_args_t()
    a.batch, a.height, a.width, a.text_len, a.ref_batch, a.views = batch, hw, hw, 7, ref_batch, views
    a.cam_rows, a.cam_batch = 4, cam_batch
    a.flags = (L.MVD_USE_IMAGE | L.MVD_SHARE_REF) if flags is None else flags
    return a


def _counts(counts):
    return (C.c_int * len(counts))(*counts)


class _StubUNet:
    """enough of MultiViewUNet for the denoiser to reach its argument checks"""

    def _exec_device(self):
        return torch.device("cpu")


# views, objects, who -> (rows, sources, B, text_rows(B), g(B), kwargs(), key())
PARSED = [
    (None, None, "forward", (0, 0, 8, 8, 1, {}, ())),
    (None, None, "engine", (0, 0, 8, 8, 1, {}, ())),
    (1, None, "forward", (0, 0, 8, 8, 1, {}, ())),                          # one view: the ordinary forward ...
    (1, None, "engine", (1, 1, 2, 2, 2, {"views": 1}, (1,))),               # ... but the engine's shared forward of one view
    (4, None, "forward", (4, 1, 8, 2, 2, {"views": 4}, (4,))),
    (4, 1, "engine", (4, 1, 4, 1, 1, {"views": 4}, (4,))),
    (4, None, "engine", (4, 1, 6, 1, 0, {"views": 4}, (4,))),               # 6 rows are no multiple of 4 views: g = 0
    (np.int64(4), None, "forward", (4, 1, 8, 2, 2, {"views": 4}, (4,))),
    (np.int64(4), np.int64(1), "engine", (4, 1, 8, 2, 2, {"views": 4}, (4,))),
    (2, 3, "forward", (6, 3, 12, 6, 2, {"views": 2, "objects": 3}, (2, 3))),
    (2, 3, "engine", (6, 3, 6, 3, 1, {"views": 2, "objects": 3}, (2, 3))),
    (None, 3, "forward", (3, 3, 6, 6, 2, {"views": 1, "objects": 3}, (1, 3))),  # objects without views: one view each
    ((3, 2, 1), None, "forward", (6, 3, 12, 6, 2, {"views": (3, 2, 1)}, ((3, 2, 1),))),
    ((3, 2, 1), 3, "engine", (6, 3, 6, 3, 1, {"views": (3, 2, 1)}, ((3, 2, 1),))),
    ([2, 2], None, "forward", (4, 2, 4, 2, 1, {"views": (2, 2)}, ((2, 2),))),   # equal counts stay counts: not the (2, 2) of objects
    ([2, 2], None, "engine", (4, 2, 10, 4, 0, {"views": (2, 2)}, ((2, 2),))),
]


@pytest.mark.parametrize("views,objects,who,want", PARSED)
def test_parse(views, objects, who, want):
    lay = ViewLayout.parse(views, objects, who)
    B = want[2]
    got = (lay.rows, lay.sources, B, lay.text_rows(B), lay.g(B), lay.kwargs(), lay.key())
    assert got == want
    assert all(type(v) is int for v in (lay.views, lay.objects) + lay.counts)       # plain ints whatever came in
    assert ViewLayout.parse(**lay.kwargs(), who="engine") == lay                    # the next layer down reads the same layout


PARSE_REJECTED = [
    ((), None, "forward", "views=(): every object needs at least one view"),
    ((), None, "engine", "engine.forward: views=(): every object needs at least one view"),
    ((3, 0), None, "forward", "views=(3, 0): every object needs at least one view"),
    ((3, 0), 2, "engine", "engine.forward: views=(3, 0): every object needs at least one view"),
    ((2, 1), 3, "forward", "views=(2, 1): objects must be None or 2, got 3"),
    ((2, 1), 3, "engine", "engine.forward: views=(2, 1): objects must be None or 2, got 3"),
    (None, 3, "engine", "engine.forward: objects = 3 needs views"),
]


@pytest.mark.parametrize("views,objects,who,msg", PARSE_REJECTED)
def test_parse_rejects(views, objects, who, msg):
    with pytest.raises(L.MvdError) as ei:
        ViewLayout.parse(views, objects, who)
    assert str(ei.value) == msg


def test_record_keys_are_what_they_were():
    from mvd_amd.engine import MVDEngine
    key = MVDEngine._ref_key
    assert key(8, 16, 16, 7, 1, np.int64(4)) == (8, 16, 16, 7, 1, 4)
    assert key(12, 16, 16, 7, 3, 2, np.int32(3)) == (12, 16, 16, 7, 3, 2, 3)
    assert key(12, 16, 16, 7, 3, np.array([3, 2, 1])) == (12, 16, 16, 7, 3, (3, 2, 1))
    assert key(2, 16, 16, 7, 2) == (2, 16, 16, 7, 2)
    # a key is a record, not a call: what a forward would reject still has one (nothing raises)
    assert key(6, 16, 16, 7, 3, 0, 3) == (6, 16, 16, 7, 3, 3)
    assert key(6, 16, 16, 7, 3, (), 0) == (6, 16, 16, 7, 3)
    assert key(6, 16, 16, 7, 3, (2, 1), 3) == (6, 16, 16, 7, 3, (2, 1))


# ------------------------------------------------------------------------------------------------ integer kinds, layer by layer
def test_the_denoiser_takes_a_numpy_integer_for_a_view_count():
    from mvd_amd.pipeline import MVDDenoiser
    from mvd_amd.scheduler import DDIMScheduler
    den = MVDDenoiser(_StubUNet(), DDIMScheduler())
    with pytest.raises(L.MvdError, match="views: one prompt for the one object, got 2 rows"):
        den(torch.zeros(2, 7, 32), 2, 1.0, views=np.int64(4))
    with pytest.raises(L.MvdError, match="objects: one prompt per object, got 3 rows of prompt_embeds for 2 objects"):
        den(torch.zeros(3, 7, 32), 2, 1.0, views=np.int64(4), objects=np.int64(2))


class _StubEngine:
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def forward(self, x, t, text, **kw):
        self.calls.append(kw)
        return torch.zeros_like(x)

    def reference_cache_valid(self, *a, **kw):
        return False


class _StubModel:
    """enough of MultiViewUNet for its forward to reach the engine call"""
    use_camera_conditioning, use_image_conditioning, cache_reference = False, True, False
    reference_stats_group = None
    dtype = torch.float32

    def __init__(self):
        self.eng = _StubEngine()

    def _sync_engine(self):
        return self.eng

    @staticmethod
    def _f32(t, dev):
        return t.float()


@pytest.mark.parametrize("views,objects,B,text_rows,ref_rows,passed", [
    (np.int64(3), None, 6, 2, 1, {"views": 3}),
    (np.int32(2), np.int64(2), 8, 4, 2, {"views": 2, "objects": 2}),
    (np.array([2, 1]), None, 3, 2, 2, {"views": (2, 1)}),
])
def test_the_unet_forward_takes_a_numpy_integer_for_a_view_count(views, objects, B, text_rows, ref_rows, passed):
    from mvd_amd.mvd_unet import MultiViewUNet
    m = _StubModel()
    MultiViewUNet.forward(m, torch.zeros(B, 4, 2, 2), 5, torch.zeros(text_rows, 7, 32), source_image_latents=torch.zeros(ref_rows, 4, 2, 2),
                          views=views, objects=objects)
    (kw,) = m.eng.calls
    assert {k: kw[k] for k in ("views", "objects") if k in kw} == passed
    assert kw["encoder_text"].shape[0] == ref_rows


# ------------------------------------------------------------------------------------------------ C entries: one message per rule
CAM = L.MVD_USE_IMAGE | L.MVD_USE_CAMERA | L.MVD_SHARE_REF
EQUAL_COUNTS_REJECTED = [
    # equal counts, batch, hw, ref_batch, flags, cam_batch, message -- the rules a call that passed the counts' own checks can break
    ((2, 2), 8, 16, 2, L.MVD_USE_IMAGE, 0, "forward: views = 2 needs MVD_SHARE_REF"),      # (views > 1 in the block: every entry's words)
    ((2, 2), 8, 16, 2, L.MVD_SHARE_REF, 0, "forward_objects: objects = 2 needs MVD_SHARE_REF with MVD_USE_IMAGE"),
    ((2, 2), 8, 16, 1, None, 0, "forward_objects: needs ref_batch == objects = 2"),
    ((2, 2), 8, 16, 2, CAM, 2, "forward_objects: the cameras must hold 1 or objects x views = 4 rows, got 2"),
    ((2, 2), 8, 8, 2, None, 0, "forward_objects: the 1 reference tokens of level"),
    # one object: the shared forward
    ((3,), 6, 16, 1, L.MVD_USE_IMAGE, 0, "forward: views = 3 needs MVD_SHARE_REF"),
    ((3,), 6, 16, 1, L.MVD_SHARE_REF, 0, "forward: MVD_SHARE_REF needs MVD_USE_IMAGE"),
    ((3,), 6, 16, 2, None, 0, "forward: MVD_SHARE_REF needs ref_batch == 1 (one object), got 2"),
    ((3,), 6, 16, 1, CAM, 2, "forward: MVD_SHARE_REF: the cameras must hold 1 or views = 3 rows, got 2"),
    ((2,), 4, 8, 1, None, 0, "forward: MVD_SHARE_REF: the 1 reference tokens of level"),
]


@pytest.mark.parametrize("counts,batch,hw,ref_batch,flags,cam_batch,msg", EQUAL_COUNTS_REJECTED)
def test_equal_counts_reject_like_the_uniform_entry(lib, counts, batch, hw, ref_batch, flags, cam_batch, msg):
    h = _tiny_engine(lib)
    try:
        O = len(counts)
        a = _args(batch, counts[0], hw, ref_batch, flags, cam_batch)         # the uniform entry's call: views in the block
        r = _args(batch, 0, hw, ref_batch, flags, cam_batch)                 # the ragged entry's: counts beside it
        rc = lib.mvd_unet_forward_objects(h, C.byref(a), O, None)
        want = L.last_error()
        assert rc != 0 and msg in want, want
        assert lib.mvd_unet_forward_ragged(h, C.byref(r), _counts(counts), O, None) == rc
        assert L.last_error() == want
        ws = lib.mvd_engine_workspace_bytes_objects(h, C.byref(a), O)
        assert ws < 0 and L.last_error() == want
        assert lib.mvd_engine_workspace_bytes_ragged(h, C.byref(r), _counts(counts), O) == ws
        assert L.last_error() == want
        if O == 1:
            assert lib.mvd_unet_forward(h, C.byref(a), None) == rc and L.last_error() == want
    finally:
        lib.mvd_engine_destroy(h)
