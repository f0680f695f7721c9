"""The contract every handle module shares (csrc/host_util.h ModuleBase, mvd_amd/_lib.py Handle), once for all six families,
on the host: ``set_weight`` and ``bind_workspace`` validate their arguments before they store anything, ``destroy(NULL)`` is
harmless.  No GPU: the pointers are host addresses that nothing dereferences, and no entry point that launches is called."""
import ctypes as C

import pytest
import torch

from tests import clip_text_ref as T
from tests import clip_vision_ref as V

FAMILIES = ("vae", "text", "vision", "vgg", "lpips", "fid")
HEAD = {"vgg": 256, "lpips": 256}      # bytes a module keeps at the head of its workspace: a buffer of that size holds nothing
ACTS = {"gelu": 0, "quick_gelu": 1}


def _create_args(family):
    """the smallest valid arguments of ``mvd_<family>_create``, without the trailing handle pointer"""
    from mvd_amd import _lib as L
    from mvd_amd import packing
    if family == "vae":      # the tiny topology of tests/test_oracle_vae.py
        c = L.mvd_vae_config_t(in_channels=3, latent_channels=4, num_levels=3, layers_per_block=1, norm_num_groups=32, norm_eps=1e-6)
        c.block_out_channels[:3] = (64, 64, 128)
        return (C.byref(c),)
    if family == "text":
        t = T.TINY
        c = L.mvd_text_config_t(vocab_size=t["vocab_size"], hidden_size=t["hidden_size"], intermediate_size=t["intermediate_size"],
                                num_layers=t["num_hidden_layers"], num_heads=t["num_attention_heads"], max_positions=t["max_position_embeddings"],
                                layer_norm_eps=t["layer_norm_eps"], act=ACTS[t["hidden_act"]])
        return (C.byref(c),)
    if family == "vision":
        t = V.TINY
        c = L.mvd_vision_config_t(image_size=t["image_size"], patch_size=t["patch_size"], hidden_size=t["hidden_size"],
                                  intermediate_size=t["intermediate_size"], num_layers=t["num_hidden_layers"], num_heads=t["num_attention_heads"],
                                  projection_dim=t["projection_dim"], layer_norm_eps=t["layer_norm_eps"], act=ACTS[t["hidden_act"]])
        return (C.byref(c),)
    if family == "fid":
        prog, bufs, names, final = packing.fid_program()
        return ((C.c_int * len(prog))(*prog), len(prog) // 13, (C.c_int * len(bufs))(*bufs), len(bufs) // 2,
                (C.c_char_p * len(names))(*[n.encode() for n in names]), len(names), final, 8)
    return ()


@pytest.fixture(params=FAMILIES)
def handle(request):
    from mvd_amd import _lib as L
    family, lib = request.param, L.lib()
    h = C.c_void_p()
    assert getattr(lib, f"mvd_{family}_create")(*_create_args(family), C.byref(h)) == 0, L.last_error()
    yield family, lib, h
    assert getattr(lib, f"mvd_{family}_destroy")(h) == 0


def test_set_weight_validates_before_it_stores(handle):
    from mvd_amd import _lib as L
    family, lib, h = handle
    set_weight = getattr(lib, f"mvd_{family}_set_weight")
    buf = (C.c_char * 64)()
    a16 = C.c_void_p((C.addressof(buf) + 15) & ~15)
    for args in ((None, b"slot", a16, 8, 0), (h, None, a16, 8, 0), (h, b"slot", None, 8, 0),      # null handle, slot, pointer
                 (h, b"slot", a16, 0, 0), (h, b"slot", a16, -3, 0),                               # numel <= 0
                 (h, b"slot", a16, 8, -1), (h, b"slot", a16, 8, 2)):                              # dtype outside {0, 1}
        assert set_weight(*args) < 0, (family, args)
        assert L.last_error() == f"{family}_set_weight: bad argument", (family, args, L.last_error())
    assert set_weight(h, b"some.slot", C.c_void_p(a16.value + 4), 8, 1) < 0
    assert L.last_error().startswith(f"{family}_set_weight: ") and "'some.slot'" in L.last_error() and "16-byte" in L.last_error()
    assert set_weight(h, b"some.slot", a16, 8, 0) == 0, L.last_error()
    assert set_weight(h, b"some.slot", a16, 12, 1) == 0, L.last_error()      # a slot may be set again


def test_bind_workspace_validates_before_it_stores(handle):
    from mvd_amd import _lib as L
    family, lib, h = handle
    bind = getattr(lib, f"mvd_{family}_bind_workspace")
    buf = (C.c_char * 4096)()
    addr = (C.addressof(buf) + 255) & ~255
    for args in ((None, C.c_void_p(addr), 1024), (h, None, 1024), (h, C.c_void_p(addr + 16), 1024),      # null handle, null / misaligned buffer
                 (h, C.c_void_p(addr), 0), (h, C.c_void_p(addr), -1)):                                   # bytes <= 0
        assert bind(*args) < 0, (family, args)
        assert L.last_error() == f"{family}_bind_workspace: bad argument (256-byte aligned buffer)", (family, args, L.last_error())
    assert (bind(h, C.c_void_p(addr), 256) < 0) == (family in HEAD), family
    assert bind(h, C.c_void_p(addr), HEAD.get(family, 0) + 1) == 0, L.last_error()
    assert bind(h, C.c_void_p(addr), 1024) == 0, L.last_error()


@pytest.mark.parametrize("family", FAMILIES)
def test_destroy_null_is_harmless(family):
    from mvd_amd import _lib as L
    assert getattr(L.lib(), f"mvd_{family}_destroy")(None) == 0


def test_python_handle_owns_what_it_creates():
    """``_lib.Handle``: create on construction, the library's message on a failed sizing call, destroy with the object"""
    from mvd_amd import _lib as L
    hd = L.Handle("vgg")
    assert hd.h and hd.ws is None and hd.workspace_bytes(2, 64, 64) > 256
    with pytest.raises(L.MvdError, match=r"^vgg workspace_bytes: .*bad shape"):
        hd.workspace_bytes(0, 64, 64)
    with pytest.raises(L.MvdError, match="mvd_text_create failed"):
        L.Handle("text", C.byref(L.mvd_text_config_t()))      # an all-zero config is no topology
    assert L.dtype_code(torch.zeros(1)) == 0 and L.dtype_code(torch.zeros(1, dtype=torch.bfloat16)) == 1
