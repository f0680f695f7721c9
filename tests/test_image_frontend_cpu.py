"""CPU checks of the image front end (N13): the numpy restatement tests/imageio_ref.py equals live PIL (when PIL is there) and the
recorded PIL output tests/golden/n13_frontend.npz byte for byte; the 0 / 255 inputs drive both passes' accumulators outside [0, 255];
every plausible mistake changes compared bytes on these inputs; and the two entry points check their arguments on the host."""
import ctypes as C
import os

import numpy as np
import pytest

import imageio_ref as R
from make_golden_n13 import golden_keys

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "n13_frontend.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def restated():
    """(case, kind, channels) -> (input, out_u8, out_f32, per-pass accumulator ranges), computed once"""
    out = {}
    for case, kind, ch, _ in golden_keys():
        x = R.make_input(case, kind, ch, 1)
        stats = []
        u8, f32 = R.frontend(x, case[2], case[3], stats=stats)
        out[(case, kind, ch)] = (x, u8, f32, stats)
    return out


def test_composite_all_alpha_value_pairs_against_pil():
    pytest.importorskip("PIL")
    a, v = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    px = np.stack([v, 255 - v, (v * 7 + a) % 256, a], -1).astype(np.uint8)[None]      # every (alpha, value) pair in the red channel
    want = R.pil_frontend(px, 256, 256)
    assert np.array_equal(R.composite_white(px), want)
    assert np.array_equal(R.composite_white(px, general=True), want)


def test_restatement_equals_live_pil(restated):
    pytest.importorskip("PIL")
    for (case, kind, ch), (x, u8, _, _) in restated.items():
        assert np.array_equal(u8, R.pil_frontend(x, case[2], case[3])), (case, kind, ch)


def test_restatement_equals_recorded_pil(restated, golden):
    assert str(golden["pil_version"])
    n = 0
    for case, kind, ch, key in golden_keys():
        assert np.array_equal(restated[(case, kind, ch)][1], golden[key]), key
        n += 1
    assert n == 9 * 4
    assert os.path.getsize(GOLDEN) < 1 << 20


def test_float_output_is_the_cpu_expression(restated):
    import torch
    for (case, kind, ch), (_, u8, f32, _) in restated.items():
        want = torch.from_numpy(u8).permute(0, 3, 1, 2).float() / 127.5 - 1.0
        assert torch.equal(torch.from_numpy(f32), want), (case, kind, ch)


def test_binary_inputs_clip_in_both_passes(restated):
    for case in R.CASES:
        stats = restated[(case, "binary", 4)][3]
        assert len(stats) == (case[0] != case[2]) + (case[1] != case[3])
        for lo, hi in stats:
            assert lo < 0 or hi > 255, (case, stats)
    # both directions of both clips somewhere in the set
    h_pass = [restated[(c, "binary", 4)][3][0] for c in R.CASES if c[1] != c[3]]
    v_pass = [restated[(c, "binary", 4)][3][-1] for c in R.CASES if c[0] != c[2] and c[1] != c[3]]
    for ranges in (h_pass, v_pass):
        assert min(lo for lo, _ in ranges) < 0 and max(hi for _, hi in ranges) > 255


FAULTS = {
    "no_rounding_constant": dict(rounding=False),
    "vertical_pass_first": dict(vertical_first=True),
    "resize_before_composite": dict(resize_first=True),
    "reciprocal_multiply": dict(reciprocal=True),
    "no_uint8_intermediate": dict(intermediate_u8=False),
    "support_2": dict(support=2.0),
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_fault_changes_compared_values(restated, fault):
    """each mistake must change bytes (for the reciprocal: floats) that the tests compare; the counts are recorded in DESIGN.md"""
    changed = 0
    for (case, kind, ch), (x, u8, f32, _) in restated.items():
        if ch != 4:
            continue
        bu8, bf32 = R.frontend(x, case[2], case[3], **FAULTS[fault])
        changed += int((bf32 != f32).sum()) if fault == "reciprocal_multiply" else int((bu8 != u8).sum())
    print(f"{fault}: {changed} compared values change")
    assert changed > 0


def test_reciprocal_and_fma_differ_on_many_byte_values():
    b = np.arange(256)
    exact = R.normalise(b.astype(np.uint8))
    recip = R.normalise(b.astype(np.uint8), reciprocal=True)
    fma = (b.astype(np.float64) * np.float64(np.float32(1.0 / 127.5)) - 1.0).astype(np.float32)     # one rounding
    assert int((recip != exact).sum()) == 111 and int((fma != exact).sum()) == 205


# ---------------------------------------------------------------- host-side argument checks of the two symbols (no GPU)
@pytest.fixture(scope="module")
def lib():
    from mvd_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L


def test_workspace_bytes_and_its_refusals(lib):
    f = lib.lib().mvd_op_image_frontend_workspace_bytes
    a = f(1, 1024, 1024, 4, 512, 512)
    b = f(8, 1024, 1024, 4, 512, 512)
    assert 1024 * 512 * 3 <= a < b < 8 * 1024 * 512 * 3 + (1 << 20)
    assert f(1, 32, 32, 3, 32, 32) >= 32 * 32 * 3
    for bad, word in (((0, 8, 8, 4, 8, 8), "bad shape"), ((1, 8, 8, 2, 8, 8), "channels"), ((1, 8, 8, 4, 0, 8), "bad shape"),
                      ((3, 16384, 16384, 4, 8192, 8192), "2^31"), ((1, 64, 4096, 4, 64, 256), "more than"), ((4096, 2048, 2048, 4, 8, 8), "2^31")):
        assert f(*bad) == -1 and word in lib.last_error(), (bad, lib.last_error())


def test_frontend_checks_its_arguments_before_any_launch(lib):
    f = lib.lib().mvd_op_image_frontend
    p = C.c_void_p(4096)
    assert f(None, 1, 8, 8, 4, 8, 8, p, p, p, 1 << 20, None) == -1 and "null source" in lib.last_error()
    assert f(p, 1, 8, 8, 4, 8, 8, None, None, p, 1 << 20, None) == -1 and "nothing to write" in lib.last_error()
    assert f(p, 1, 8, 8, 5, 8, 8, p, p, p, 1 << 20, None) == -1 and "channels" in lib.last_error()
    assert f(p, 1, 8, 8, 4, 8, 8, p, C.c_void_p(4098), p, 1 << 20, None) == -1 and "aligned" in lib.last_error()
    assert f(p, 1, 8, 8, 4, 8, 8, p, p, C.c_void_p(4100), 1 << 20, None) == -1 and "256-byte" in lib.last_error()
    assert f(p, 1, 8, 8, 4, 8, 8, p, p, None, 1 << 20, None) == -1
    assert f(p, 1, 16, 16, 4, 8, 8, p, p, p, 64, None) == -4 and "too small" in lib.last_error()
    spans = (C.c_int * 4)()
    assert lib.lib().mvd_op_image_frontend_spans(spans) == 0 and all(s > 0 for s in spans)


def test_composite_resize_refuses_cpu_tensors():
    import torch
    from mvd_amd import image_frontend as F
    from mvd_amd._lib import MvdError
    with pytest.raises(MvdError, match="CPU tensor"):
        F.composite_resize(torch.zeros(1, 8, 8, 4, dtype=torch.uint8), (4, 4))
    with pytest.raises(MvdError, match="uint8"):
        F.composite_resize(torch.zeros(1, 8, 8, 4), (4, 4))
    with pytest.raises(MvdError, match="not a GPU"):
        F.load_image_device("nothing.png", (4, 4), "cpu")
