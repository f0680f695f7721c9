"""Bit-exact tests of ``mvd_op_image_frontend`` (csrc/imageio.hip) and of what stands on it (``composite_resize``,
``load_image_device``, ``DeviceCollate``).

Every comparison is ``torch.equal``: the bytes against PIL's recorded output (tests/golden/n13_frontend.npz) and against the numpy
restatement tests/imageio_ref.py, which tests/test_image_frontend_cpu.py pins to live PIL; the floats against the CPU's
``float() / 127.5 - 1.0``.  The source is a slice of a larger buffer of random bytes (at an offset that keeps the 16-byte path, and at
an odd one), the outputs are pre-filled and have guard bytes behind them, and so has the workspace behind its reported size.
Without csrc/imageio.hip this file fails at the binding's symbol check."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import imageio_ref as R
from make_golden_n13 import golden_keys

pytestmark = pytest.mark.gpu

GUARD = 4096
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "n13_frontend.npz")


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mvd_amd import _lib
    _lib.lib()
    return _lib


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def big_random():
    g = torch.Generator().manual_seed(13)
    return torch.randint(0, 256, (4 * 300 * 520 * 4 + 4096,), dtype=torch.uint8, generator=g).cuda()


def run_op(L, big, x, out_h, out_w, mode, offset):
    """one call on x (numpy (B, h, w, ch)) placed at `offset` bytes into a copy of the random buffer; returns (u8 | None, f32 | None)
    after checking the guards"""
    B, h, w, ch = x.shape
    buf = big.clone()
    n = x.size
    buf[offset:offset + n] = torch.from_numpy(x.reshape(-1)).cuda()
    src = buf[offset:offset + n]
    need = L.lib().mvd_op_image_frontend_workspace_bytes(B, h, w, ch, out_h, out_w)
    assert need > 0, L.last_error()
    ws = torch.full((need + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    nu, nf = B * out_h * out_w * 3, B * 3 * out_h * out_w
    u = torch.full((nu + GUARD,), 0x5A, dtype=torch.uint8, device="cuda") if mode != "float" else None
    f = torch.full((nf + GUARD // 4,), float("nan"), dtype=torch.float32, device="cuda") if mode != "uint8" else None
    L.call("mvd_op_image_frontend", C.c_void_p(src.data_ptr()), B, h, w, ch, out_h, out_w, C.c_void_p(u.data_ptr() if u is not None else None),
           C.c_void_p(f.data_ptr() if f is not None else None), C.c_void_p(ws.data_ptr()), need, L.stream())
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0xA5).all()), "wrote beyond the reported workspace size"
    if u is not None:
        assert bool((u[nu:] == 0x5A).all()), "wrote behind out_u8"
        u = u[:nu].view(B, out_h, out_w, 3).cpu()
    if f is not None:
        assert bool(f[nf:].isnan().all()), "wrote behind out_f32"
        f = f[:nf].view(B, 3, out_h, out_w).cpu()
    return u, f


def expect(x, case):
    u8, f32 = R.frontend(x, case[2], case[3])
    want_f = torch.from_numpy(u8).permute(0, 3, 1, 2).float() / 127.5 - 1.0          # the CPU expression itself
    assert torch.equal(torch.from_numpy(f32), want_f)
    return torch.from_numpy(u8), want_f


def first_diff(got, want):
    bad = (got != want).nonzero()
    return f"{len(bad)} differ, first at {bad[0].tolist()}: {got[tuple(bad[0])].item()} != {want[tuple(bad[0])].item()}" if len(bad) else ""


@pytest.mark.parametrize("case", R.CASES, ids=R.case_name)
def test_every_case_every_output_mode(L, big_random, golden, case):
    oh, ow = case[2], case[3]
    for ch in (4, 3):
        x3 = R.make_input(case, "random", ch, 3)
        want_u3, want_f3 = expect(x3, case)
        assert np.array_equal(want_u3[:1].numpy(), golden[f"{R.case_name(case)}_random_c{ch}"])
        for batch in (1, 3):
            x, want_u, want_f = x3[:batch], want_u3[:batch], want_f3[:batch]
            # offset 20: 4-byte aligned, not 16 (RGBA keeps its 16-byte loads, chunks straddle the start); 7: the bytewise path
            for offset in ((20, 7) if ch == 4 else (7,)):
                u, f = run_op(L, big_random, x, oh, ow, "both", offset)
                assert torch.equal(u, want_u), (ch, batch, offset, first_diff(u, want_u))
                assert torch.equal(f, want_f), (ch, batch, offset, first_diff(f, want_f))
            u1, _ = run_op(L, big_random, x, oh, ow, "uint8", 32)
            _, f1 = run_op(L, big_random, x, oh, ow, "float", 32)
            assert torch.equal(u1, want_u) and torch.equal(f1, want_f), (ch, batch)
            u2, f2 = run_op(L, big_random, x, oh, ow, "both", 20 if ch == 4 else 7)
            assert torch.equal(u2, u) and torch.equal(f2, f)           # two calls, the same bits


def test_binary_and_smooth_images_equal_recorded_pil(L, big_random, golden):
    for case, kind, ch, key in golden_keys():
        if kind == "random":
            continue
        u, f = run_op(L, big_random, R.make_input(case, kind, ch, 1), case[2], case[3], "both", 16)
        want = torch.from_numpy(golden[key])
        assert torch.equal(u, want), (key, first_diff(u, want))
        assert torch.equal(f, want.permute(0, 3, 1, 2).float() / 127.5 - 1.0), key


def test_all_byte_values_through_the_float_output(L, big_random):
    x = np.arange(256, dtype=np.uint8).repeat(3).reshape(1, 16, 16, 3)      # no resize: the bytes go straight through
    u, f = run_op(L, big_random, x, 16, 16, "both", 3)
    assert torch.equal(u, torch.from_numpy(x))
    table = torch.arange(256, dtype=torch.uint8).float() / 127.5 - 1.0
    assert torch.equal(f[0, 0].reshape(-1), table) and torch.equal(f[0, 2].reshape(-1), table)
    from mvd_amd import image_frontend as F
    g = F.composite_resize(torch.from_numpy(x).cuda(), (16, 16))
    assert torch.equal(g.cpu(), f)


def test_alphas_on_both_sides_of_every_workgroup_boundary(L, big_random):
    from mvd_amd import image_frontend as F
    sp = F.spans()
    case = (300, 520, 136, 264)
    h, w, oh, ow = case
    # the case crosses every kind of boundary: several column spans and row groups in both kernels
    assert ow > sp["h_cols"] and h > sp["h_rows"] and ow > sp["v_cols"] and oh > sp["v_rows"]
    rng = np.random.RandomState(5)
    x = rng.randint(0, 256, (1, h, w, 4)).astype(np.uint8)
    x[..., 3] = 255
    alphas = np.array([0, 1, 127, 128, 254, 255], np.uint8)
    _, xb, _ = R.coefficients(w, ow)
    _, yb, _ = R.coefficients(h, oh)
    cols, rows = {0, w - 1}, {0, h - 1}
    for c in list(range(sp["h_cols"], ow, sp["h_cols"])) + list(range(sp["v_cols"], ow, sp["v_cols"])):
        for o in (c - 1, c):                                  # every source column the two output columns at the boundary read
            cols.update(range(xb[o][0], xb[o][0] + xb[o][1]))
    for r in range(sp["v_rows"], oh, sp["v_rows"]):
        for o in (r - 1, r):
            rows.update((yb[o][0], yb[o][0] + yb[o][1] - 1))
    rows.update(r + d for r in range(sp["h_rows"], h, sp["h_rows"]) for d in (-1, 0))
    for i, c in enumerate(sorted(cols)):
        x[0, :, c, 3] = alphas[(np.arange(h) + i) % 6]
    for i, r in enumerate(sorted(rows)):
        x[0, r, :, 3] = alphas[(np.arange(w) + i) % 6]
    for (yy, xx), a in zip(((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)), (0, 1, 127, 254)):
        x[0, yy, xx, 3] = a
    want_u, want_f = expect(x, case)
    assert not np.array_equal(want_u.numpy(), R.resize_u8(x[..., :3], oh, ow))          # the alphas matter
    for offset in (16, 20, 5):
        u, f = run_op(L, big_random, x, oh, ow, "both", offset)
        assert torch.equal(u, want_u), (offset, first_diff(u, want_u))
        assert torch.equal(f, want_f), offset


def test_composite_resize_shapes_and_modes(L):
    from mvd_amd import image_frontend as F
    case = (53, 47, 32, 32)
    x = R.make_input(case, "smooth", 4, 3)
    want_u, want_f = expect(x, case)
    xd = torch.from_numpy(x).cuda()
    f, u = F.composite_resize(xd, (32, 32), out="both")
    assert torch.equal(f.cpu(), want_f) and torch.equal(u.cpu(), want_u)
    assert torch.equal(F.composite_resize(xd[0], (32, 32)).cpu(), want_f[:1])
    assert torch.equal(F.composite_resize(xd, (32, 32), out="uint8").cpu(), want_u)
    # PIL's (width, height) order
    c2 = (100, 100, 40, 24)
    x2 = R.make_input(c2, "random", 3, 1)
    assert torch.equal(F.composite_resize(torch.from_numpy(x2).cuda(), (24, 40), out="uint8").cpu(), expect(x2, c2)[0])


def test_load_image_device_equals_load_image(L, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from mvd_amd import image_frontend as F
    from mvd_amd.utils import load_image
    rng = np.random.RandomState(3)
    for mode, shape in (("RGBA", (90, 70, 4)), ("RGB", (64, 64, 3)), ("L", (50, 60))):
        p = tmp_path / f"img_{mode}.png"
        Image.fromarray(rng.randint(0, 256, shape).astype(np.uint8), mode).save(p)
        for size in ((64, 64), (48, 80)):
            assert torch.equal(F.load_image_device(p, size, "cuda").cpu(), load_image(p, size)), (mode, size)


def test_device_collate_equals_host_mode(L, tmp_path):
    pytest.importorskip("PIL")
    import n13_tree as T
    from mvd_amd.dataset import DeviceCollate, ObjaverseDataset
    from torch.utils.data import DataLoader, default_collate
    root = T.build_tree(tmp_path)
    kw = dict(data_root=str(root), split="train", split_ratio=(1.0, 0.0, 0.0), target_size=(32, 32), max_views_per_object=3)
    host = ObjaverseDataset(**kw)
    dev = ObjaverseDataset(frontend="device", **kw)
    assert len(host) == len(dev) > 4
    hl = DataLoader(host, batch_size=5, shuffle=False)
    dl = DataLoader(dev, batch_size=5, shuffle=False, collate_fn=DeviceCollate("cuda", (32, 32)))
    n = 0
    for hb, db in zip(hl, dl):
        assert list(hb.keys()) == list(db.keys())
        for k in hb:
            if isinstance(hb[k], torch.Tensor):
                assert db[k].dtype == hb[k].dtype and db[k].shape == hb[k].shape
                assert torch.equal(db[k].cpu(), hb[k]), k
            else:
                assert db[k] == hb[k], k
        assert db["source_image"].is_cuda and db["target_image"].is_cuda
        n += 1
    assert n >= 2
