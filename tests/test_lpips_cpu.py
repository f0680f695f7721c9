"""Host side of LPIPS: the network tables, the weight packing against an explicit im2col, the three key
families, offline weight resolution, every refusal of the Python surface, the C ABI's host-side checks and sizing dry run, and
the condition the GPU tests' distance bound rests on (lpips_ref.case: the bound stays below 0.3 d).  No GPU."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import lpips_ref as R

ALL_CASES = [(net, *s, close) for net in ("alex", "vgg") for s in R.SHAPES[net] for close in (False, True)]


# ------------------------------------------------------------------------------------------------ tables
def test_tables_match_the_restatement():
    from mvd_amd import lpips as M
    from mvd_amd import packing as P
    assert tuple((l[0], *l[2:]) for l in R.ALEX_LAYERS if l[1] == "conv") == P.ALEX_CONVS
    assert tuple(l[0] for l in R.ALEX_LAYERS if l[1] == "pool") == P.ALEX_POOLS
    assert [i for i, _ in M.ALEX_LAYERS] == [l[0] for l in R.ALEX_LAYERS] == list(range(12))
    assert [("conv" if "conv" in k else "pool" if "pool" in k else "relu") for _, k in M.ALEX_LAYERS] == [l[1] for l in R.ALEX_LAYERS]
    assert M.ALEX_TAPS == R.ALEX_TAPS and M.TAP_CHANNELS == R.CHANNELS
    assert P.LPIPS_SHIFT == R.SHIFT and P.LPIPS_SCALE == R.SCALE
    # the VGG tower's front end is the same affine map
    import vgg_ref as V
    assert all(abs(2 * m - 1 - s) < 1e-12 for m, s in zip(V.MEAN, R.SHIFT)) and all(abs(2 * d - s) < 1e-12 for d, s in zip(V.STD, R.SCALE))
    for (h, w), want in (((31, 31), [(7, 7), (3, 3), (1, 1)]), ((47, 66), [(11, 15), (5, 7), (2, 3)])):
        assert M.alex_tap_sizes(h, w)[:3] == want == R.alex_tap_sizes(h, w)[:3]
        taps = R.alex_taps(R.synthetic_alex_state_dict(), torch.zeros(1, 3, h, w))
        assert [tuple(t.shape[2:]) for t in taps] == M.alex_tap_sizes(h, w) and [t.shape[1] for t in taps] == list(R.CHANNELS["alex"])


# ------------------------------------------------------------------------------------------------ packing
def _im2col(x, k, stride, pad):
    """x (B, C, H, W) -> (B * oh * ow, k * k * C), column (ky * k + kx) * C + c, zero padding"""
    B, Cn, H, W = x.shape
    oh, ow = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    xp = F.pad(x, (pad, pad, pad, pad))
    cols = [xp[:, :, ky:ky + stride * (oh - 1) + 1:stride, kx:kx + stride * (ow - 1) + 1:stride].permute(0, 2, 3, 1).reshape(B * oh * ow, Cn)
            for ky in range(k) for kx in range(k)]
    return torch.cat(cols, 1)


@pytest.mark.parametrize("cin,cout,k,stride,pad,hw", [(3, 64, 11, 4, 2, (31, 38)), (64, 192, 5, 1, 2, (5, 7))])
def test_packed_weight_times_im2col_is_conv2d(cin, cout, k, stride, pad, hw):
    """integers in fp64: every product and sum is exact, so the two sides are equal, not close"""
    from mvd_amd.packing import ALEX_CONV1_COLS, pack_alex_conv
    g = torch.Generator().manual_seed(cin + cout)
    w = torch.randint(-3, 4, (cout, cin, k, k), generator=g).double()
    x = torch.randint(-5, 6, (2, cin, *hw), generator=g).double()
    want = F.conv2d(x, w, stride=stride, padding=pad).permute(0, 2, 3, 1).reshape(-1, cout)
    wp = pack_alex_conv(w).double()
    cols = _im2col(x, k, stride, pad)
    if cin == 3:
        assert wp.shape == (cout, ALEX_CONV1_COLS) and torch.count_nonzero(wp[:, 363:]) == 0
        cols = F.pad(cols, (0, ALEX_CONV1_COLS - 363), value=7.0)        # whatever the pad columns of the rows hold, the weights there are 0
    else:
        assert wp.shape == (cout, 1600)
    assert torch.equal(cols @ wp.T, want)


def test_pack_alex_slots():
    from mvd_amd.packing import normalize_lpips_lin_keys, pack_alex
    sd = R.synthetic_alex_state_dict()
    slots = pack_alex(sd, normalize_lpips_lin_keys(R.synthetic_lins("alex"), R.CHANNELS["alex"]), "cpu")
    shapes = {0: (64, 384), 3: (192, 1600), 6: (384, 9 * 192), 8: (256, 9 * 384), 10: (256, 9 * 256)}
    for idx, shape in shapes.items():
        w, b = slots[f"features.{idx}.weight"], slots[f"features.{idx}.bias"]
        assert w.dtype == torch.bfloat16 and tuple(w.shape) == shape and w.is_contiguous()
        assert b.dtype == torch.float32 and torch.equal(b, sd[f"features.{idx}.bias"])
    for k, c in enumerate(R.CHANNELS["alex"]):
        assert slots[f"lin{k}.weight"].shape == (c,) and slots[f"lin{k}.weight"].dtype == torch.float32
    # the synthetic weights are bf16 values: packing rounds nothing away
    w0 = slots["features.0.weight"].float()[:, :363].reshape(64, 11, 11, 3).permute(0, 3, 1, 2)
    assert torch.equal(w0, sd["features.0.weight"])


# ------------------------------------------------------------------------------------------------ keys
def _lpips_style(net, sd):
    """the keys of lpips.LPIPS(net).state_dict(): net.sliceK.N.*, lin{k}.model.1.weight and lins.{k}.model.1.weight"""
    slices = {"alex": {0: 1, 3: 2, 6: 3, 8: 4, 10: 5}, "vgg": {0: 1, 2: 1, 5: 2, 7: 2, 10: 3, 12: 3, 14: 3, 17: 4, 19: 4, 21: 4, 24: 5, 26: 5, 28: 5}}[net]
    out = {"scaling_layer.shift": torch.tensor(R.SHIFT).view(1, 3, 1, 1), "scaling_layer.scale": torch.tensor(R.SCALE).view(1, 3, 1, 1)}
    for k, v in sd.items():
        idx, leaf = k.split(".")[1:]
        out[f"net.slice{slices[int(idx)]}.{idx}.{leaf}"] = v
    for k, v in R.synthetic_lins(net).items():
        out[k] = v
        out["lins." + k[3:]] = v
    return out


@pytest.mark.parametrize("net", ["alex", "vgg"])
def test_key_normalisation(net):
    from mvd_amd._lib import MvdError
    from mvd_amd.lpips import LPIPS
    from mvd_amd.packing import ALEX_CONVS, VGG16_CONVS, normalize_backbone_keys, normalize_lpips_lin_keys
    sd, lins = R.backbone(net), R.synthetic_lins(net)
    convs = ALEX_CONVS if net == "alex" else VGG16_CONVS
    sliced = {k[len("features."):]: v for k, v in sd.items()}
    full = _lpips_style(net, sd)
    for form in (sd, sliced, full, {**sd, "classifier.6.bias": torch.zeros(1000)}):
        got = normalize_backbone_keys(form, convs, net)
        assert list(got) == list(sd) and all(got[k] is sd[k] for k in sd)
    want = {f"lin{k}.weight": lins[f"lin{k}.model.1.weight"].reshape(-1) for k in range(5)}
    for form in (lins, {"lins." + k[3:]: v for k, v in lins.items()}, full):
        got = normalize_lpips_lin_keys(form, R.CHANNELS[net])
        assert list(got) == list(want) and all(torch.equal(got[k], want[k]) for k in want)
    # a full lpips state dict serves both arguments, given as either
    for kw in (dict(backbone=full), dict(model_path=full), dict(backbone=sd, model_path=lins), dict(backbone=sliced, model_path=full)):
        m = LPIPS(net=net, **kw)
        assert all(torch.equal(m.backbone[k], sd[k]) for k in sd) and all(torch.equal(m.lins[k], want[k]) for k in want)
    missing = {k: v for k, v in sd.items() if k != "features.0.bias"}
    with pytest.raises(MvdError, match="features.0.bias"):
        normalize_backbone_keys(missing, convs, net)
    with pytest.raises(MvdError, match="shape"):
        normalize_backbone_keys({**sd, "features.0.weight": torch.zeros(64, 3, 3)}, convs, net)
    with pytest.raises(MvdError, match="lin4"):
        normalize_lpips_lin_keys({k: v for k, v in lins.items() if not k.startswith("lin4")}, R.CHANNELS[net])
    with pytest.raises(MvdError, match="shape"):
        normalize_lpips_lin_keys({**lins, "lin0.model.1.weight": torch.zeros(64)}, R.CHANNELS[net])
    with pytest.raises(MvdError, match="state dict"):
        normalize_backbone_keys([1, 2], convs, net)


# ------------------------------------------------------------------------------------------------ the surface's refusals
def make(net="alex", **kw):
    from mvd_amd.lpips import LPIPS
    return LPIPS(net=net, backbone=R.backbone(net), model_path=R.synthetic_lins(net), **kw)


def test_constructor_arguments():
    from mvd_amd._lib import MvdError
    m = make(pretrained=True, lpips=True, use_dropout=True, eval_mode=True, verbose=False)       # lpips' own keywords
    assert m.to("cuda") is m and m.eval() is m and m.cuda() is m
    for kw, pat in ((dict(spatial=True), "spatial"), (dict(lpips=False), "lpips"), (dict(pnet_rand=True), "pnet_rand"),
                    (dict(version="0.0"), "version"), (dict(max_pairs_per_pass=0), "max_pairs_per_pass"), (dict(colour=1), "colour")):
        with pytest.raises(MvdError, match=pat):
            make(**kw)
    from mvd_amd.lpips import LPIPS
    with pytest.raises(MvdError, match="squeeze"):
        LPIPS(net="squeeze", backbone=R.backbone("alex"), model_path=R.synthetic_lins("alex"))


def test_negative_linear_weight_is_refused():
    from mvd_amd._lib import MvdError
    from mvd_amd.lpips import LPIPS
    lins = dict(R.synthetic_lins("alex"))
    bad = lins["lin2.model.1.weight"].clone()
    bad[0, 17, 0, 0] = -1e-3
    lins["lin2.model.1.weight"] = bad
    with pytest.raises(MvdError, match="negative"):
        LPIPS(net="alex", backbone=R.backbone("alex"), model_path=lins)


def test_small_and_cpu_inputs_are_refused():
    from mvd_amd._lib import MvdError
    alex, vgg = make("alex"), make("vgg")
    with pytest.raises(MvdError, match="31 x 31"):
        alex(torch.zeros(1, 3, 30, 64), torch.zeros(1, 3, 30, 64))
    with pytest.raises(MvdError, match="16 x 16"):
        vgg(torch.zeros(1, 3, 15, 32), torch.zeros(1, 3, 15, 32))
    x = torch.zeros(1, 3, 32, 32)
    for m in (alex, vgg):
        with pytest.raises(MvdError, match="no CPU fallback"):
            m(x, x)
        with pytest.raises(MvdError, match="no CPU fallback"):
            m.features(x)
        with pytest.raises(MvdError, match=r"\(B, 3, H, W\)"):
            m(x[0], x[0])


def test_weights_resolve_offline_only(tmp_path, monkeypatch):
    from mvd_amd import lpips as M
    from mvd_amd._lib import MvdError
    home = tmp_path / "torch_home"
    monkeypatch.setenv("TORCH_HOME", str(home))
    monkeypatch.setenv("HOME", str(tmp_path / "nobody"))
    monkeypatch.setattr(M, "_lpips_package_dirs", lambda: [])           # no lpips package
    ck = home / "hub" / "checkpoints"
    sd, lins = R.backbone("alex"), R.synthetic_lins("alex")
    with pytest.raises(MvdError) as e:
        M.LPIPS(net="alex")
    assert str(ck / M.ALEX_FILE) in str(e.value) and "Nothing is downloaded" in str(e.value)       # the paths tried
    ck.mkdir(parents=True)
    torch.save(sd, str(ck / M.ALEX_FILE))
    with pytest.raises(MvdError) as e:
        M.LPIPS(net="alex")
    assert str(ck / "lpips-v0.1-alex.pth") in str(e.value) and "linear-head" in str(e.value)
    torch.save(lins, str(ck / "lpips-v0.1-alex.pth"))
    m = M.LPIPS(net="alex")
    assert all(torch.equal(m.backbone[k], sd[k]) for k in sd)
    assert torch.equal(m.lins["lin3.weight"], lins["lin3.model.1.weight"].reshape(-1))
    # the lpips package's own file, located without importing the package
    pkg = tmp_path / "site" / "lpips"
    (pkg / "weights" / "v0.1").mkdir(parents=True)
    other = {k: v * 2 for k, v in lins.items()}
    torch.save(other, str(pkg / "weights" / "v0.1" / "alex.pth"))
    monkeypatch.setattr(M, "_lpips_package_dirs", lambda: [str(pkg)])
    assert M.lin_weight_candidates("alex")[0] == str(pkg / "weights" / "v0.1" / "alex.pth")
    assert torch.equal(M.LPIPS(net="alex").lins["lin0.weight"], other["lin0.model.1.weight"].reshape(-1))
    with pytest.raises(MvdError, match="does not exist"):
        M.LPIPS(net="alex", backbone=str(tmp_path / "missing.pth"))
    with pytest.raises(MvdError, match="does not exist"):
        M.LPIPS(net="alex", model_path=str(tmp_path / "missing.pth"))
    not_sd = tmp_path / "list.pth"
    torch.save([1, 2, 3], str(not_sd))
    with pytest.raises(MvdError, match="not a state dict"):
        M.LPIPS(net="alex", backbone=str(not_sd))


# ------------------------------------------------------------------------------------------------ the C ABI on the host
def test_lpips_host_side_checks_and_dry_run():
    """argument validation and the sizing dry run need no GPU"""
    from mvd_amd import _lib as L
    lib = L.lib()
    h = C.c_void_p()
    assert lib.mvd_lpips_create(C.byref(h)) == 0
    small, big, bigger = (lib.mvd_lpips_workspace_bytes(h, *a) for a in ((2, 31, 31), (2, 64, 64), (4, 64, 64)))
    assert 0 < small < big < bigger
    # at least the im2col rows of conv1: images x 15 x 15 rows of 384 bf16
    assert bigger >= 4 * 15 * 15 * 384 * 2
    assert lib.mvd_lpips_workspace_bytes(h, 1, 30, 64) < 0 and b"31" in lib.mvd_last_error()
    assert lib.mvd_lpips_workspace_bytes(h, 1, 64, 30) < 0
    assert lib.mvd_lpips_workspace_bytes(h, 1 << 20, 32768, 32768) < 0 and b"2^31" in lib.mvd_last_error()
    buf = (C.c_char * 4096)()
    addr = (C.addressof(buf) + 255) & ~255
    assert lib.mvd_lpips_bind_workspace(h, C.c_void_p(addr), 1024) == 0
    assert lib.mvd_lpips_bind_workspace(h, C.c_void_p(addr + 16), 1024) < 0
    one = C.c_float()
    # no weights yet: the missing slot is reported before anything is launched
    assert lib.mvd_lpips_distance(h, C.c_void_p(addr), C.c_void_p(addr), 1, 32, 32, 0, C.byref(one), None, None, None) == -10
    assert b"features.0.weight" in lib.mvd_last_error()
    w = (C.c_char * 64)()
    a16 = (C.addressof(w) + 15) & ~15
    assert lib.mvd_lpips_set_weight(h, b"features.0.weight", C.c_void_p(a16), 7, 1) == 0
    assert lib.mvd_lpips_distance(h, C.c_void_p(addr), C.c_void_p(addr), 1, 32, 32, 0, C.byref(one), None, None, None) == -11
    assert lib.mvd_lpips_set_weight(h, b"features.0.weight", C.c_void_p(a16), 64 * 384, 0) == 0      # the size is right, the dtype is not
    assert lib.mvd_lpips_distance(h, C.c_void_p(addr), C.c_void_p(addr), 1, 32, 32, 0, C.byref(one), None, None, None) == -11
    assert lib.mvd_lpips_set_weight(h, b"features.0.weight", C.c_void_p(a16 + 4), 7, 1) < 0          # alignment
    assert lib.mvd_lpips_distance(h, C.c_void_p(addr), C.c_void_p(addr), 1, 30, 32, 0, C.byref(one), None, None, None) == -1
    assert lib.mvd_lpips_distance(h, C.c_void_p(addr), C.c_void_p(addr), 1, 32, 32, 0, None, None, None, None) == -1
    assert lib.mvd_lpips_destroy(h) == 0
    px = (C.c_int * 3)(1, 256, 257)
    assert lib.mvd_op_lpips_head_ws_bytes(3, px, 5) == 256 + 256                    # 5 x (1 + 1 + 2) chunk sums of 8 bytes, rounded up
    assert lib.mvd_op_lpips_head_ws_bytes(9, px, 1) < 0 and lib.mvd_op_lpips_head_ws_bytes(3, px, 0) < 0
    assert lib.mvd_op_maxpool3x3s2(C.c_void_p(addr), 1, 2, 5, 8, C.c_void_p(addr), None) == -1
    assert lib.mvd_op_maxpool3x3s2(C.c_void_p(addr), 1, 5, 5, 12, C.c_void_p(addr), None) == -1
    assert lib.mvd_op_im2col_patch(C.c_void_p(addr), 2, 1, 31, 31, None, None, C.c_void_p(addr), None) == -1
    assert lib.mvd_op_im2col_patch(C.c_void_p(addr), 0, 1, 6, 31, None, None, C.c_void_p(addr), None) == -1


@pytest.mark.parametrize("size,pp", [(160, 8), (192, 6), (128, 13), (96, 15), (64, 2), (31, 16), (512, 8)])
def test_workspace_covers_every_shorter_pass(size, pp):
    """the split-K of a convolution is not monotone in the batch (160 x 160: conv2 of 7 pairs is split two ways, that of 8 pairs is
    not), but the bytes of a pass must be: a workspace sized for a full pass of pp pairs holds every remainder pass"""
    from mvd_amd import _lib as L
    lib = L.lib()
    h = C.c_void_p()
    assert lib.mvd_lpips_create(C.byref(h)) == 0
    need = [lib.mvd_lpips_workspace_bytes(h, 2 * n, size, size) for n in range(1, pp + 1)]
    assert all(a > 0 for a in need) and all(a <= b for a, b in zip(need, need[1:])), need
    odd = [lib.mvd_lpips_workspace_bytes(h, n, size, size) for n in range(1, 2 * pp + 1)]      # mvd_lpips_features takes any count
    assert all(a <= b for a, b in zip(odd, odd[1:])), odd
    assert lib.mvd_lpips_destroy(h) == 0


# ------------------------------------------------------------------------------------------------ the synthetic inputs
@pytest.mark.parametrize("net,pairs,h,w,close", ALL_CASES)
def test_the_distance_bound_is_a_bound_worth_having(net, pairs, h, w, close):
    """the condition the GPU tests rely on: with eta_l = 2 x the emulation's error on g_l, sum_l d_l (2 eta_l + eta_l^2) stays
    below 0.3 d for every pair; the emulation itself is inside that bound; the taps are neither dead nor exploding; identical
    inputs give exactly 0"""
    c = R.case(net, pairs, h, w, close)
    print(f"{net} {(pairs, h, w)} close={close}: tap emulation rel-L2 {['%.2e' % e for e in c.emu]}, eps_l max {c.eps.max().item():.3e}, "
          f"d {c.d.tolist()}, bound / d {[b / d for b, d in zip(c.bound, c.d.tolist())]}, "
          f"emulation |dd| / d {((c.d_emu - c.d).abs() / c.d).tolist()}")
    assert all(0.0 < e <= 1e-2 for e in c.emu), c.emu
    for p in range(pairs):
        d = c.d[p].item()
        assert d > 0.0 and c.bound[p] <= 0.3 * d, (p, d, c.bound[p])
        assert abs(c.d_emu[p].item() - d) <= c.bound[p]
    assert all(0.05 <= float(t.double().pow(2).mean().sqrt()) <= 20.0 for t in c.taps)
    if not close:
        z = R.distance(net, c.sd, c.lins, c.x, c.x.clone())
        assert torch.equal(z, torch.zeros(pairs))
        # fp32 and fp64 restatements agree: the reference the GPU is held to is not itself noisy
        d32 = R.distance(net, c.sd, c.lins, c.x, c.y)
        assert torch.allclose(d32.double(), c.d, rtol=1e-4, atol=0)


@pytest.mark.parametrize("net", ["alex", "vgg"])
def test_restatement_against_the_lpips_package(net):
    """where lpips and torchvision import: the package's own class on the shared state dict"""
    lp = pytest.importorskip("lpips")
    pytest.importorskip("torchvision")
    m = lp.LPIPS(net=net, pretrained=False, pnet_rand=True, verbose=False).eval()
    sd = _lpips_style(net, R.backbone(net))
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not [k for k in missing if not k.startswith("scaling_layer")] and not unexpected, (missing, unexpected)
    pairs, h, w = R.SHAPES[net][1]
    c = R.case(net, pairs, h, w)
    with torch.no_grad():
        want = m(c.x, c.y).reshape(-1)
    got = R.distance(net, c.sd, c.lins, c.x, c.y)
    assert torch.allclose(got, want, rtol=1e-4, atol=1e-7)
