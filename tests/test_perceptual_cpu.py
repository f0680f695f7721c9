"""Host side of the VGG-16 perceptual loss: the network's schema, the weight packing against an explicit
im2col, offline weight resolution, the integration shim, and the condition of the GPU tests' synthetic inputs.  No GPU."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

import vgg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ schema
def test_layer_table_and_parameter_count():
    from mvd_amd import packing as P
    from mvd_amd.perceptual import VGG16FeaturesHIP
    assert P.VGG16_CONVS == R.CONVS and P.VGG16_POOLS == R.POOLS and P.VGG16_PARAMS == R.PARAMS == 14_714_688
    assert [i for i, k in R.layer_table() if k == "conv"] == [0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28]
    assert [i for i, k in R.layer_table() if k == "pool"] == [4, 9, 16, 23] and R.layer_table()[-1] == (28, "conv")
    m = VGG16FeaturesHIP()
    sd = m.state_dict()
    want = [f"features.{i}.{leaf}" for i, _, _ in R.CONVS for leaf in ("weight", "bias")]
    assert list(sd) == want and len(sd) == 26
    assert sum(t.numel() for t in sd.values()) == R.PARAMS
    assert sum(t.numel() for t in R.synthetic_state_dict().values()) == R.PARAMS
    # every convolution continues where the previous one stopped
    for (_, _, cout), (_, cin, _) in zip(R.CONVS, R.CONVS[1:]):
        assert cout == cin


def test_state_dict_key_forms_and_errors():
    from mvd_amd._lib import MvdError
    from mvd_amd.packing import normalize_vgg_keys
    from mvd_amd.perceptual import VGG16FeaturesHIP
    sd = R.synthetic_state_dict()
    tv = dict(sd)
    tv["classifier.0.weight"] = torch.zeros(4, 4)                 # torchvision's full model: ignored
    tv["features.0.num_batches_tracked"] = torch.zeros(())
    sliced = {k[len("features."):]: v for k, v in sd.items()}     # the keys of vgg16().features[:29].state_dict()
    for form in (sd, tv, sliced):
        got = normalize_vgg_keys(form)
        assert list(got) == list(sd) and all(got[k] is sd[k] for k in sd)
        m = VGG16FeaturesHIP()
        m.load_state_dict(form)
        assert all(torch.equal(m.state_dict()[k], sd[k]) for k in sd)
    missing = {k: v for k, v in sd.items() if k != "features.17.bias"}
    with pytest.raises(MvdError, match="features.17.bias"):
        VGG16FeaturesHIP().load_state_dict(missing)
    wrong = dict(sd)
    wrong["features.5.weight"] = torch.zeros(128, 64, 1, 1)
    with pytest.raises(MvdError, match="features.5.weight"):
        VGG16FeaturesHIP().load_state_dict(wrong)
    with pytest.raises(MvdError, match="state dict"):
        normalize_vgg_keys([1, 2, 3])
    with pytest.raises(MvdError, match="no weights"):
        VGG16FeaturesHIP()._sync(torch.device("cpu"))


# ------------------------------------------------------------------------------------------------ packing
def _im2col_slices(x):
    """x (B, C, H, W), C % 64 == 0 -> (B*H*W, 9*C) in the implicit-GEMM K order [C/64][ky][kx][64] of gemm.hip, zero padding"""
    B, C, H, W = x.shape
    xp = F.pad(x, (1, 1, 1, 1))
    cols = []
    for cs in range(C // 64):
        for ky in range(3):
            for kx in range(3):
                cols.append(xp[:, cs * 64:(cs + 1) * 64, ky:ky + H, kx:kx + W].permute(0, 2, 3, 1).reshape(B * H * W, 64))
    return torch.cat(cols, 1)


def _im2col_in(x):
    """x (B, 3, H, W) -> (B*H*W, 64): column tap * 3 + channel, zero padded from 27 (im2col_in_kernel of misc.hip)"""
    B, C, H, W = x.shape
    xp = F.pad(x, (1, 1, 1, 1))
    cols = [xp[:, :, ky:ky + H, kx:kx + W].permute(0, 2, 3, 1).reshape(B * H * W, C) for ky in range(3) for kx in range(3)]
    return F.pad(torch.cat(cols, 1), (0, 64 - 9 * C))


@pytest.mark.parametrize("cin,cout", [(3, 64), (64, 128), (128, 64)])
def test_packed_weight_times_im2col_is_conv2d(cin, cout):
    """integers in fp64: every product and sum is exact, so the two sides are equal, not close"""
    from mvd_amd.packing import pack_vgg_conv
    g = torch.Generator().manual_seed(cin + cout)
    w = torch.randint(-3, 4, (cout, cin, 3, 3), generator=g).double()
    x = torch.randint(-5, 6, (2, cin, 5, 7), generator=g).double()
    want = F.conv2d(x, w, padding=1).permute(0, 2, 3, 1).reshape(-1, cout)
    wp = pack_vgg_conv(w).double()
    assert wp.shape == (cout, 64 if cin == 3 else 9 * cin)
    cols = _im2col_in(x) if cin == 3 else _im2col_slices(x)
    assert torch.equal(cols @ wp.T, want)
    if cin == 3:
        assert torch.count_nonzero(wp[:, 27:]) == 0


def test_pack_vgg_slots():
    from mvd_amd.packing import pack_vgg
    sd = R.synthetic_state_dict()
    slots = pack_vgg(sd, "cpu")
    assert list(slots) == list(sd)
    for idx, cin, cout in R.CONVS:
        w, b = slots[f"features.{idx}.weight"], slots[f"features.{idx}.bias"]
        assert w.dtype == torch.bfloat16 and tuple(w.shape) == (cout, 64 if cin == 3 else 9 * cin) and w.is_contiguous()
        assert b.dtype == torch.float32 and torch.equal(b, sd[f"features.{idx}.bias"])
    # the synthetic weights are bf16 values: packing rounds nothing away
    w0 = slots["features.2.weight"].float().reshape(64, 1, 3, 3, 64).permute(0, 1, 4, 2, 3).reshape(64, 64, 3, 3)
    assert torch.equal(w0, sd["features.2.weight"])


# ------------------------------------------------------------------------------------------------ offline resolution
def test_weights_resolve_offline_only(tmp_path, monkeypatch):
    from mvd_amd._lib import MvdError
    from mvd_amd.perceptual import VGG16_FILE, PerceptualLoss, hub_checkpoint_dirs
    sd = R.synthetic_state_dict()
    home = tmp_path / "torch_home"
    monkeypatch.setenv("TORCH_HOME", str(home))
    monkeypatch.setenv("HOME", str(tmp_path / "nobody"))
    assert hub_checkpoint_dirs()[0] == str(home / "hub" / "checkpoints")
    with pytest.raises(MvdError, match="nothing is downloaded"):
        PerceptualLoss()
    (home / "hub" / "checkpoints").mkdir(parents=True)
    full = dict(sd)
    full["classifier.6.bias"] = torch.zeros(1000)
    torch.save(full, str(home / "hub" / "checkpoints" / VGG16_FILE))
    same = lambda m: all(torch.equal(m.vgg.state_dict()[k], sd[k]) for k in sd)      # noqa: E731
    assert same(PerceptualLoss())                                    # TORCH_HOME
    assert same(PerceptualLoss("cuda", weights=str(home / "hub" / "checkpoints" / VGG16_FILE)))
    assert same(PerceptualLoss(weights=sd))
    monkeypatch.delenv("TORCH_HOME")
    fallback = tmp_path / "nobody" / ".cache" / "torch" / "hub" / "checkpoints"
    fallback.mkdir(parents=True)
    torch.save(sd, str(fallback / VGG16_FILE))
    assert same(PerceptualLoss())                                    # ~/.cache/torch
    with pytest.raises(MvdError, match="does not exist"):
        PerceptualLoss(weights=str(tmp_path / "missing.pth"))
    wrong = dict(sd)
    wrong["features.28.weight"] = torch.zeros(512, 512, 3)
    with pytest.raises(MvdError, match="features.28.weight"):
        PerceptualLoss(weights=wrong)
    not_sd = tmp_path / "list.pth"
    torch.save([1, 2, 3], str(not_sd))
    with pytest.raises(MvdError, match="not a state dict"):
        PerceptualLoss(weights=str(not_sd))
    with pytest.raises(MvdError, match="max_pairs_per_pass"):
        PerceptualLoss(weights=sd, max_pairs_per_pass=0)


def test_safetensors_file(tmp_path):
    st = pytest.importorskip("safetensors.torch")
    from mvd_amd.perceptual import PerceptualLoss
    sd = R.synthetic_state_dict()
    path = str(tmp_path / "vgg16.safetensors")
    st.save_file({k: v.contiguous() for k, v in sd.items()}, path)
    m = PerceptualLoss(weights=path)
    assert all(torch.equal(m.vgg.state_dict()[k], sd[k]) for k in sd)


def test_cpu_tensors_raise():
    from mvd_amd._lib import MvdError
    from mvd_amd.perceptual import PerceptualLoss, VGG16FeaturesHIP
    loss = PerceptualLoss(weights=R.synthetic_state_dict())
    assert loss.to("cuda") is loss
    x = R.synthetic_images(1, 32, 32)
    with pytest.raises(MvdError, match="no CPU fallback"):
        loss(x, x)
    with pytest.raises(MvdError, match="no CPU fallback"):
        loss.per_sample(x, x)
    m = VGG16FeaturesHIP()
    m.load_state_dict(R.synthetic_state_dict())
    with pytest.raises(MvdError, match="no CPU fallback"):
        m(x)
    with pytest.raises(MvdError, match=r"\(B, 3, H, W\)"):
        loss(x[0], x[0])


def test_shim_exports_perceptual_loss():
    p = os.path.join(ROOT, "integration")
    sys.path.insert(0, p)
    saved = {k: sys.modules.pop(k) for k in [k for k in sys.modules if k == "src" or k.startswith("src.")]}
    try:
        from src.training.losses import PerceptualLoss, compute_losses          # noqa: F401
        from mvd_amd.perceptual import PerceptualLoss as Own
        assert PerceptualLoss is Own
    finally:
        sys.path.remove(p)
        for k in [k for k in sys.modules if k == "src" or k.startswith("src.")]:
            del sys.modules[k]
        sys.modules.update(saved)


# ------------------------------------------------------------------------------------------------ the C ABI on the host
def test_vgg_host_side_checks_and_dry_run():
    """argument validation and the sizing dry run need no GPU"""
    import ctypes as C
    from mvd_amd import _lib as L
    lib = L.lib()
    h = C.c_void_p()
    assert lib.mvd_vgg_create(C.byref(h)) == 0
    small, big = lib.mvd_vgg_workspace_bytes(h, 2, 32, 32), lib.mvd_vgg_workspace_bytes(h, 4, 64, 64)
    assert 0 < small < big
    # two ping-pong maps of images x h x w x 64 bf16 plus the fp32 partials of the largest split-K convolution
    assert 2 * 4 * 64 * 64 * 64 * 2 <= big < 6 * 4 * 64 * 64 * 64 * 2
    assert lib.mvd_vgg_workspace_bytes(h, 1, 15, 32) < 0 and b"16" in lib.mvd_last_error()
    assert lib.mvd_vgg_workspace_bytes(h, 1 << 20, 2048, 2048) < 0 and b"2^31" in lib.mvd_last_error()
    buf = (C.c_char * 4096)()
    addr = (C.addressof(buf) + 255) & ~255
    assert lib.mvd_vgg_bind_workspace(h, C.c_void_p(addr), 1024) == 0
    one = C.c_float()
    # no weights yet: the missing slot is reported before anything is launched
    assert lib.mvd_vgg_perceptual(h, C.c_void_p(addr), C.c_void_p(addr), 1, 32, 32, C.byref(one), None, None) == -10
    assert b"features.0.weight" in lib.mvd_last_error()
    w = (C.c_char * 64)()
    a16 = (C.addressof(w) + 15) & ~15
    assert lib.mvd_vgg_set_weight(h, b"features.0.weight", C.c_void_p(a16), 7, 1) == 0
    assert lib.mvd_vgg_perceptual(h, C.c_void_p(addr), C.c_void_p(addr), 1, 32, 32, C.byref(one), None, None) == -11
    assert lib.mvd_vgg_set_weight(h, b"features.0.weight", C.c_void_p(a16 + 4), 7, 1) < 0          # alignment
    assert lib.mvd_vgg_destroy(h) == 0
    assert lib.mvd_op_sqdiff_mean_ws_bytes(3, 4096 * 5 + 4) == 256 + 256            # 3 x 6 chunk sums of 8 bytes, rounded up
    assert lib.mvd_op_sqdiff_mean_ws_bytes(0, 16) < 0


# ------------------------------------------------------------------------------------------------ the synthetic inputs
@pytest.mark.parametrize("pairs,h,w", R.SHAPES)
def test_emulation_is_close_to_the_fp32_tower(pairs, h, w):
    """the condition the GPU tests rely on: bf16 storage moves the conv5_3 map by well under 1e-2 rel-L2 on these inputs, the
    map is neither dead nor exploding, and identical inputs give a loss of exactly 0"""
    c = R.case(pairs, h, w)
    print("shape", (pairs, h, w), "emulation rel-L2 per tap", c.emu, "rms conv5_3", R.rms(c.feat))
    assert c.feat.shape == (2 * pairs, 512, h // 16, w // 16)
    assert all(0.0 < e <= 1e-2 for e in c.emu.values()), c.emu
    assert 0.5 <= R.rms(c.feat) <= 4.0
    assert float(c.x.min()) >= -1.0 and float(c.x.max()) <= 1.0
    assert R.perceptual_loss(c.sd, c.x, c.x.clone()).item() == 0.0
    assert R.perceptual_loss(c.sd, c.x, c.y).item() > 0.0


def test_restatement_against_torchvision():
    """where torchvision imports: its own vgg16().features[:29] on the shared state dict"""
    tv = pytest.importorskip("torchvision")
    net = tv.models.vgg16(weights=None).features[:29].eval()
    sd = R.synthetic_state_dict()
    net.load_state_dict({k[len("features."):]: v for k, v in sd.items()})
    assert [type(m).__name__ for m in net] == [{"conv": "Conv2d", "relu": "ReLU", "pool": "MaxPool2d"}[k] for _, k in R.layer_table()]
    x = R.synthetic_images(2, 40, 56)
    with torch.no_grad():
        want = net(tv.transforms.Normalize(mean=list(R.MEAN), std=list(R.STD))((x + 1) / 2))
        got = R.features(sd, x)
    assert torch.allclose(got, want, rtol=1e-5, atol=1e-5)
