"""CPU-side checks of the FID row (N10): the BatchNorm fold, the packed weight layout of ``mvd_op_conv_relu_slice``, the layer
table, ``fid_from_statistics``, the sizing dry run, the weight-loading errors, the restatement of tests/fid_ref.py against
torchmetrics / torch-fidelity where those import, and the measurement behind ``FEAT_EMU_REL`` / ``FID_EMU_REL``."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

import fid_ref as R
from mvd_amd import packing as P
from mvd_amd._lib import MvdError


# ------------------------------------------------------------------------------------------------ fold, packing, table
def test_batchnorm_fold_matches_batch_norm_eval():
    g = torch.Generator().manual_seed(1)
    cin, cout = 12, 20
    w = torch.randn(cout, cin, 3, 3, generator=g)
    gamma, beta = 1 + 0.3 * torch.randn(cout, generator=g), 0.2 * torch.randn(cout, generator=g)
    mean, var = 0.3 * torch.randn(cout, generator=g), 0.5 + torch.rand(cout, generator=g)
    x = torch.randn(2, cin, 7, 6, generator=g).double()
    want = F.batch_norm(F.conv2d(x, w.double(), padding=1), mean.double(), var.double(), gamma.double(), beta.double(), training=False, eps=1e-3)
    wf, bf = P.fold_batchnorm(w, gamma, beta, mean, var)
    assert wf.dtype == torch.float32 and bf.dtype == torch.float32
    got = F.conv2d(x, wf.double(), bf.double(), padding=1)
    # the fold is rounded to fp32 once per factor: a few 2^-24 of the largest term
    assert float((got - want).abs().max()) <= 8 * 2.0 ** -24 * float(want.abs().max()) * math.sqrt(9 * cin)


def im2col(x, kh, kw, stride, ph, pw, pad_to, fill):
    """x (B, cin, H, W) -> rows (B oh ow, kh kw pad_to) with column (ky kw + kx) pad_to + c; columns c >= cin hold ``fill``"""
    B, cin, H, W = x.shape
    oh, ow = (H + 2 * ph - kh) // stride + 1, (W + 2 * pw - kw) // stride + 1
    xp = F.pad(x, (pw, pw, ph, ph))
    rows = torch.full((B, oh, ow, kh * kw, pad_to), float(fill), dtype=x.dtype)
    for ky in range(kh):
        for kx in range(kw):
            patch = xp[:, :, ky:ky + stride * (oh - 1) + 1:stride, kx:kx + stride * (ow - 1) + 1:stride]
            rows[:, :, :, ky * kw + kx, :cin] = patch.permute(0, 2, 3, 1)
    return rows.reshape(B * oh * ow, kh * kw * pad_to)


FORMS = sorted({(e[7], e[8], e[9], e[10], e[11]) for e in P.INCEPTION_FID_CONVS})


@pytest.mark.parametrize("cin", [32, 48, 80])
@pytest.mark.parametrize("form", FORMS, ids=lambda f: f"k{f[0]}x{f[1]}s{f[2]}p{f[3]}{f[4]}")
def test_packed_weights_times_im2col_is_the_convolution(form, cin):
    kh, kw, stride, ph, pw = form
    g = torch.Generator().manual_seed(cin + 7 * kh + 11 * kw)
    x = torch.randint(-3, 4, (2, cin, 9, 8), generator=g).double()
    w = torch.randint(-2, 3, (24, cin, kh, kw), generator=g).double()
    want = F.conv2d(x, w, stride=stride, padding=(ph, pw)).permute(0, 2, 3, 1).reshape(-1, 24)
    pad = P.fid_cin_pad(cin)
    assert pad % 32 == 0 and 0 <= pad - cin < 32 and (pad == cin) == (cin % 32 == 0)
    wp = P.pack_slice_conv(w)
    assert wp.shape == (24, kh * kw * pad) and wp.dtype == w.dtype
    # the rows carry 99 in the padded columns: the packed weights must be zero there
    assert torch.equal(im2col(x, kh, kw, stride, ph, pw, pad, 99) @ wp.t(), want)


def test_first_layer_packs_into_the_front_ends_channels():
    w = torch.randint(-2, 3, (32, 3, 3, 3)).double()
    wp = P.pack_slice_conv(w, P.FID_INPUT_CHANNELS).reshape(32, 9, 32)
    assert torch.equal(wp[:, :, :3], w.permute(0, 2, 3, 1).reshape(32, 9, 3)) and torch.count_nonzero(wp[:, :, 3:]) == 0


def test_layer_table():
    convs = P.INCEPTION_FID_CONVS
    assert len(convs) == 94 and len({e[1] for e in convs}) == 94
    hw, ch = P.fid_geometry(), P.fid_buffer_channels()
    sizes = {"Conv2d_1a": 149, "Conv2d_2a": 147, "Conv2d_2b": 147, "MaxPool_1": 73, "Conv2d_3b": 73, "Conv2d_4a": 71, "MaxPool_2": 35,
             "Mixed_5b": 35, "Mixed_5c": 35, "Mixed_5d": 35, "Mixed_6a": 17, "Mixed_6b": 17, "Mixed_6c": 17, "Mixed_6d": 17, "Mixed_6e": 17,
             "Mixed_7a": 8, "Mixed_7b": 8, "Mixed_7c": 8}
    for name, s in sizes.items():
        assert hw[name] == (s, s), (name, hw[name])
    chans = {"MaxPool_2": 192, "Mixed_5b": 256, "Mixed_5c": 288, "Mixed_5d": 288, "Mixed_6a": 768, "Mixed_6b": 768, "Mixed_6c": 768, "Mixed_6d": 768,
             "Mixed_6e": 768, "Mixed_7a": 1280, "Mixed_7b": 2048, "Mixed_7c": 2048}
    for name, c in chans.items():
        assert ch[name] == c, (name, ch[name])
    # every concatenation is written exactly once per channel, and every convolution reads all channels of its source
    cover = {}
    for e in P.INCEPTION_FID_LAYERS:
        dst, lo, n = e[3], e[4], (e[6] if e[0] == "conv" else e[5])
        cover.setdefault(dst, []).append((lo, lo + n))
        assert (e[5] if e[0] == "conv" else e[5]) == ch[e[2]], e
    for dst, spans in cover.items():
        spans.sort()
        assert spans[0][0] == 0 and spans[-1][1] == ch[dst] and all(a[1] == b[0] for a, b in zip(spans, spans[1:])), (dst, spans)
    assert {e[5] for e in convs} == {3, 32, 48, 64, 80, 96, 128, 160, 192, 256, 288, 384, 448, 768, 1280, 2048}
    assert P.fid_parameter_count() == sum(v.numel() for k, v in R.synthetic_inception_state_dict(0).items()
                                          if not k.startswith("fc.") and not k.endswith("num_batches_tracked")) == 21_820_000
    prog, bufs, names, final = P.fid_program()
    assert len(prog) == 13 * len(P.INCEPTION_FID_LAYERS) and len(names) == 94 and bufs[2 * final] == 2048 and bufs[2 * final + 1] == 1
    assert bufs[0] == P.FID_INPUT_CHANNELS and sum(bufs[1::2]) == 1


# ------------------------------------------------------------------------------------------------ fid_from_statistics
def spd(g, d, lo=0.5, hi=2.0):
    q, _ = torch.linalg.qr(torch.randn(d, d, generator=g, dtype=torch.float64))
    ev = lo + (hi - lo) * torch.rand(d, generator=g, dtype=torch.float64)
    return (q * ev) @ q.T


def test_fid_from_statistics_identical_and_diagonal():
    from mvd_amd.fid import fid_from_statistics
    g = torch.Generator().manual_seed(3)
    d = 64
    mu, s = torch.randn(d, generator=g, dtype=torch.float64), spd(g, d)
    assert abs(float(fid_from_statistics(mu, s, mu, s))) <= 1e-9 * float(s.trace())
    s1, s2 = 0.5 + torch.rand(d, generator=g, dtype=torch.float64), 0.5 + torch.rand(d, generator=g, dtype=torch.float64)
    mu2 = torch.randn(d, generator=g, dtype=torch.float64)
    want = float((mu - mu2).square().sum() + (s1.sqrt() - s2.sqrt()).square().sum())
    got = float(fid_from_statistics(mu, torch.diag(s1), mu2, torch.diag(s2)))
    assert abs(got - want) <= 1e-10 * want


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_fid_from_statistics_against_sqrtm_and_eigvals(seed):
    import scipy.linalg
    from mvd_amd.fid import fid_from_statistics
    g = torch.Generator().manual_seed(10 + seed)
    d = 64
    mu1, mu2 = torch.randn(d, generator=g, dtype=torch.float64), torch.randn(d, generator=g, dtype=torch.float64)
    s1, s2 = spd(g, d), spd(g, d, 0.2, 3.0)
    got = float(fid_from_statistics(mu1, s1, mu2, s2))
    root = scipy.linalg.sqrtm((s1 @ s2).numpy())
    want = float((mu1 - mu2).square().sum() + s1.trace() + s2.trace()) - 2.0 * float(root.trace().real)
    assert abs(got - want) <= 1e-8 * abs(want)
    tm = float(R.tm_compute_fid(mu1, s1, mu2, s2))
    assert abs(got - tm) <= 1e-8 * abs(tm)


def test_fid_from_statistics_rank_deficient():
    """rank 2 at d = 64 (three samples a side): finite, real, and equal to the value the features themselves give"""
    from mvd_amd.fid import fid_from_statistics
    g = torch.Generator().manual_seed(5)
    f1, f2 = torch.randn(3, 64, generator=g), 0.5 + 1.5 * torch.randn(3, 64, generator=g)
    (mu1, s1), (mu2, s2) = (R.tm_statistics(R.tm_update(R.new_state(64), f)) for f in (f1, f2))
    assert torch.linalg.matrix_rank(s1) == 2
    got = fid_from_statistics(mu1, s1, mu2, s2)
    assert got.dtype == torch.float64 and got.dim() == 0 and math.isfinite(float(got))
    want, _ = R.fid_of_features(f1, f2)
    assert abs(float(got) - want) <= 1e-9 * want
    with pytest.raises(ValueError):
        fid_from_statistics(mu1, s1, mu2[:32], s2)


# ------------------------------------------------------------------------------------------------ schedule (no GPU needed), errors
def test_workspace_query_is_monotone():
    from mvd_amd.fid import _FidHandle
    h = _FidHandle(8)
    sizes = [h.workspace_bytes(n) for n in range(1, 9)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])), sizes
    assert 8 << 20 < sizes[0] < 64 << 20, sizes[0]      # about 25 MiB of maps per image
    # beyond the pass size only the feature rows grow
    assert h.workspace_bytes(11) - sizes[7] == 3 * 2048 * 4
    small = _FidHandle(2)
    assert small.workspace_bytes(5) < sizes[2]
    from mvd_amd import _lib as L
    assert L.lib().mvd_fid_feature_dim(h.h) == 2048


def test_create_rejects_a_broken_program():
    import ctypes as C
    from mvd_amd import _lib as L
    prog, bufs, names, final = P.fid_program()
    bad = list(prog)
    bad[5] = 40      # cout of the first convolution: not a multiple of 16
    h = C.c_void_p()
    rc = L.lib().mvd_fid_create((C.c_int * len(bad))(*bad), len(bad) // 13, (C.c_int * len(bufs))(*bufs), len(bufs) // 2,
                                (C.c_char_p * len(names))(*[n.encode() for n in names]), len(names), final, 8, C.byref(h))
    assert rc != 0 and "op 0" in L.last_error()


def test_weight_sources_and_errors(tmp_path, monkeypatch):
    from mvd_amd import fid as FID
    with pytest.raises(MvdError, match="does not exist"):
        FID.load_inception_fid_weights(str(tmp_path / "nothing.pth"))
    monkeypatch.setenv("TORCH_HOME", str(tmp_path / "home"))
    monkeypatch.setenv("HOME", str(tmp_path / "nohome"))
    with pytest.raises(MvdError, match="Nothing is downloaded"):
        FID.load_inception_fid_weights(None)
    sd = dict(R.synthetic_inception_state_dict(0))
    ckpt = tmp_path / "home" / "hub" / "checkpoints"
    os.makedirs(ckpt)
    torch.save(sd, str(ckpt / FID.INCEPTION_FID_FILES[1]))
    got = P.normalize_inception_fid_keys(FID.load_inception_fid_weights(None))
    assert len(got) == 5 * 94 and not any(k.startswith("fc.") or k.endswith("num_batches_tracked") for k in got)
    assert torch.equal(got["Mixed_7c.branch_pool.conv.weight"], sd["Mixed_7c.branch_pool.conv.weight"])
    torch.save([1, 2, 3], str(tmp_path / "list.pth"))
    with pytest.raises(MvdError, match="not a state dict"):
        FID.load_inception_fid_weights(str(tmp_path / "list.pth"))
    missing = {k: v for k, v in sd.items() if k != "Mixed_6c.branch7x7_2.bn.running_var"}
    with pytest.raises(MvdError, match="Mixed_6c.branch7x7_2.bn.running_var' is missing"):
        P.normalize_inception_fid_keys(missing)
    wrong = dict(sd)
    wrong["Conv2d_1a_3x3.conv.weight"] = torch.zeros(32, 3, 5, 5)
    with pytest.raises(MvdError, match="expected \\(32, 3, 3, 3\\)"):
        P.normalize_inception_fid_keys(wrong)
    with pytest.raises(MvdError, match="expected a state dict"):
        P.normalize_inception_fid_keys([1, 2])
    prefixed = {"module." + k: v for k, v in sd.items()}
    assert len(P.normalize_inception_fid_keys(prefixed)) == 5 * 94


def test_protocol_arguments_without_a_gpu():
    from mvd_amd.fid import FrechetInceptionDistance
    sd = R.synthetic_inception_state_dict(0)
    for feature in (64, 192, 768, "2048", 2048.0):
        with pytest.raises(ValueError, match="only the 2048"):
            FrechetInceptionDistance(feature=feature, weights=sd)
    m = FrechetInceptionDistance(weights=sd, device="cpu")
    assert m.real_features_sum.dtype == torch.float64 and m.real_features_sum.shape == (2048,)
    assert m.fake_features_cov_sum.dtype == torch.float64 and m.fake_features_cov_sum.shape == (2048, 2048)
    assert m.real_features_num_samples.dtype == torch.long and m.fake_features_num_samples.dim() == 0
    with pytest.raises(RuntimeError, match="More than one sample"):
        m.compute()
    with pytest.raises(MvdError, match="GPU only"):
        m.update(torch.zeros(2, 3, 32, 32, dtype=torch.uint8), real=True)


# ------------------------------------------------------------------------------------------------ the restatement against the packages
def test_compute_against_torchmetrics():
    fid_mod = pytest.importorskip("torchmetrics.image.fid")
    from mvd_amd.fid import fid_from_statistics
    g = torch.Generator().manual_seed(21)
    mu1, mu2 = torch.randn(64, generator=g, dtype=torch.float64), torch.randn(64, generator=g, dtype=torch.float64)
    s1, s2 = spd(g, 64), spd(g, 64)
    want = float(fid_mod._compute_fid(mu1, s1, mu2, s2))
    assert abs(float(R.tm_compute_fid(mu1, s1, mu2, s2)) - want) <= 1e-12 * abs(want)
    assert abs(float(fid_from_statistics(mu1, s1, mu2, s2)) - want) <= 1e-8 * abs(want)


def test_tower_against_torch_fidelity(tmp_path):
    tf = pytest.importorskip("torch_fidelity.feature_extractor_inceptionv3")
    sd = R.synthetic_inception_state_dict(0)
    path = str(tmp_path / "inception.pth")
    torch.save(dict(sd), path)
    net = tf.FeatureExtractorInceptionV3("inception-v3-compat", ["2048"], feature_extractor_weights_path=path).eval()
    real, _ = R.test_images(0)
    with torch.no_grad():
        want = net(real[:2])[0].float()
    # the package keeps conv and BatchNorm apart and its weights in fp32; this restatement folds and rounds the weights to bf16
    plain = {e[1]: P.fold_batchnorm(*(sd[f"{e[1]}.{leaf}"] for leaf in ("conv.weight", "bn.weight", "bn.bias", "bn.running_mean", "bn.running_var")))
             for e in P.INCEPTION_FID_CONVS}
    got = torch.cat([R.tower(R.front_end(real[i:i + 1]), plain).mean((2, 3)) for i in range(2)])
    assert float((got - want).norm() / want.norm()) <= 1e-4


# ------------------------------------------------------------------------------------------------ the measurement behind the GPU bounds
def test_emulation_error_constants():
    """Seeds 0-2, four real and four fake 64 x 64 images each: the bf16 emulation against the fp32 tower at pool3 (per-image
    rel-L2) and in the FID.  The constants of fid_ref.py lie between the measured maximum and twice it."""
    feat, fid = 0.0, 0.0
    for seed in R.MEASURE_SEEDS:
        r32, f32 = R.reference_features(seed, False)
        rbf, fbf = R.reference_features(seed, True)
        for a, b in zip(torch.cat([rbf, fbf]), torch.cat([r32, f32])):
            feat = max(feat, float((a - b).norm() / b.norm()))
        want, _ = R.fid_of_features(r32, f32)
        got, _ = R.fid_of_features(rbf, fbf)
        assert want > 0.1, "the two sets are too close for a relative figure"
        fid = max(fid, abs(got - want) / want)
        print(f"seed {seed}: FID fp32 {want:.6f}, emulation {got:.6f}; running maxima: features {feat:.3e}, FID {fid:.3e}")
    assert feat <= R.FEAT_EMU_REL <= 2 * feat, (feat, R.FEAT_EMU_REL)
    assert fid <= R.FID_EMU_REL <= 2 * fid, (fid, R.FID_EMU_REL)
