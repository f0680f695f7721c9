"""KID and the Inception score (row N11) without a GPU: the exactness of the integer test inputs, the host logic (subset draws,
chunk bounds, argument errors, the fc-weight lookup, the exported symbols), the restatements of tests/kid_ref.py against
torchmetrics where it imports, and the measurement behind ``KID_EMU_REL``."""
import ctypes as C
import random

import pytest
import torch

import fid_ref as R
import kid_ref as K
from mvd_amd import _lib as L
from mvd_amd import packing as P
from mvd_amd._lib import MvdError


# ------------------------------------------------------------------------------------------------ the integer inputs are exact
def test_integer_inputs_are_exact():
    """features over {-1, 0, 1} with at most 255 non-zeros a row, d = 2048, gamma = 2^-11, coef 1, degree 3: every kernel value
    is (dot + 2048)^3 / 2^33 and every sum over m^2 <= 130^2 of them is below 2^51, so fp64 adds them exactly in any order"""
    m, d = 130, 2048
    x, y = K.integer_features(m, d, 0), K.integer_features(m, d, 1)
    assert int(x.abs().sum(1).max()) <= 255 and set(x.unique().tolist()) <= {-1.0, 0.0, 1.0}
    dots = torch.cat([(x.long() @ x.long().T).flatten(), (x.long() @ y.long().T).flatten(), (y.long() @ y.long().T).flatten()])
    assert int(dots.abs().max()) <= 255
    nxx, nyy, nxy = K.exact_sums(x, y, 3)
    assert max(nxx, nyy, nxy) < 2 ** 51      # the numerators of the sums (over 2^33): integers fp64 holds exactly, as is every partial sum
    assert (255 + d) ** 3 < 2 ** 53      # a kernel value's numerator is an fp64 integer
    k_xx, k_xy = K.poly_kernel(x.double(), x.double(), 3, 2.0 ** -11, 1.0), K.poly_kernel(x.double(), y.double(), 3, 2.0 ** -11, 1.0)
    off = k_xx[~torch.eye(m, dtype=torch.bool)].tolist()
    full = k_xy.flatten().tolist()
    rng = random.Random(0)
    for _ in range(3):
        rng.shuffle(off)
        rng.shuffle(full)
        s_off, s_full = 0.0, 0.0
        for v in off:
            s_off += v
        for v in full:
            s_full += v
        assert s_off * 2 ** 33 == nxx and s_full * 2 ** 33 == nxy
    sxx, syy, sxy, _ = K.mmd_terms(x, y, 3, 2.0 ** -11, 1.0)
    assert (sxx, syy, sxy) == (nxx / 2 ** 33, nyy / 2 ** 33, nxy / 2 ** 33)


# ------------------------------------------------------------------------------------------------ host logic
def test_kid_subsets_are_torchmetrics_draws():
    from mvd_amd.kid import kid_subsets
    torch.manual_seed(11)
    got = kid_subsets(9, 7, 5, 4)
    torch.manual_seed(11)
    want = K.draw_subsets(9, 7, 5, 4)
    assert got.dtype == torch.int32 and got.shape == (5, 2, 4)
    for s, (a, b) in enumerate(want):
        assert torch.equal(got[s, 0].long(), a) and torch.equal(got[s, 1].long(), b)
    assert int(got[:, 0].max()) < 9 and int(got[:, 1].max()) < 7 and int(got.min()) >= 0
    with pytest.raises(ValueError, match="should be smaller than the number of samples"):
        kid_subsets(9, 3, 2, 4)
    with pytest.raises(ValueError, match="should be smaller than the number of samples"):
        kid_subsets(3, 9, 2, 4)
    with pytest.raises(ValueError, match="at least 2"):
        kid_subsets(9, 9, 2, 1)


@pytest.mark.parametrize("splits", [1, 3, 10])
@pytest.mark.parametrize("n", [1, 9, 10, 11, 25, 130])
def test_chunk_bounds_are_torch_chunk(n, splits):
    from mvd_amd.kid import chunk_bounds
    want = [(int(c[0]), int(c[-1]) + 1) for c in torch.arange(n).chunk(splits)]
    assert chunk_bounds(n, splits) == want


def test_constructor_and_compute_errors():
    from mvd_amd.kid import InceptionScore, KernelInceptionDistance
    sd = K.synthetic_inception_state_dict(0)
    for feature in (64, 192, 768, "2048", 2048.0):
        with pytest.raises(ValueError, match="only the 2048"):
            KernelInceptionDistance(feature=feature, weights=sd)
    for kw, msg in ((dict(subsets=0), "`subsets`"), (dict(subsets=1.5), "`subsets`"), (dict(subset_size=0), "`subset_size`"),
                    (dict(subset_size=True), "`subset_size`"), (dict(degree=0), "`degree`"), (dict(gamma=0.0), "`gamma`"), (dict(gamma=1), "`gamma`"),
                    (dict(coef=0.0), "`coef`"), (dict(coef=1), "`coef`"), (dict(reset_real_features=1), "`reset_real_features`"),
                    (dict(normalize=0), "`normalize`"), (dict(inception="net"), "InceptionV3FeaturesHIP")):
        with pytest.raises(ValueError, match=msg):
            KernelInceptionDistance(weights=sd, **kw)
    m = KernelInceptionDistance(weights=sd, subsets=2, subset_size=3, device="cpu")
    assert m.real_features == [] and m.fake_features == [] and m.gamma is None and m.coef == 1.0 and m.degree == 3
    with pytest.raises(ValueError, match="should be smaller than the number of samples"):
        m.compute()
    with pytest.raises(MvdError, match="GPU only"):
        m.update(torch.zeros(2, 3, 32, 32, dtype=torch.uint8), real=True)
    with pytest.raises(MvdError, match="GPU only"):
        m.update_features(torch.zeros(2, 2048), real=True)
    for kw, msg in ((dict(feature="logits"), "only 'logits_unbiased'"), (dict(feature=2048), "only 'logits_unbiased'"), (dict(splits=0), "`splits`"),
                    (dict(normalize=1), "`normalize`")):
        with pytest.raises(ValueError, match=msg):
            InceptionScore(weights=sd, **kw)
    s = InceptionScore(weights=sd, device="cpu")
    assert s.features == [] and s.splits == 10
    with pytest.raises(ValueError, match="no samples"):
        s.compute()
    with pytest.raises(MvdError, match="GPU only"):
        s.update(torch.zeros(2, 3, 32, 32, dtype=torch.uint8))
    with pytest.raises(MvdError, match="GPU only"):
        s.update_features(torch.zeros(2, 2048))


def test_fc_weight_lookup():
    from mvd_amd.fid import FrechetInceptionDistance, InceptionV3FeaturesHIP
    from mvd_amd.kid import InceptionScore, KernelInceptionDistance
    sd = K.synthetic_inception_state_dict(0)
    w = P.inception_fc_weight(sd)
    assert w.shape == P.INCEPTION_FC_SHAPE == (1008, 2048) and w.dtype == torch.float32 and w.is_contiguous() and torch.equal(w, sd["fc.weight"])
    for prefix in ("module.", "model.", "inception.", "base.", "module.model."):
        assert torch.equal(P.inception_fc_weight({prefix + k: v for k, v in sd.items()}), w)
    assert torch.equal(P.inception_fc_weight({"fc.weight": sd["fc.weight"].double()}), w.double().float())
    bare = {k: v for k, v in sd.items() if k != "fc.weight"}
    with pytest.raises(MvdError, match="'fc.weight' is missing"):
        P.inception_fc_weight(bare)
    assert P.inception_fc_weight(bare, required=False) is None
    for bad in (torch.zeros(1000, 2048), torch.zeros(2048, 1008), torch.zeros(1008)):
        with pytest.raises(MvdError, match="'fc.weight' has shape"):
            P.inception_fc_weight({**bare, "fc.weight": bad}, required=False)
    with pytest.raises(MvdError, match="expected a state dict"):
        P.inception_fc_weight([1, 2])
    assert len(P.normalize_inception_fid_keys(sd)) == 5 * 94      # the tower's lookup is what it was
    # the tower keeps the weight when there is one; FID and KID never need it, the Inception score does
    assert torch.equal(InceptionV3FeaturesHIP(sd).fc_weight, w)
    net = InceptionV3FeaturesHIP(bare)
    assert net.fc_weight is None
    FrechetInceptionDistance(weights=bare, device="cpu")
    KernelInceptionDistance(weights=bare, device="cpu")
    assert FrechetInceptionDistance(inception=net, device="cpu").inception is net
    assert KernelInceptionDistance(inception=net, device="cpu").inception is net
    with pytest.raises(MvdError, match="no 'fc.weight'"):
        InceptionScore(weights=bare, device="cpu")
    with pytest.raises(MvdError, match="no 'fc.weight'"):
        InceptionScore(inception=net, device="cpu")
    with pytest.raises(ValueError, match="InceptionV3FeaturesHIP"):
        FrechetInceptionDistance(inception=object(), device="cpu")


def test_symbols_and_host_checks():
    """the five entry points are exported, and every argument error is reported on the host (no GPU is needed to get one)"""
    lib = L.lib()
    for name in ("mvd_op_kid_workspace_bytes", "mvd_op_kid_mmd", "mvd_op_fc_logits", "mvd_op_inception_score_workspace_bytes",
                 "mvd_op_inception_score"):
        assert hasattr(lib, name) and name in L.EXPORTED_SYMBOLS
    # 64 x 64 tiles: xx and yy keep the upper triangle, xy every tile; one fp64 partial each, rounded up to 256 bytes
    for m, tiles in ((2, 3), (64, 3), (65, 10), (130, 21), (1000, 2 * 136 + 256)):
        assert lib.mvd_op_kid_workspace_bytes(1, m) == -(-tiles * 8 // 256) * 256
        assert lib.mvd_op_kid_workspace_bytes(100, m) == -(-100 * tiles * 8 // 256) * 256
    assert lib.mvd_op_kid_workspace_bytes(1, 1) < 0 and "m >= 2" in L.last_error()
    assert lib.mvd_op_kid_workspace_bytes(0, 5) < 0
    p = C.c_void_p(4096)      # aligned, never dereferenced: every call below fails its host checks
    mmd = lambda **k: lib.mvd_op_kid_mmd(k.get("f", p), k.get("nr", 8), p, k.get("nf", 8), k.get("d", 64), p, 1, k.get("m", 4), k.get("deg", 3), 1.0, 1.0,      # noqa: E731
                                         p, k.get("ws", 1 << 20), None, p, None)
    assert mmd(m=1) == -1 and "m <=" in L.last_error()
    assert mmd(m=9) == -1 and mmd(nf=3) == -1 and mmd(nr=3) == -1
    assert mmd(d=96) == -1 and "multiple of 64" in L.last_error()
    assert mmd(deg=0) == -1 and "degree" in L.last_error()
    assert mmd(f=C.c_void_p(4100)) == -1 and "misaligned" in L.last_error()
    assert mmd(ws=8) == -4 and "workspace" in L.last_error()
    assert mmd(f=None) == -1
    assert lib.mvd_op_fc_logits(p, 1, 66, p, 16, p, None) == -1 and "multiple of 4" in L.last_error()
    assert lib.mvd_op_fc_logits(p, 0, 64, p, 16, p, None) == -1
    ws = lib.mvd_op_inception_score_workspace_bytes(25, 1008, 10)
    assert ws >= (25 + 9 * 1008 + 25) * 8      # lse, log mean_p of the 9 chunks torch.chunk(10) makes of 25 rows, kl
    assert lib.mvd_op_inception_score_workspace_bytes(0, 1008, 10) < 0 and lib.mvd_op_inception_score_workspace_bytes(5, 1008, 0) < 0
    assert lib.mvd_op_inception_score(p, 25, 1008, p, 10, p, 8, p, None, None) == -4 and "workspace" in L.last_error()
    assert lib.mvd_op_inception_score(p, 25, 1008, p, 0, p, 1 << 20, p, None, None) == -1


# ------------------------------------------------------------------------------------------------ the restatements against the package
def test_poly_mmd_against_torchmetrics():
    kid_mod = pytest.importorskip("torchmetrics.image.kid")
    x, y = K.gaussian_like_features(17, 256, 0).double(), K.gaussian_like_features(17, 256, 1).double()
    for degree, gamma, coef in ((3, None, 1.0), (2, 0.01, 0.5), (1, None, 2.0)):
        want = kid_mod.poly_mmd(x, y, degree, gamma, coef)
        assert torch.equal(K.poly_mmd(x, y, degree, gamma, coef), want)
        sxx, syy, sxy, _ = K.mmd_terms(x, y, degree, gamma, coef)
        assert abs((sxx + syy) / (17 * 16) - 2 * sxy / 17 ** 2 - float(want)) <= 1e-12 * abs(float(want)) + 1e-15


def test_inception_score_against_torchmetrics():
    inc = pytest.importorskip("torchmetrics.image.inception")
    g = torch.Generator().manual_seed(3)
    logits = (3.0 * torch.randn(25, K.CLASSES, generator=g)).double()

    class Identity(torch.nn.Module):
        def forward(self, x):
            return x
    for splits in (1, 3, 10):
        metric = inc.InceptionScore(feature=Identity(), splits=splits)
        metric.features.append(logits)
        torch.manual_seed(5)
        mean, std = metric.compute()
        torch.manual_seed(5)
        kl = K.inception_score_chunks(logits, torch.randperm(25), splits)
        assert torch.equal(kl.mean(), mean) and (torch.equal(kl.std(), std) or (torch.isnan(std) and splits == 1))


# ------------------------------------------------------------------------------------------------ the measurement behind the GPU bound
def test_emulation_error_constant():
    """Seeds 0-2, four real and four fake 64 x 64 images each, subset_size 3, 4 subsets: per subset |KID_emu - KID_fp32| / T for
    the bf16 emulation of the tower against the fp32 tower.  ``KID_EMU_REL`` lies between the measured maximum and twice it."""
    worst = 0.0
    m, subsets = K.MEASURE["subset_size"], K.MEASURE["subsets"]
    for seed in R.MEASURE_SEEDS:
        r32, f32 = R.reference_features(seed, False)
        rbf, fbf = R.reference_features(seed, True)
        torch.manual_seed(seed)
        draws = K.draw_subsets(4, 4, subsets, m)
        v32, scales = K.kid_scores(r32, f32, subsets, m, draws=draws)
        vbf, _ = K.kid_scores(rbf, fbf, subsets, m, draws=draws)
        for a, b, t in zip(vbf.tolist(), v32.tolist(), scales):
            worst = max(worst, abs(a - b) / t)
        print(f"seed {seed}: KID fp32 {float(v32.mean()):.6e}, emulation {float(vbf.mean()):.6e}, T {sum(scales) / subsets:.4f}; running maximum {worst:.3e}")
    assert worst <= K.KID_EMU_REL <= 2 * worst, (worst, K.KID_EMU_REL)
