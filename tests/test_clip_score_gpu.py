"""Row N7 on the GPU: the preprocessing kernels against recorded PIL / transformers output (byte for byte), the existing
flash attention at the ViT's token counts, ``CLIPVisionModelHIP`` (C ABI ``mvd_vision_encode``) against the fp32 CPU
restatement tests/clip_vision_ref.py on identical seeded weights, pooling / projection / cosine in isolation against fp64,
``CLIPScore`` end to end on a snapshot written without transformers, and the error paths.

Tolerances.  Preprocessing: the uint8 level exact, ``pixel_values`` within 1e-6 (the issue's figure; the arithmetic is
transformers' operation for operation).  Attention: what tests/test_ops_gpu.py holds ``mvd_op_attention`` to (max-abs <= 2^-6
max|ref|).  Encoder: rel-L2 <= 2e-2, the text tower's bound, because the restatement with every GEMM operand and weight rounded
to bf16 sits at 3.1e-3 .. 5.0e-3 on the CPU (tests/test_clip_score_cpu.py), under a third of it; cosines and scores follow at
|d cos| <= 2 x 2e-2.  Pool / project / cosine are fp32 kernels: 1e-5 against fp64.  Every test prints its figures before it
asserts; DESIGN.md section 9, row N7 records them."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import clip_vision_ref as V

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ("r40x56", "r56x40", "r17x23", "r32x32", "r64x64", "r5x7")
ENC_REL, COS_TOL = 2e-2, 2 * 2e-2


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "clip_preprocess_cases.npz")))


def _u8_level(pv, mean=V.CLIP_MEAN, std=V.CLIP_STD):
    m, s = np.array(mean, dtype=np.float64).reshape(3, 1, 1), np.array(std, dtype=np.float64).reshape(3, 1, 1)
    return np.rint((pv.astype(np.float64) * s + m) * 255).astype(np.int64)


# ------------------------------------------------------------------------------- preprocessing
@pytest.mark.parametrize("name", SMALL)
def test_preprocess_matches_recorded_processor_output(golden, name):
    """size = crop = 32 from 40x56 (B = 3, distinct images, x offset), 56x40 (y offset), 17x23 (upsampling), 32x32 (both passes
    skipped), 64x64, 5x7 (taps clipped at both borders)."""
    from mvd_amd.vision_encoder import CLIPImageProcessorLite
    proc = CLIPImageProcessorLite(size={"shortest_edge": 32}, crop_size={"height": 32, "width": 32})
    u8, want = torch.from_numpy(golden[name + "_in"]), golden[name + "_pv"]
    out = proc(images=u8.cuda(), return_tensors="pt", padding=True).to("cuda")
    got = out["pixel_values"].cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float32 and out.pixel_values is out["pixel_values"]
    bad = int((_u8_level(got) != _u8_level(want)).sum())
    err = float(np.abs(got - want).max())
    print(f"preprocess {name}: {bad} differing bytes of {want.size}, pixel_values max-abs {err:.3g}")
    assert bad == 0 and err <= 1e-6
    again = proc(images=list(u8.cuda()))["pixel_values"].cpu().numpy()         # a list of (3, H, W) tensors; tables already resident
    assert np.array_equal(again, got)


def test_preprocess_real_size_patch_rows_p14(golden):
    """96x64 -> shortest edge 224 -> 224 crop, P = 14: the uint8 crop equals PIL's, the patch rows the encoder will read are
    the bf16 rounding of the same values in (c, py, px) order with 52 zero pad columns (588 -> 640)."""
    from mvd_amd import _lib as L
    from mvd_amd.vision_encoder import CLIPVisionConfigLite, _VisionHandle
    cfg = CLIPVisionConfigLite(**dict(V.L14, num_hidden_layers=0))
    h = _VisionHandle(cfg)
    x = torch.from_numpy(golden["big_in"]).float().cuda()
    pv = h.preprocess(x, False, 224, 224, V.CLIP_MEAN, V.CLIP_STD, True, True)
    off = L.lib().mvd_vision_patch_rows_offset(h.h)
    assert off >= 0, L.last_error()
    rows = h.ws[off:off + 256 * 640 * 2].view(torch.bfloat16).view(256, 640).float().cpu()
    got = pv.cpu().numpy()
    bad = int((_u8_level(got) != golden["big_u8"].astype(np.int64)).sum())
    want_pv = V.normalize_u8(golden["big_u8"])
    print(f"preprocess 96x64 -> 224: {bad} differing bytes, pixel_values max-abs {np.abs(got - want_pv).max():.3g}")
    assert bad == 0 and np.abs(got - want_pv).max() <= 1e-6
    want_rows = V.patch_rows(torch.from_numpy(got), 14).to(torch.bfloat16).float()
    assert cfg.patch_k == 640 and torch.equal(rows[:, :588], want_rows) and not rows[:, 588:].any()
    # patch rows alone (no pixel_values), non-square source with a crop offset, P = 8: the same bytes
    h8 = _VisionHandle(CLIPVisionConfigLite(**V.TINY))
    x8 = torch.from_numpy(golden["r40x56_in"]).float().cuda()
    h8.preprocess(x8, False, 32, 32, V.CLIP_MEAN, V.CLIP_STD, True, False)
    off = L.lib().mvd_vision_patch_rows_offset(h8.h)
    rows8 = h8.ws[off:off + 3 * 16 * 192 * 2].view(torch.bfloat16).view(48, 192).float().cpu()
    assert torch.equal(rows8, V.patch_rows(torch.from_numpy(golden["r40x56_pv"]), 8).to(torch.bfloat16).float())


def test_preprocess_quantises_like_the_reference(golden):
    """[-1, 1] input with values on and next to every quantisation boundary (and outside the range): ((x.clamp(-1, 1) + 1) / 2
    * 255).to(uint8) exactly; then the same through a resize."""
    from mvd_amd.vision_encoder import CLIPVisionConfigLite, _VisionHandle
    h = _VisionHandle(CLIPVisionConfigLite(**V.TINY))
    q = torch.from_numpy(golden["quant_in"]).reshape(1, 3, 16, 16)
    pv = h.preprocess(q.cuda(), True, 16, 16, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), False, True).cpu().numpy()
    got = np.rint(pv.astype(np.float64) * 255).astype(np.int64)
    want = golden["quant_u8"].reshape(1, 3, 16, 16).astype(np.int64)
    print(f"quantisation: {int((got != want).sum())} differing bytes of {want.size}")
    assert np.array_equal(got, want)
    pv = h.preprocess(q.cuda(), True, 32, 32, V.CLIP_MEAN, V.CLIP_STD, False, True).cpu().numpy()
    assert np.array_equal(pv, V.preprocess(golden["quant_u8"].reshape(1, 3, 16, 16), 32, 32))


# ------------------------------------------------------------------------------- attention at the ViT's token counts
@pytest.mark.parametrize("B,heads", [(2, 2), (1, 16)])
@pytest.mark.parametrize("n", [5, 17, 50, 197, 257])
@pytest.mark.parametrize("peaked", [False, True])
def test_attention_prescaled_at_vit_token_counts(B, heads, n, peaked):
    """``mvd_op_attention`` in the engine form (q carries 64^-0.5 log2 e) with nq = nk = n odd, against fp32 softmax; the peaked
    case puts one large score in the last key tile (a late jump of the running max)."""
    import torch.nn.functional as F
    from mvd_amd import ops
    from mvd_amd.packing import QSCALE
    Cc = heads * 64
    g = torch.Generator().manual_seed(n * 10 + heads)
    qkv = torch.randn(B, n, 3 * Cc, generator=g).to(torch.bfloat16)
    if peaked:
        qkv[:, n - 1, Cc:2 * Cc] = (qkv[:, n - 1, Cc:2 * Cc].float() * 6).to(torch.bfloat16)
    qkv[..., :Cc] = (qkv[..., :Cc].float() * QSCALE).to(torch.bfloat16)
    sp = lambda t: t.float().view(B, n, heads, 64).transpose(1, 2)   # noqa: E731
    want = F.scaled_dot_product_attention(sp(qkv[..., :Cc]) * 0.6931471805599453, sp(qkv[..., Cc:2 * Cc]), sp(qkv[..., 2 * Cc:]), scale=1.0)
    want = want.transpose(1, 2).reshape(B, n, Cc)
    d = qkv.cuda()
    got = ops.attention(d[..., :Cc], d[..., Cc:2 * Cc], d[..., 2 * Cc:], heads, scale=0.0).float().cpu()
    err, ref = (got - want).abs().max().item(), want.abs().max().item()
    print(f"attention {B}x{heads} n={n} peaked={peaked}: max-abs {err:.4g} / max|ref| {ref:.4g} = {err / ref:.3g}")
    assert torch.isfinite(got).all() and err <= 2 ** -6 * ref + 1e-6


# ------------------------------------------------------------------------------- the encoder
_MODELS = {}
_CFGS = {"tiny": V.TINY, "p14": V.P14, "b32": V.B32, "l14": V.L14, "l14_full": V.L14_FULL}


def _model(kind):
    """(cfg, state dict, CLIPVisionModelHIP on the GPU), one per config and module."""
    if kind not in _MODELS:
        from mvd_amd.vision_encoder import CLIPVisionConfigLite, CLIPVisionModelHIP
        cfg = _CFGS[kind]
        sd = V.seeded_vision_state_dict(cfg, seed=3)
        m = CLIPVisionModelHIP(CLIPVisionConfigLite(**cfg))
        res = m.load_state_dict(sd)
        assert not res.missing_keys and not res.unexpected_keys
        _MODELS[kind] = (cfg, sd, m.to("cuda").eval())
    return _MODELS[kind]


@pytest.mark.parametrize("kind,B", [("tiny", 1), ("tiny", 3), ("p14", 2), ("b32", 2), ("l14", 2), ("l14_full", 1)])
def test_encoder_parity(kind, B):
    """17 tokens (B = 1, 3), 5 tokens with K padded 588 -> 640, ViT-B/32 geometry (50 tokens, 2 layers), ViT-L/14 geometry (257
    tokens: 4 layers at B = 2, all 24 layers at B = 1)."""
    cfg, sd, m = _model(kind)
    pv = V.seeded_pixel_values(cfg, B, seed=B)
    with torch.no_grad():
        want = V.vision_forward(sd, pv, cfg)
    m(pixel_values=pv.cuda())                                     # sizes and binds the workspace for this shape
    m._handle.ws.view(torch.float32).fill_(float("nan"))          # poison: nothing a kernel did not write may reach the result
    out = m(pixel_values=pv.cuda())
    assert out[0] is out.last_hidden_state and out[1] is out.image_embeds
    hid, raw, nrm = m.encode(pv.cuda(), want_hidden=True)
    assert torch.equal(hid, out[0]) and torch.equal(raw, out[1]) and torch.equal(m.get_image_features(pixel_values=pv.cuda()), raw)
    assert hid.shape == (B, V.num_tokens(cfg), cfg["hidden_size"]) and raw.shape == nrm.shape == (B, cfg["projection_dim"])
    rels = []
    for name, g, w in (("last_hidden_state", hid, want[0]), ("image_embeds", raw, want[1]), ("normalised", nrm, want[2])):
        g = g.cpu()
        assert g.dtype == torch.float32 and torch.isfinite(g).all(), name
        rels.append(V.rel_l2(g, w))
        print(f"vision encoder {kind} B={B} {name}: rel-L2 {rels[-1]:.3e}, max-abs / max|ref| {((g - w).abs().max() / w.abs().max()).item():.3e}")
    dcos = (1 - (nrm.cpu().double() * want[2].double()).sum(-1)).abs().max().item()
    print(f"vision encoder {kind} B={B}: |1 - cos(got, ref)| {dcos:.3e}; |norm - 1| {(nrm.norm(dim=-1) - 1).abs().max().item():.2e}")
    assert max(rels) <= ENC_REL and dcos <= COS_TOL, (kind, B, rels, dcos)
    assert (nrm.norm(dim=-1) - 1).abs().max().item() <= 1e-5


def test_encoder_rows_are_independent_and_deterministic():
    """Bidirectional attention mixes the tokens of one image only: changing image 1 of a batch leaves the rows of images 0 and
    2 bit-identical; two calls give the same bits."""
    cfg, sd, m = _model("tiny")
    a = V.seeded_pixel_values(cfg, 3, seed=7)
    b = a.clone()
    b[1] = V.seeded_pixel_values(cfg, 1, seed=8)[0]
    ha, ra, _ = m.encode(a.cuda(), want_hidden=True)
    hb, rb, _ = m.encode(b.cuda(), want_hidden=True)
    assert torch.equal(ha[0], hb[0]) and torch.equal(ha[2], hb[2]) and not torch.equal(ha[1], hb[1])
    assert torch.equal(ra[0], rb[0]) and not torch.equal(ra[1], rb[1])
    assert torch.equal(m.encode(a.cuda(), want_hidden=True)[0], ha)


# ------------------------------------------------------------------------------- pool / project / cosine
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("proj", [64, 768])
def test_pool_project_and_cosine_against_fp64(B, proj):
    import torch.nn.functional as F
    from mvd_amd.clip_score import clip_cosine, pool_project
    g = torch.Generator().manual_seed(B * 1000 + proj)
    T, H = 12, 1024 if proj == 768 else 128
    hid, dl = torch.randn(B, T, H, generator=g), 0.1 * torch.randn(B, T, H, generator=g)
    w = torch.randn(proj, H, generator=g) / H ** 0.5
    gam, bet = 1 + 0.2 * torch.randn(H, generator=g), 0.1 * torch.randn(H, generator=g)
    # image rule: token 0 of hidden + delta, LayerNorm, projection
    raw, nrm = pool_project(hid.cuda(), w.cuda(), delta=dl.cuda(), ln=(gam.cuda(), bet.cuda()))
    want = F.linear(F.layer_norm((hid + dl)[:, 0].double(), (H,), gam.double(), bet.double(), 1e-5), w.double())
    e1 = ((raw.cpu().double() - want).abs().max() / want.abs().max()).item()
    e2 = (nrm.cpu().double() - want / want.norm(dim=-1, keepdim=True)).abs().max().item()
    assert torch.equal(pool_project(hid.cuda(), w.cuda(), delta=dl.cuda(), ln=(gam.cuda(), bet.cuda()))[1], nrm)        # same bits
    # text rules: the argmax of the ids (eos 2), the first end token (eos 500), no end token at all (position 0)
    ids = torch.randint(3, 400, (B, T), generator=g)
    ids[:, 0] = 1
    for b in range(B):
        ids[b, 2 + b % 4], ids[b, 6 + b % 5] = 998, 500
        ids[b, 11] = 500                                             # a second end token behind the first
    errs = []
    for eos, rows in ((2, [2 + b % 4 for b in range(B)]), (500, [6 + b % 5 for b in range(B)]), (7000, [0] * B)):
        assert V.pooled_position(ids, eos).tolist() == rows
        r2, n2 = pool_project(hid.cuda(), w.cuda(), ids=ids.cuda(), eos_token_id=eos)
        w2 = F.linear(hid[torch.arange(B), rows].double(), w.double())
        errs.append(((r2.cpu().double() - w2).abs().max() / w2.abs().max()).item())
        errs.append((n2.cpu().double() - w2 / w2.norm(dim=-1, keepdim=True)).abs().max().item())
    # cosine of normalised rows and their mean
    other = F.normalize(torch.randn(B, proj, generator=g), dim=-1).cuda()
    rows_, mean = clip_cosine(nrm, other)
    wr = (nrm.cpu().double() * other.cpu().double()).sum(-1)
    e3, e4 = (rows_.cpu().double() - wr).abs().max().item(), abs(mean.item() - wr.mean().item())
    print(f"pool/project B={B} proj={proj}: image raw {e1:.2e} norm {e2:.2e}; text {max(errs):.2e}; cosine rows {e3:.2e} mean {e4:.2e}")
    assert max(e1, e2, e3, e4, *errs) <= 1e-5
    assert mean.dim() == 0 and rows_.shape == (B,)
    r2_, m2_ = clip_cosine(nrm, other)
    assert torch.equal(r2_, rows_) and torch.equal(m2_, mean)
    assert abs(clip_cosine(nrm, nrm)[1].item() - 1) <= 1e-6


# ------------------------------------------------------------------------------- CLIPScore end to end
PROMPTS = ["a photo of a red chair", "the front view of the chair", "the red chair"]


@pytest.fixture(scope="module")
def snapshot(tmp_path_factory):
    from mvd_amd.clip_score import CLIPScore
    from tests.clip_fixture import build_clip_snapshot
    snap, parts = build_clip_snapshot(tmp_path_factory.mktemp("clip"))
    return CLIPScore(snap).to("cuda"), parts, snap


def _ref_image_norm(parts, u8):
    pv = torch.from_numpy(V.preprocess(u8.numpy(), 32, 32))
    with torch.no_grad():
        return V.vision_forward(parts["vision"], pv, parts["vision_cfg"])[2]


def test_clip_score_call_update_compute(snapshot, tmp_path):
    from mvd_amd.clip_score import CLIPScore
    metric, parts, snap = snapshot
    g = torch.Generator().manual_seed(1)
    u8 = torch.randint(0, 256, (3, 3, 40, 56), generator=g, dtype=torch.uint8)
    ids = metric._ids(PROMPTS)
    with torch.no_grad():
        txt = V.text_embeds(parts["text"], ids, parts["text_cfg"], parts["text_projection"], parts["eos"])[1]
    want, want_mean = V.clip_scores(_ref_image_norm(parts, u8), txt)
    metric.reset()
    got = metric.scores(u8.cuda(), PROMPTS).cpu()
    print(f"CLIPScore per sample {got.tolist()} vs restatement {want.tolist()}: max |d| {(got - want).abs().max().item():.3g} (of 100)")
    assert (got - want).abs().max().item() <= 100 * COS_TOL
    batch = metric(u8.cuda(), PROMPTS)                                   # forward: this batch's value, and it enters the state
    assert batch.dim() == 0 and batch.is_cuda and abs(batch.item() - max(got.mean().item(), 0.0)) <= 1e-4
    metric.update(list(u8[:2].cuda()), PROMPTS[:2])                      # a list of images, a second update
    total = metric.compute()
    expect = max((got.sum().item() + got[:2].sum().item()) / 5, 0.0)
    print(f"CLIPScore update x2 + compute: {total.item():.5f} (expected {expect:.5f})")
    assert total.dim() == 0 and abs(total.item() - expect) <= 1e-4
    with pytest.raises(ValueError, match="images but"):
        metric.scores(u8.cuda(), PROMPTS[:2])
    # the clamp is on the mean: with text_projection negated every cosine changes sign, so one of the two means is negative
    from safetensors.torch import load_file, save_file
    from tests.clip_fixture import build_clip_snapshot
    snap2, _ = build_clip_snapshot(tmp_path)
    sd = load_file(os.path.join(snap2, "model.safetensors"))
    sd["text_projection.weight"] = -sd["text_projection.weight"]
    save_file(sd, os.path.join(snap2, "model.safetensors"))
    neg = CLIPScore(snap2).to("cuda")
    s2 = neg.scores(u8.cuda(), PROMPTS).cpu()
    assert (s2 + got).abs().max().item() <= 1e-4
    metric.reset()
    vals = []
    for mt, s in ((metric, got), (neg, s2)):
        mt.update(u8.cuda(), PROMPTS)
        vals.append(mt.compute().item())
        assert abs(vals[-1] - max(s.mean().item(), 0.0)) <= 1e-4
    print(f"CLIPScore clamp: means {got.mean().item():.4f} / {s2.mean().item():.4f} -> compute {vals}")
    assert min(vals) == 0.0 and min(got.mean().item(), s2.mean().item()) < 0
    metric.reset()
    with pytest.raises(Exception, match="before any update"):
        metric.compute()


class _Foreign:
    """Another library's metric object as validation._clip_score sees it: ``.to``, ``.model``, ``.processor`` only."""

    def __init__(self, metric):
        self.model, self.processor = metric.model, metric.processor

    def to(self, device):
        return self


def test_image_similarity_fused_and_generic_routes(snapshot):
    from mvd_amd import validation as VAL
    metric, parts, _ = snapshot
    g = torch.Generator().manual_seed(2)
    a = (torch.rand(3, 3, 40, 56, generator=g) * 2.4 - 1.2)             # beyond [-1, 1] on both sides: the clamp matters
    b = (a + 0.6 * torch.randn(a.shape, generator=g)).contiguous()
    same = metric.image_similarity(a.cuda(), a.cuda())
    assert same.dim() == 0 and same.is_cuda and abs(same.item() - 1) <= 1e-5
    got = metric.image_similarity(a.cuda(), b.cuda()).item()
    na, nb = _ref_image_norm(parts, V.quantize(a)), _ref_image_norm(parts, V.quantize(b))
    want = (na.double() * nb.double()).sum(-1).mean().item()
    zero = torch.zeros((), device="cuda")
    fused = VAL._clip_score(metric, a.cuda(), b.cuda(), torch.device("cuda"), zero).item()
    generic = VAL._clip_score(_Foreign(metric), a.cuda(), b.cuda(), torch.device("cuda"), zero).item()
    print(f"image_similarity: {got:.6f} vs restatement {want:.6f} (|d| {abs(got - want):.2e}); fused {fused:.7f} vs generic route {generic:.7f}")
    assert abs(got - want) <= COS_TOL and fused == got and abs(fused - generic) <= 1e-5
    assert VAL._clip_score(None, a.cuda(), b.cuda(), torch.device("cuda"), zero) is zero
    # no host synchronisation on the fused route once the weights are packed and the geometry's tables are resident
    ad, bd = a.cuda(), b.cuda()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = metric.image_similarity(ad, bd)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert again.item() == got


def test_compute_losses_fills_clip_score(snapshot):
    from types import SimpleNamespace
    from mvd_amd import validation as VAL
    from mvd_amd.scheduler import DDPMScheduler
    metric, parts, _ = snapshot

    class VAE:
        config = SimpleNamespace(scaling_factor=0.5)

        def decode(self, z):       # (B, 4, 8, 8) latents -> (B, 3, 24, 24) images in about [-1.3, 1.3]
            return SimpleNamespace(sample=torch.tanh(torch.nn.functional.interpolate(z[:, :3], scale_factor=3.0, mode="bilinear")) * 1.3)
    g = torch.Generator().manual_seed(3)
    B = 2
    lat = lambda: torch.randn(B, 4, 8, 8, generator=g).cuda()          # noqa: E731
    pred, noise, noisy, target = lat(), lat(), lat(), lat()
    sched = DDPMScheduler()
    ts = torch.tensor([10, 500]).cuda()
    got = VAL.compute_losses(pred, noise, noisy_latents=noisy, timesteps=ts, target_latents=target, vae=VAE(), scheduler=sched,
                             base_scheduler=sched, clip_score_metric_obj=metric)
    cs = got["clip_score"]
    assert cs.dim() == 0 and cs.is_cuda and -1 - 1e-5 <= cs.item() <= 1 + 1e-5 and cs.item() != 0.0
    # the same number by hand: the denoised and target images through image_similarity
    a, s = VAL.noise_tables(sched, pred.device)
    pt = sched.config.prediction_type
    at, st = a[ts].view(-1, 1, 1, 1), s[ts].view(-1, 1, 1, 1)
    den = (noisy - st * pred) / at if pt == "epsilon" else at * noisy - st * pred
    want = metric.image_similarity(VAE().decode(den / 0.5).sample, VAE().decode(target / 0.5).sample).item()
    print(f"compute_losses clip_score {cs.item():.6f} (by hand {want:.6f})")
    assert abs(cs.item() - want) <= 1e-4


# ------------------------------------------------------------------------------- error paths
def test_error_paths_launch_nothing():
    from mvd_amd import _lib as L
    from mvd_amd.vision_encoder import CLIPVisionModelHIP
    cfg, sd, m = _model("tiny")
    pv = V.seeded_pixel_values(cfg, 1, seed=1).cuda()
    m(pixel_values=pv)                                                  # (packs and registers the weights)
    with pytest.raises(L.MvdError, match="pixel_values must be"):
        m(pixel_values=torch.zeros(1, 3, 16, 16, device="cuda"))
    lib = L.lib()
    c = L.mvd_vision_config_t()
    c.image_size, c.patch_size, c.hidden_size, c.intermediate_size, c.num_layers, c.num_heads, c.projection_dim = 32, 8, 128, 256, 2, 2, 64
    c.layer_norm_eps, c.act = 1e-5, 1
    h = C.c_void_p()
    L.call("mvd_vision_create", C.byref(c), C.byref(h))
    sent = torch.full((1, 64), 123.0, device="cuda")
    sent_pv = torch.full((1, 3, 32, 32), 123.0, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())                              # noqa: E731
    enc = (h, p(pv), 1, None, p(sent), None, None)
    assert lib.mvd_vision_encode(*enc) < 0 and "missing weight slot" in L.last_error()
    for slot, t in m._packed.items():
        L.call("mvd_vision_set_weight", h, slot.encode(), p(t), t.numel(), 0 if t.dtype == torch.float32 else 1)
    assert lib.mvd_vision_encode(*enc) < 0 and "workspace not bound" in L.last_error()
    img = torch.rand(1, 3, 5, 7, device="cuda")
    three = (C.c_float * 3)(0.5, 0.5, 0.5)
    pre = lambda b, hh, ww: lib.mvd_vision_preprocess(h, p(img), b, hh, ww, 1, 32, 32, three, three, 1, p(sent_pv), None)   # noqa: E731
    assert pre(1, 5, 7) < 0 and "workspace not bound" in L.last_error()
    ws = torch.empty(4096, dtype=torch.uint8, device="cuda")
    L.call("mvd_vision_bind_workspace", h, p(ws), ws.numel())
    assert lib.mvd_vision_encode(*enc) < 0 and "workspace too small" in L.last_error()
    assert pre(1, 5, 7) < 0 and "workspace too small" in L.last_error()
    assert pre(1, 0, 7) < 0 and "image size" in L.last_error()
    assert pre(1, 5, 0) < 0 and "image size" in L.last_error()
    assert pre(0, 5, 7) < 0 and "batch" in L.last_error()
    assert lib.mvd_vision_encode(h, p(pv), 0, None, p(sent), None, None) < 0 and "batch" in L.last_error()
    need = lib.mvd_vision_workspace_bytes(h, 1, 5, 7, 32)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    L.call("mvd_vision_bind_workspace", h, p(ws), ws.numel())
    assert lib.mvd_vision_encode(h, None, 1, None, p(sent), None, None) < 0 and "patch rows" in L.last_error()   # nothing preprocessed yet
    torch.cuda.synchronize()
    assert bool((sent == 123.0).all()) and bool((sent_pv == 123.0).all())          # nothing was written
    # and the raw ABI agrees with the module bit for bit
    L.call("mvd_vision_encode", *enc)
    torch.cuda.synchronize()
    assert torch.equal(sent, m.get_image_features(pixel_values=pv))
    lib.mvd_vision_destroy(h)
    with pytest.raises(L.MvdError, match="head dimension"):
        from mvd_amd.vision_encoder import CLIPVisionConfigLite
        CLIPVisionModelHIP(CLIPVisionConfigLite(**dict(cfg, hidden_size=160)))
