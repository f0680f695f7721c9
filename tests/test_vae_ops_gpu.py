"""Operator-level parity of the SD-2.1 VAE's kernels at the VAE's own shapes, 512x512 and 768x768 (the reference's infer.py
decodes at 768x768).  test_vae_gpu.py checks encode / decode end to end (rel-L2 2e-2); here each kernel meets a plain reference
of the same operation on the same bf16-rounded operands: fp32 torch on the GPU, fp64 where the kernel is fp32 throughout.
Every GEMM / conv goes through the heuristic (force_cfg = -1) with the split-K factor the VAE's own launches take.

Tolerances (each test states its own): bf16 outputs use test_cfg4_shapes_gpu.close() -- |err| <= 2^-7 * max|ref| and
rel-L2 <= 6e-3 (bf16 storage, fp32 accumulate); fp32 outputs 1e-4 * max|ref|.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from tests.branch_check import branch_close
from tests.test_cfg4_shapes_gpu import close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mvd_amd import ops as O
    return O


def grnd(*shape, scale=1.0, seed=0, dtype=torch.bfloat16):
    g = torch.Generator(device="cuda").manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g, device="cuda") * scale).to(dtype)


def conv3_ref(x, w, b, stride=1, ups=False, asym=False):
    """3x3 convolution in fp32 as nine shifted matmuls (NHWC): x (B, H, W, Ci), w (Co, Ci, 3, 3) -> (B, OH, OW, Co).
    pad 1, or (asym, stride 2) zero padding on the bottom / right edge only (Downsample2D(padding=0)); ups: nearest 2x first."""
    x = x.float()
    if ups:
        x = x.repeat_interleave(2, 1).repeat_interleave(2, 2)
    xp = F.pad(x, (0, 0, 0, 1, 0, 1)) if asym else F.pad(x, (0, 0, 1, 1, 1, 1))
    B, Hp, Wp, _ = xp.shape
    oh, ow = (Hp - 3) // stride + 1, (Wp - 3) // stride + 1
    out = b.float().expand(B, oh, ow, w.shape[0]).clone()
    for dy in range(3):
        for dx in range(3):
            xs = xp[:, dy:dy + stride * (oh - 1) + 1:stride, dx:dx + stride * (ow - 1) + 1:stride, :]
            out += xs @ w[:, :, dy, dx].float().T
    return out


# ------------------------------------------------------------------------------- 1. the attention's row softmax
def _softmax_rows(n, seed):
    """Rows of the kinds a softmax gets wrong: random, all near -1e4 (exp underflows without the max), all near +80 (the sum
    overflows fp32 without it: 9216 * e^80 > 3.4e38), one dominant entry, the max in the last element."""
    g = torch.Generator(device="cuda").manual_seed(seed + n)
    r = lambda: torch.randn(n, generator=g, device="cuda", dtype=torch.float32)   # noqa: E731
    rows = [4.0 * r(), 4.0 * r(), -1.0e4 + r(), 80.0 + r()]
    dom = r()
    dom[(7 * n) // 11] = 200.0                                   # every other entry exp(< -190): 0 in fp32
    rows.append(dom)
    last = 4.0 * r()
    last[-1] = last.max() + 1.0
    rows.append(last)
    return torch.stack(rows).contiguous()


@pytest.mark.parametrize("n", [1, 64, 257, 1000, 4096, 9216])
def test_softmax_rows(ops, n):
    """softmax_rows_kernel (fp32 scores -> bf16 probabilities, one workgroup per row) against the fp64 softmax of the same fp32
    scores, element by element: |p - ref| <= (2^-8 + 2^-14) * ref + 1e-30.  2^-8 * ref is bf16's half-ulp (correct rounding of
    the fp32 value); 2^-14 (~250 fp32 ulps) covers __expf of arguments down to ~-40 and the fp32 row sum; 1e-30 is the floor below
    which the fp32 exponential may flush.  The dominant-entry row must come out exactly 1 and 0, and the kernel's value at the
    reference argmax must be its row maximum (bf16 may tie the top two)."""
    s = _softmax_rows(n, 5)
    p = ops.softmax_rows(s)
    torch.cuda.synchronize()
    ref = torch.softmax(s.double(), dim=-1)
    pd = p.double()
    assert torch.isfinite(pd).all()
    err = (pd - ref).abs()
    bound = (2 ** -8 + 2 ** -14) * ref + 1e-30
    worst = (err / bound).max().item()
    assert worst <= 1.0, f"n={n}: worst |p - ref| / bound = {worst:.3g}"
    dom = pd[4]
    k = (7 * n) // 11
    assert dom[k].item() == 1.0 and (dom[torch.arange(n, device="cuda") != k] == 0).all(), "dominant row not exactly one-hot"
    am = ref.argmax(dim=-1)
    assert torch.equal(pd.gather(1, am[:, None])[:, 0], pd.max(dim=-1).values), "argmax of the reference is not the kernel's max"
    if n > 1:
        assert pd[5, -1].item() == pd[5].max().item()
    print(f"softmax n={n}: worst err / bound {worst:.3f}")


# ------------------------------------------------------------------------------- 2. the mid-block attention block
QK_SCALE = 2.1        # q and k weights x 2.1: score std ~ 2.1^2 = 4.4 (a peaked softmax; asserted from the reference below)
OUT_SCALE = 2.0       # the out-projection x 2: branch rms ~ rms(x) (asserted >= 1/3)


@pytest.fixture(scope="module")
def sd21_vae(ops):
    """The SD-2.1 VAE on seeded weights; both mid-block attentions re-scaled as above, their q / k / v / out matrices rounded to
    bf16 in the state dict itself, so that the engine and the reference multiply by the same numbers."""
    from mvd_amd.vae import AutoencoderKLHIP, VAEConfig
    from oracle import vae as OV
    ocfg = OV.VAEConfig.sd21()
    p = OV.init_params(ocfg, 4)
    for coder in ("encoder", "decoder"):
        a = f"{coder}.mid_block.attentions.0"
        for nm, sc in (("to_q", QK_SCALE), ("to_k", QK_SCALE), ("to_v", 1.0), ("to_out.0", OUT_SCALE)):
            p[f"{a}.{nm}.weight"] = (p[f"{a}.{nm}.weight"] * sc).to(torch.bfloat16).float()
    m = AutoencoderKLHIP(VAEConfig(block_out_channels=ocfg.block_out_channels, layers_per_block=ocfg.layers_per_block))
    m.load_state_dict(p, strict=True)
    return ocfg, p, m.to("cuda").eval()


def _attn_params(p, coder):
    a = f"{coder}.mid_block.attentions.0"
    return {k: v.cuda() for k, v in p.items() if k.startswith(a + ".")}, a


@pytest.mark.parametrize("coder", ["encoder", "decoder"])
@pytest.mark.parametrize("batch,h,w", [(1, 8, 8), (2, 8, 8), (1, 64, 64), (2, 64, 64), (1, 96, 96), (2, 96, 96)])
def test_mid_attention_block(sd21_vae, coder, batch, h, w):
    """One mid-block attention (C = 512) through mvd_vae_mid_attention -- VCtx::attention, the code encode / decode run: GroupNorm,
    q / k, V^T = W_v . x^T, S = q.k^T / sqrt(C) in fp32, row softmax, P.V + b_v, out-projection + residual -- at 64, 4096 (512x512)
    and 9216 (768x768) positions, against oracle/vae.py's _attention in fp32 on the GPU on the same bf16 input.
    The softmax is peaked (median row entropy <= log(hw) / 2, asserted) and the branch is at least a third of x (rms, asserted),
    so a wrong scale, a dropped tail or a bad tile changes the result.  The BRANCH out - x is compared (tests/branch_check.py):
    || out - ref || <= 1e-2 * || ref - x || + 1.25 * || bf16(ref) - ref ||.  1e-2: the engine stores xn, q, k, V^T, P and the
    attention output in bf16 (~1e-3 rms each), and the rounding of xn, q and k moves the logits by ~2^-9 of their spread (4.4):
    ~1e-2 on single probabilities, ~6e-3 measured on the branch; the second term is the bf16 rounding of out itself."""
    from oracle import vae as OV
    ocfg, p, m = sd21_vae
    pa, key = _attn_params(p, coder)
    C, hw = 512, h * w
    g = torch.Generator(device="cuda").manual_seed(batch * 1000 + hw + (coder == "decoder"))
    off = 0.5 * torch.randn(C, generator=g, device="cuda")
    x = (torch.randn(batch, h, w, C, generator=g, device="cuda") + off).to(torch.bfloat16)
    out = m.mid_attention(x, decoder=coder == "decoder")
    xr = x.float().permute(0, 3, 1, 2).contiguous()
    ref = OV._attention(pa, key, xr, ocfg).permute(0, 2, 3, 1)
    # the regime: peaked softmax rows, a branch that is not small against x
    hn = F.group_norm(xr.view(batch, C, hw), ocfg.norm_num_groups, pa[f"{key}.group_norm.weight"], pa[f"{key}.group_norm.bias"],
                      ocfg.norm_eps).transpose(1, 2)
    q = F.linear(hn, pa[f"{key}.to_q.weight"], pa[f"{key}.to_q.bias"])
    k = F.linear(hn, pa[f"{key}.to_k.weight"], pa[f"{key}.to_k.bias"])
    lp = torch.log_softmax(q @ k.transpose(1, 2) / math.sqrt(C), dim=-1)
    ent = -(lp.exp() * lp).sum(-1).median().item()
    del q, k, lp
    assert ent <= 0.5 * math.log(hw), f"softmax not peaked: median row entropy {ent:.3g} vs log(hw) {math.log(hw):.3g}"
    xf = x.float()
    ratio = ((ref - xf).pow(2).mean().sqrt() / xf.pow(2).mean().sqrt()).item()
    assert ratio >= 1 / 3, f"branch rms / x rms = {ratio:.3g}"
    err, bound = branch_close(out, ref, xf, what=f"{coder} attention B={batch} hw={hw}")
    print(f"{coder} B={batch} hw={hw}: entropy {ent:.2f} / log(hw) {math.log(hw):.2f}, branch/x {ratio:.2f}, "
          f"branch err {err:.4f} <= {bound:.4f}")


def test_mid_attention_refuses_ragged_positions(sd21_vae):
    """hw not a multiple of 64 (10x10 positions; a 100x100 latent in decode) is refused with MvdError before any launch: the
    output buffers keep their sentinel."""
    import ctypes as C
    from mvd_amd import _lib as L
    _, _, m = sd21_vae
    m.mid_attention(torch.zeros(1, 8, 8, 512, dtype=torch.bfloat16, device="cuda"), decoder=True)   # binds a workspace
    x = torch.ones(1, 10, 10, 512, dtype=torch.bfloat16, device="cuda")
    out = torch.full_like(x, 7.0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for dec in (0, 1):
        with pytest.raises(L.MvdError, match="multiples of 64"):
            L.call("mvd_vae_mid_attention", m._h, dec, C.c_void_p(x.data_ptr()), 1, 10, 10, C.c_void_p(out.data_ptr()), stream)
    with pytest.raises(L.MvdError, match="multiples of 64"):
        m.mid_attention(x, decoder=False)
    z = torch.zeros(1, 4, 100, 100, device="cuda")
    img = torch.full((1, 3, 800, 800), 7.0, device="cuda")
    with pytest.raises(L.MvdError, match="multiples of 64"):
        L.call("mvd_vae_decode", m._h, C.c_void_p(z.data_ptr()), 1, 100, 100, C.c_void_p(img.data_ptr()), stream)
    with pytest.raises(L.MvdError, match="multiples of 64"):
        m.decode(z)
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (img == 7.0).all(), "a refused call wrote its output"


# ------------------------------------------------------------------------------- 3. every conv / GEMM launch of encode + decode
def vae_launches(size):
    """The distinct GEMM / implicit-conv launches of one SD-2.1 encode (size x size image) and decode (size / 8 latent), batch 1,
    mirroring encode_impl / decode_impl / VCtx of vae.hip.  ('conv', H, W, cin, cout, stride, ups, residual, shortcut channels) and
    ('linear', M, N, K, bias, residual, fp32 output, alpha)."""
    from oracle import vae as OV
    cfg = OV.VAEConfig.sd21()
    ch, n, R = cfg.block_out_channels, len(cfg.block_out_channels), cfg.layers_per_block
    out = []

    def add(t):
        if t not in out:
            out.append(t)

    def resnet(h, ci, co):
        add(("conv", h, h, ci, co, 1, 0, False, 0))                         # conv1 on GN+SiLU(x)
        add(("conv", h, h, co, co, 1, 0, ci == co, 0 if ci == co else ci))  # conv2 + x, or || 1x1 conv_shortcut(x)

    def mid(h, c):
        hw = h * h
        resnet(h, c, c)
        add(("linear", hw, c, c, True, False, False, 1.0))                   # q / k projections
        add(("linear", c, hw, c, False, False, False, 1.0))                  # V^T = W_v . x^T  (roles swapped)
        add(("linear", hw, hw, c, False, False, True, 1.0 / math.sqrt(c)))   # S = q.k^T / sqrt(C), fp32
        add(("linear", hw, c, hw, True, False, False, 1.0))                  # P.V + b_v, K = hw
        add(("linear", hw, c, c, True, True, False, 1.0))                    # out-projection + residual

    h = size
    add(("linear", h * h, ch[0], 64, True, False, False, 1.0))               # encoder conv_in: im2col rows, K = 9*3 -> 64
    prev = ch[0]
    for i, c in enumerate(ch):
        for j in range(R):
            resnet(h, prev if j == 0 else c, c)
        prev = c
        if i + 1 < n:
            add(("conv", h, h, c, c, 2, 0, False, 0))                       # Downsample2D: bottom/right pad + stride 2
            h //= 2
    mid(h, ch[-1])
    add(("linear", h * h, ch[-1], 64, True, False, False, 1.0))              # decoder conv_in: K = 9*4 -> 64
    prev = ch[-1]
    for i, c in enumerate(reversed(ch)):
        for j in range(R + 1):
            resnet(h, prev if j == 0 else c, c)
        prev = c
        if i + 1 < n:
            add(("conv", h, h, c, c, 1, 1, False, 0))                       # Upsample2D: nearest 2x + conv
            h *= 2
    return out


def _ids(launches):
    def one(t):
        if t[0] == "conv":
            _, h, w, ci, co, st, up, res, sc = t
            return f"conv{h}x{w}_{ci}-{co}" + ("_s2" if st == 2 else "") + ("_up" if up else "") + ("_res" if res else "") + (f"_sc{sc}" if sc else "")
        _, m, n, k, bias, res, f32, alpha = t
        return f"lin{m}x{n}x{k}" + ("_res" if res else "") + ("_f32" if f32 else "") + ("_alpha" if alpha != 1.0 else "")
    return [one(t) for t in launches]


_L512, _L768 = vae_launches(512), vae_launches(768)


def _run_launch(ops, t, seed):
    from mvd_amd.packing import _conv_w
    if t[0] == "linear":
        _, m, n, k, bias, res, f32, alpha = t
        a, w = grnd(m, k, seed=seed), grnd(n, k, scale=1 / math.sqrt(k), seed=seed + 1)
        b = grnd(n, seed=seed + 2, dtype=torch.float32) if bias else None
        r = grnd(m, n, seed=seed + 3) if res else None
        sk = ops.engine_splitk(m, n, k)
        got = ops.linear(a, w, b, res=r, alpha=alpha, out_f32=f32, splitk=sk)
        want = a.float() @ w.float().T
        if b is not None:
            want += b
        want *= alpha
        if r is not None:
            want += r.float()
        return got, want, f32
    _, h, w_, ci, co, st, up, res, sc = t
    x = grnd(1, h, w_, ci, seed=seed)
    w3 = grnd(co, ci, 3, 3, scale=1 / math.sqrt(9 * ci + sc), seed=seed + 1)
    b = grnd(co, seed=seed + 2, dtype=torch.float32)
    oh, ow = (h * 2, w_ * 2) if up else ((h // 2, w_ // 2) if st == 2 else (h, w_))
    r = grnd(1, oh, ow, co, seed=seed + 3) if res else None
    s = grnd(1, oh, ow, sc, seed=seed + 4) if sc else None
    wsc = grnd(co, sc, scale=1 / math.sqrt(9 * ci + sc), seed=seed + 5) if sc else None
    wp = _conv_w(w3).to(torch.bfloat16)
    if sc:
        wp = torch.cat([wp, wsc], dim=1).contiguous()
    sk = ops.engine_splitk(oh * ow, co, 9 * ci + sc, conv=True)
    got = ops.conv3x3(x, wp, b, stride=st, upsample=bool(up), res=r, shortcut=s, splitk=sk, asym_pad=st == 2)
    want = conv3_ref(x, w3, b, stride=st, ups=bool(up), asym=st == 2)
    if r is not None:
        want += r.float()
    if sc:
        want += s.float() @ wsc.float().T
    return got, want, False


@pytest.mark.parametrize("t", _L512, ids=_ids(_L512))
def test_vae_launch_512(ops, t):
    """One distinct conv / GEMM launch of an SD-2.1 encode + decode at 512x512 (batch 1) vs fp32 torch on the same bf16 operands:
    close() of test_cfg4_shapes_gpu (2^-7 * max|ref|, rel-L2 6e-3); fp32 outputs (the score GEMM) 1e-4 * max|ref|."""
    got, want, f32 = _run_launch(ops, t, 11)
    plan = ops.last_gemm_plan()
    rel = close(got, want, tol=1e-4 if f32 else 2 ** -7, what=str(t))
    print(f"{_ids([t])[0]}: cfg {plan['cfg']} split {plan['splitk']} rel-L2 {rel:.3g}")


@pytest.mark.parametrize("t", _L768, ids=_ids(_L768))
def test_vae_launch_768(ops, t):
    """The same at 768x768 (M up to 589,824 rows; the 9216 x 9216 fp32 score GEMM, P.V with K = 9216): same bounds."""
    got, want, f32 = _run_launch(ops, t, 13)
    plan = ops.last_gemm_plan()
    rel = close(got, want, tol=1e-4 if f32 else 2 ** -7, what=str(t))
    print(f"{_ids([t])[0]}: cfg {plan['cfg']} split {plan['splitk']} rel-L2 {rel:.3g}")


# ------------------------------------------------------------------------------- 4. GroupNorm at the VAE's maps
# (hw, C) of the encoder's and the decoder's GroupNorms at 768x768: 4 channels per group (C = 128) up to 16
_GN768 = [(589824, 128), (589824, 256), (147456, 128), (147456, 256), (147456, 512), (36864, 256), (36864, 512), (9216, 512)]


@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("hw,c", _GN768)
def test_groupnorm_vae_maps(ops, hw, c, silu):
    """GroupNorm (32 groups, eps 1e-6) +- SiLU over the VAE's 768x768 maps (the two-kernel form at 4 channels per group, the
    one-pass form above) vs fp64 on the same bf16 input.  Each group sits on a common offset of ~+-20 (|mean| ~ 20 x the spread:
    E[x^2] - mean^2 would lose every digit) with channel offsets of 0.3 inside it.  Bound: close() of test_cfg4_shapes_gpu."""
    g = torch.Generator(device="cuda").manual_seed(hw + c + silu)
    grp = (20.0 * torch.randn(32, 1, generator=g, device="cuda")).expand(32, c // 32).reshape(c)
    off = grp + 0.3 * torch.randn(c, generator=g, device="cuda")
    x = (torch.randn(1, hw, c, generator=g, device="cuda") + off).to(torch.bfloat16)
    gamma = 1.0 + 0.1 * torch.randn(c, generator=g, device="cuda")
    beta = 0.1 * torch.randn(c, generator=g, device="cuda")
    got = ops.groupnorm(x, gamma, beta, groups=32, eps=1e-6, silu=silu)
    want = F.group_norm(x.double().transpose(1, 2), 32, gamma.double(), beta.double(), 1e-6).transpose(1, 2)
    if silu:
        want = F.silu(want)
    rel = close(got, want, what=f"groupnorm hw={hw} C={c} silu={silu}")
    print(f"groupnorm hw={hw} C={c} silu={silu}: rel-L2 {rel:.3g}")


# ------------------------------------------------------------------------------- 5. conv_out
@pytest.mark.parametrize("h,c,cout", [(512, 128, 3), (768, 128, 3), (64, 512, 8), (96, 512, 8)])
def test_conv_out_vae(ops, h, c, cout):
    """conv_out: the decoder's C = 128 -> 3 at 512x512 and 768x768, the encoder's C = 512 -> 8 at 64x64 and 96x96 (fp32 output,
    fp32 accumulate) vs fp64 on the same bf16 operands: 1e-4 * max|ref|, as test_ops_gpu.test_conv_in_out."""
    from mvd_amd.packing import _conv_w
    x = grnd(1, h, h, c, seed=21)
    w = grnd(cout, c, 3, 3, scale=1 / math.sqrt(9 * c), seed=22)
    b = grnd(cout, seed=23, dtype=torch.float32)
    got = ops.conv_out(x, _conv_w(w, tap_major=True).to(torch.bfloat16).contiguous(), b)
    want = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), padding=1)
    rel = close(got, want, tol=1e-4, what=f"conv_out {h}x{h} C={c} -> {cout}")
    print(f"conv_out {h} C={c} -> {cout}: rel-L2 {rel:.3g}")


# ------------------------------------------------------------------------------- 6. gaussian_sample
def test_gaussian_sample_clamp(ops):
    """DiagonalGaussianDistribution.sample() x scaling factor (0.18215) with logvar spread over [-40, 30], so that both clamp
    bounds (-30, 20) are crossed, on a non-square map; the mean is drawn at the size of the std so that a missing lower clamp
    (std e^-20 instead of e^-15) is not hidden under it.  Reference: the fp64 formula on the same fp32 inputs.  Bound:
    12 fp32 ulps (2^-23) of (|mean| + |std * noise|) * scale -- __expf(0.5 lv) alone is ~6 ulps off at |0.5 lv| = 15."""
    B, c, H, W = 2, 4, 48, 80
    g = torch.Generator(device="cuda").manual_seed(9)
    n = B * c * H * W
    lv = torch.linspace(-40.0, 30.0, n, device="cuda")[torch.randperm(n, generator=g, device="cuda")].view(B, c, H, W)
    std = torch.exp(0.5 * lv.double().clamp(-30.0, 20.0))
    mean = (torch.randn(B, c, H, W, generator=g, device="cuda", dtype=torch.float64) * std).float()
    noise = torch.randn(B, c, H, W, generator=g, device="cuda")
    mom = torch.cat([mean, lv], dim=1).contiguous()
    out = torch.empty_like(noise)
    import ctypes as C
    from mvd_amd import _lib as L
    L.call("mvd_op_gaussian_sample", C.c_void_p(mom.data_ptr()), C.c_void_p(noise.data_ptr()), B, c, H * W, 0.18215,
           C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    want = (mean.double() + std * noise.double()) * 0.18215
    bound = 12 * 2 ** -23 * (mean.double().abs() + (std * noise.double()).abs()) * 0.18215
    ratio = ((out.double() - want).abs() / bound.clamp_min(1e-300)).max().item()
    assert ratio <= 1.0, f"gaussian_sample: worst err / bound {ratio:.3g}"
    assert (lv < -30).any() and (lv > 20).any()
    print(f"gaussian_sample: worst err / bound {ratio:.3f}")


# ------------------------------------------------------------------------------- 7. activations of 2 GiB
def test_resnet_conv_past_2gib(ops):
    """GroupNorm+SiLU and a resnet conv 128 -> 128 + residual at 512x512, batch 32 (a batch-32 decode's last level): input and
    output are 32 x 512 x 512 x 128 x 2 B = 2^31 B each.  Images 0, 15, 16 and 31 (either side of 2^30 bytes, and the last) are
    checked one by one: GroupNorm against fp64 on the same bf16 input, the conv against fp32 torch on the kernel's own GroupNorm
    output + the residual; bounds: close() of test_cfg4_shapes_gpu.  The plan must be the 128x128 lock-step tile (config 3) over all
    65,536 row tiles: the 32-bit buffer-addressed kernels (gemm_pp, gemm_sm, conv_ws) refuse operands of 2^31 bytes."""
    from mvd_amd.packing import _conv_w
    B, H, C = 32, 512, 128
    x = torch.empty(B, H, H, C, dtype=torch.bfloat16, device="cuda")
    assert x.numel() * 2 == 2 ** 31
    g = torch.Generator(device="cuda").manual_seed(17)
    off = torch.randn(C, generator=g, device="cuda")
    for i in range(B):
        x[i] = (torch.randn(H, H, C, generator=g, device="cuda") + off).to(torch.bfloat16)
    gamma = 1.0 + 0.1 * torch.randn(C, generator=g, device="cuda")
    beta = 0.1 * torch.randn(C, generator=g, device="cuda")
    t = ops.groupnorm(x.view(B, H * H, C), gamma, beta, groups=32, eps=1e-6, silu=True).view(B, H, H, C)
    w = grnd(C, C, 3, 3, scale=1 / math.sqrt(9 * C), seed=31)
    b = grnd(C, seed=32, dtype=torch.float32)
    sk = ops.engine_splitk(B * H * H, C, 9 * C, conv=True)
    out = ops.conv3x3(t, _conv_w(w).to(torch.bfloat16).contiguous(), b, res=x, splitk=sk)
    plan = ops.last_gemm_plan()
    assert sk == 1 and plan["cfg"] == 3 and plan["splitk"] == 1 and plan["tiles"] == B * H * H // 128, plan
    for i in (0, 15, 16, 31):
        gn = F.silu(F.group_norm(x[i:i + 1].double().permute(0, 3, 1, 2), 32, gamma.double(), beta.double(), 1e-6)).permute(0, 2, 3, 1)
        r1 = close(t[i:i + 1], gn, what=f"2 GiB groupnorm image {i}")
        want = conv3_ref(t[i:i + 1], w, b) + x[i:i + 1].float()
        r2 = close(out[i:i + 1], want, what=f"2 GiB conv image {i}")
        print(f"2 GiB image {i}: groupnorm rel-L2 {r1:.3g}, conv rel-L2 {r2:.3g}")
    print(f"2 GiB plan: {plan}")
