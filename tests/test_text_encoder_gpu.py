"""Row N5 on the GPU: the causal attention kernel (``mvd_op_attention_causal``), ``CLIPTextModelHIP`` (C ABI
``mvd_text_encode``) against the fp32 CPU restatement tests/clip_text_ref.py on identical seeded weights, exact causality,
the error paths, and ``create_mvd_pipeline(..., text_encoder="hip")`` on a snapshot written without transformers
(/root/reference/src/models/pipeline.py:52-75).

Tolerances: the attention operator is held to what tests/test_ops_gpu.py::test_attention holds ``mvd_op_attention`` to
(max-abs <= 2^-6 * max|ref|).  The full encoder is held to the project's end-to-end tolerance (rel-L2 <= 2e-2, max-abs <=
5e-2 * max|ref|, tests/test_vae_gpu.py): the restatement with every GEMM operand and weight rounded to bf16 and an fp32
residual stream sits at rel-L2 6.2e-3 (tiny) / 6.5e-3 (SD-2.1 size) on the CPU, so the bound leaves ~3x over storage
precision alone.  Every test prints its figures before it asserts; DESIGN.md section 9, row N5 records them."""
import ctypes as C

import pytest
import torch

from tests import clip_text_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _bf(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16)


def _causal_ref(q, k, v, heads, scale=0.125):
    B, n, _ = q.shape
    sp = lambda t: t.float().view(B, n, heads, 64).transpose(1, 2)   # noqa: E731
    s = sp(q) @ sp(k).transpose(-1, -2) * scale + torch.full((n, n), float("-inf")).triu(1)
    return (s.softmax(-1) @ sp(v)).transpose(1, 2).reshape(B, n, heads * 64)


# ------------------------------------------------------------------------------- the attention operator
@pytest.mark.parametrize("B,heads,n", [(1, 16, 77), (3, 4, 77), (2, 20, 13), (64, 16, 77)])
def test_attention_causal_op(B, heads, n):
    from mvd_amd import ops
    from mvd_amd.packing import QSCALE
    Cc = heads * 64
    qkv = _bf(B, n, 3 * Cc, seed=B * 100 + n)                    # one fused buffer: q | k | v views with row stride 3C
    want = _causal_ref(qkv[..., :Cc], qkv[..., Cc:2 * Cc], qkv[..., 2 * Cc:], heads)
    d = qkv.cuda()
    got = ops.attention_causal(d[..., :Cc], d[..., Cc:2 * Cc], d[..., 2 * Cc:], heads, 0.125).float().cpu()
    assert torch.isfinite(got).all()
    err, ref = (got - want).abs().max().item(), want.abs().max().item()
    print(f"attention_causal {B}x{heads}x{n} scale=0.125: max-abs {err:.4g} / max|ref| {ref:.4g} = {err / ref:.3g}")
    assert err <= 2 ** -6 * ref
    # row 0 sees only itself: the output is v[0] (to bf16 rounding: v is bf16 already, so exactly)
    assert torch.equal(got[:, 0], qkv[:, 0, 2 * Cc:].float())
    # the prescaled form (scale = 0): q carries 64^-0.5 * log2(e)
    pre = qkv.clone()
    pre[..., :Cc] = (qkv[..., :Cc].float() * QSCALE).to(torch.bfloat16)
    want2 = _causal_ref((pre[..., :Cc].float() / QSCALE), pre[..., Cc:2 * Cc], pre[..., 2 * Cc:], heads)
    d2 = pre.cuda()
    got2 = ops.attention_causal(d2[..., :Cc], d2[..., Cc:2 * Cc], d2[..., 2 * Cc:], heads, 0.0).float().cpu()
    err2, ref2 = (got2 - want2).abs().max().item(), want2.abs().max().item()
    print(f"attention_causal {B}x{heads}x{n} prescaled: max-abs {err2:.4g} / max|ref| {ref2:.4g} = {err2 / ref2:.3g}")
    assert torch.isfinite(got2).all() and err2 <= 2 ** -6 * ref2


def test_attention_causal_ignores_later_keys_exactly():
    """Changing k / v rows >= t leaves the output rows < t bit-identical (no mask leak, no read of padded rows)."""
    from mvd_amd import ops
    B, heads, n, Cc = 2, 4, 77, 256
    a = _bf(B, n, 3 * Cc, seed=7)
    for t in (1, 16, 17, 40, 76):
        b = a.clone()
        b[:, t:] = _bf(B, n - t, 3 * Cc, seed=100 + t) * 3
        outs = [ops.attention_causal(x.cuda()[..., :Cc], x.cuda()[..., Cc:2 * Cc], x.cuda()[..., 2 * Cc:], heads, 0.125).cpu() for x in (a, b)]
        assert torch.equal(outs[0][:, :t], outs[1][:, :t]), t
        assert not torch.equal(outs[0][:, t:], outs[1][:, t:])


def test_attention_causal_rejects_bad_arguments():
    from mvd_amd import ops
    from mvd_amd._lib import MvdError
    x = torch.zeros(1, 97, 192, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(MvdError, match="exceeds 96"):
        ops.attention_causal(x[..., :64], x[..., 64:128], x[..., 128:], 1)


# ------------------------------------------------------------------------------- the encoder
_MODELS = {}


def _model(kind):
    """(cfg, state dict, CLIPTextModelHIP on the GPU), one per size and module."""
    if kind not in _MODELS:
        from mvd_amd.text_encoder import CLIPTextConfigLite, CLIPTextModelHIP
        cfg = R.TINY if kind == "tiny" else R.SD21
        sd = R.seeded_state_dict(cfg, seed=3)
        m = CLIPTextModelHIP(CLIPTextConfigLite(**cfg))
        res = m.load_state_dict(sd)
        assert not res.missing_keys and not res.unexpected_keys
        _MODELS[kind] = (cfg, sd, m.to("cuda").eval())
    return _MODELS[kind]


def _ref(cfg, sd, ids):
    with torch.no_grad():
        return R.text_forward(sd, ids, cfg["num_hidden_layers"], cfg["num_attention_heads"], cfg["hidden_act"], cfg["layer_norm_eps"])


@pytest.mark.parametrize("kind,B", [("tiny", 1), ("tiny", 3), ("sd21", 1), ("sd21", 2), ("sd21", 32)])
def test_encoder_parity(kind, B):
    cfg, sd, m = _model(kind)
    ids = R.prompt_like_ids(cfg, B, seed=B)
    want = _ref(cfg, sd, ids)
    m(ids.cuda())                                                # sizes and binds the workspace for this shape
    m._ws.view(torch.float32).fill_(float("nan"))                # poison: nothing a kernel did not write may reach the result
    out = m(ids.cuda())
    assert isinstance(out, tuple) and out[0] is out.last_hidden_state
    got = out[0]
    assert got.dtype == torch.float32 and got.is_cuda and got.shape == (B, cfg["max_position_embeddings"], cfg["hidden_size"])
    got = got.cpu()
    assert torch.isfinite(got).all()
    rel = R.rel_l2(got, want)
    mx = ((got - want).abs().max() / want.abs().max()).item()
    print(f"text encoder {kind} B={B}: rel-L2 {rel:.3e}, max-abs / max|ref| {mx:.3e} (max-abs {(got - want).abs().max().item():.3e}, "
          f"rms {want.pow(2).mean().sqrt().item():.3f})")
    assert rel <= 2e-2 and mx <= 5e-2, (kind, B, rel, mx)


@pytest.mark.parametrize("kind", ["tiny", "sd21"])
def test_encoder_causality_is_exact(kind):
    """ids A and A' that differ only at positions >= t: rows < t of the two outputs are bit-identical.  Same kernels, same
    shapes, row-independent arithmetic: any difference is a mask leak or a read of padded rows."""
    cfg, sd, m = _model(kind)
    a = R.prompt_like_ids(cfg, 2, seed=9)
    base = m(a.cuda())[0].cpu()
    for t in (5, 40):
        b = a.clone()
        b[:, t:] = torch.randint(1, cfg["vocab_size"], b[:, t:].shape, generator=torch.Generator().manual_seed(t))
        assert not torch.equal(a[:, t:], b[:, t:])
        other = m(b.cuda())[0].cpu()
        assert torch.equal(base[:, :t], other[:, :t]), (kind, t)
        assert not torch.equal(base[:, t:], other[:, t:])
    assert torch.equal(m(a.cuda())[0].cpu(), base)              # and the encode is deterministic


def test_encoder_short_sequence_and_position_rows():
    """seq_len < max_positions uses position rows 0..T-1; a causal encoder gives the same rows as the full-length call."""
    cfg, sd, m = _model("tiny")
    ids = R.prompt_like_ids(cfg, 2, seed=4)
    short = m(ids[:, :20].cuda())[0].cpu()
    want = _ref(cfg, sd, ids[:, :20])
    assert R.rel_l2(short, want) <= 2e-2
    assert short.shape == (2, 20, cfg["hidden_size"])


def test_error_paths_launch_nothing():
    from mvd_amd import _lib as L
    from mvd_amd.text_encoder import CLIPTextConfigLite, CLIPTextModelHIP
    cfg, sd, m = _model("tiny")
    m(R.prompt_like_ids(cfg, 1, seed=1).cuda())                  # (packs and registers the weights)
    bad = R.prompt_like_ids(cfg, 1, seed=1)
    bad[0, 3] = cfg["vocab_size"]
    with pytest.raises(L.MvdError, match="token ids"):
        m(bad.cuda())
    with pytest.raises(L.MvdError, match="max_position_embeddings"):
        m(torch.zeros(1, 78, dtype=torch.long, device="cuda"))
    # the C ABI itself: encode before the weights are set, an unbound and a too small workspace, seq_len > max_positions
    lib = L.lib()
    c = L.mvd_text_config_t()
    c.vocab_size, c.hidden_size, c.intermediate_size, c.num_layers, c.num_heads, c.max_positions = 1000, 128, 512, 2, 2, 77
    c.layer_norm_eps, c.act = 1e-5, 1
    h = C.c_void_p()
    L.call("mvd_text_create", C.byref(c), C.byref(h))
    ids = torch.zeros(1, 77, dtype=torch.int32, device="cuda")
    sentinel = torch.full((1, 77, 128), 123.0, device="cuda")
    args = (h, C.c_void_p(ids.data_ptr()), 1, 77, C.c_void_p(sentinel.data_ptr()), None)
    assert lib.mvd_text_encode(*args) < 0 and "missing weight slot" in L.last_error()
    for slot, t in m._packed.items():
        L.call("mvd_text_set_weight", h, slot.encode(), C.c_void_p(t.data_ptr()), t.numel(), 0 if t.dtype == torch.float32 else 1)
    assert lib.mvd_text_encode(*args) < 0 and "workspace not bound" in L.last_error()
    ws = torch.empty(4096, dtype=torch.uint8, device="cuda")
    L.call("mvd_text_bind_workspace", h, C.c_void_p(ws.data_ptr()), ws.numel())
    assert lib.mvd_text_encode(*args) < 0 and "workspace too small" in L.last_error()
    assert lib.mvd_text_encode(h, C.c_void_p(ids.data_ptr()), 1, 78, C.c_void_p(sentinel.data_ptr()), None) < 0
    assert "max_positions" in L.last_error()
    torch.cuda.synchronize()
    assert bool((sentinel == 123.0).all())                       # nothing was written
    need = lib.mvd_text_workspace_bytes(h, 1, 77)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    L.call("mvd_text_bind_workspace", h, C.c_void_p(ws.data_ptr()), ws.numel())
    ids = R.prompt_like_ids(cfg, 1, seed=2).to(torch.int32).cuda()
    L.call("mvd_text_encode", h, C.c_void_p(ids.data_ptr()), 1, 77, C.c_void_p(sentinel.data_ptr()), None)
    torch.cuda.synchronize()
    assert torch.equal(sentinel, m(ids.long())[0])               # the raw ABI and the module agree bit for bit
    lib.mvd_text_destroy(h)
    with pytest.raises(L.MvdError, match="hidden_act"):
        CLIPTextModelHIP(CLIPTextConfigLite(**dict(cfg, hidden_act="relu")))


# ------------------------------------------------------------------------------- the pipeline
PROMPTS = ["a photo of a red chair", "", "The  front VIEW of the chair", "the red chair!"]


@pytest.mark.parametrize("pad_token", ["<|endoftext|>", "!"])
def test_pipeline_with_native_text_encoder(tmp_path, pad_token):
    from mvd_amd.clip_tokenizer import CLIPTokenizerLite
    from mvd_amd.mvd_unet import create_mvd_pipeline
    from mvd_amd.text_encoder import CLIPTextModelHIP
    from tests.hub_fixture import REPO
    from tests.text_fixture import build_text_snapshot, expected_ids, fixture_vocab
    cache, snap, sds, tcfg = build_text_snapshot(str(tmp_path), pad_token=pad_token)
    kw = dict(dtype=torch.float32, cache_dir=str(tmp_path), cam_output_dim=96, cam_hidden_dim=48)
    pipe = create_mvd_pipeline(REPO, sampler="ddim", text_encoder="hip", **kw).to("cuda")
    assert isinstance(pipe.text_encoder, CLIPTextModelHIP) and isinstance(pipe.tokenizer, CLIPTokenizerLite)
    tok = pipe.tokenizer
    assert tok.model_max_length == 77 and tok.pad_token_id == fixture_vocab()[0][pad_token] and (tok.bos_token_id, tok.eos_token_id) == (0, 1)
    ids = tok(PROMPTS, padding="max_length", max_length=tok.model_max_length, truncation=True, return_tensors="pt").input_ids
    assert ids.tolist() == [expected_ids(p, pad_token) for p in PROMPTS]
    try:
        from transformers import CLIPTokenizer
    except ImportError:
        CLIPTokenizer = None
    if CLIPTokenizer is not None:
        vocab, merges = fixture_vocab()
        ref_tok = CLIPTokenizer(vocab=vocab, merges=[tuple(m.split()) for m in merges], pad_token=pad_token)
        assert ref_tok(PROMPTS, padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids.tolist() == ids.tolist()
    # the encoder on the snapshot's weights
    got = pipe.text_encoder(ids.cuda())[0].cpu()
    want = R.text_forward(sds["text_encoder"], ids, tcfg["num_hidden_layers"], tcfg["num_attention_heads"], tcfg["hidden_act"])
    rel, mx = R.rel_l2(got, want), ((got - want).abs().max() / want.abs().max()).item()
    print(f"pipeline text encoder (pad {pad_token!r}): rel-L2 {rel:.3e}, max-abs / max|ref| {mx:.3e}")
    assert torch.isfinite(got).all() and rel <= 2e-2 and mx <= 5e-2
    # prompt strings add nothing but the encode
    lat = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(2))
    call = dict(guidance_scale=7.5, num_inference_steps=2, output_type="latent")
    torch.manual_seed(0)
    a = pipe(prompt="a photo of a red chair", negative_prompt="", latents=lat.clone(), **call)["images"]
    pe = pipe.text_encoder(tok("a photo of a red chair", padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids.cuda())[0]
    ne = pipe.text_encoder(tok("", padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids.cuda())[0]
    torch.manual_seed(0)
    b = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat.clone(), **call)["images"]
    assert a.shape == (1, 4, 16, 16) and torch.isfinite(a).all() and torch.equal(a, b)
    c = pipe(prompt="the front view", negative_prompt="", latents=lat.clone(), **call)["images"]
    assert not torch.equal(a, c)                                 # the prompt reaches the result
    # without the keyword: today's components (transformers' when the package imports, else none)
    default = create_mvd_pipeline(REPO, **kw)
    try:
        import transformers
    except ImportError:
        assert default.text_encoder is None and default.tokenizer is None
    else:
        assert isinstance(default.text_encoder, transformers.CLIPTextModel) and isinstance(default.tokenizer, transformers.CLIPTokenizer)
        dt = default.tokenizer(PROMPTS, padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids
        assert dt.tolist() == ids.tolist()


def test_pipeline_native_text_encoder_requires_the_files(tmp_path):
    from mvd_amd._lib import MvdError
    from mvd_amd.mvd_unet import create_mvd_pipeline
    from tests.hub_fixture import REPO, build_fake_hf_cache
    build_fake_hf_cache(str(tmp_path), with_text_encoder=False)
    with pytest.raises(MvdError, match="lacks"):
        create_mvd_pipeline(REPO, dtype=torch.float32, cache_dir=str(tmp_path), cam_output_dim=96, cam_hidden_dim=48, text_encoder="hip")
    with pytest.raises(ValueError, match="text_encoder"):
        create_mvd_pipeline(REPO, dtype=torch.float32, cache_dir=str(tmp_path), cam_output_dim=96, cam_hidden_dim=48, text_encoder="onnx")
