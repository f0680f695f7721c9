"""The CLIP towers equal the composition of their operators, bit for bit.

``mvd_text_encode`` / ``mvd_vision_encode`` run a host schedule (text.hip encode_impl, vision.hip vencode_impl, clip_layer.h
clip_layers) over one arena: buffers are reused, the split-K partials alias the space behind the activations, every split-K launch
takes its tile counters at a running offset.  Here the same launches are composed in Python on the module's own packed weights (q
rows prescaled), one plain buffer per activation and a fresh workspace per GEMM: the operator entries of tests/test_clip_ops_gpu.py,
``ops.attention_causal(scale=0)``, ``mvd_debug_clip_linear`` (ClipCtx::linear itself: the small-M planner with its in-kernel
split-K, else the tiled kernels) and ``mvd_debug_clip_attention`` (the function vencode_impl calls).  The tower runs on a
NaN-poisoned workspace.  ``torch.equal`` is required: a difference is a schedule error, a kernel reading what it should not (a stale
f1 or g1), or a launch that depends on the workspace's history."""
import pytest
import torch

from tests import clip_text_ref as RT
from tests import clip_vision_ref as V

pytestmark = pytest.mark.gpu

TEXT = {
    "tiny": RT.TINY,
    # H = 1024, I = 4096 at 77 .. 231 rows: the small-M planner splits K and the tile counters come into play
    "wide": dict(RT.TINY, hidden_size=1024, intermediate_size=4096, num_attention_heads=16, hidden_act="gelu"),
    "no-layers": dict(RT.TINY, num_hidden_layers=0),
}
VISION = {
    "tiny": V.TINY,
    "p14": V.P14,
    "wide": dict(V.TINY, hidden_size=1024, intermediate_size=4096, num_attention_heads=16, projection_dim=768, hidden_act="gelu"),
}
_MODELS = {}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mvd_amd import ops as O
    return O


def _text(kind):
    if ("text", kind) not in _MODELS:
        from mvd_amd.text_encoder import CLIPTextConfigLite, CLIPTextModelHIP
        m = CLIPTextModelHIP(CLIPTextConfigLite(**TEXT[kind]))
        m.load_state_dict(RT.seeded_state_dict(TEXT[kind], seed=11))
        _MODELS["text", kind] = m.to("cuda").eval()
    return _MODELS["text", kind]


def _vision(kind):
    if ("vision", kind) not in _MODELS:
        from mvd_amd.vision_encoder import CLIPVisionConfigLite, CLIPVisionModelHIP
        m = CLIPVisionModelHIP(CLIPVisionConfigLite(**VISION[kind]))
        m.load_state_dict(V.seeded_vision_state_dict(VISION[kind], seed=12))
        _MODELS["vision", kind] = m.to("cuda").eval()
    return _MODELS["vision", kind]


ROUTES = []          # (small-M tile or -1, split-K factor) of every GEMM a replay launched


def _linear(ops, *a, **k):
    return ops.clip_linear(*a, route=ROUTES, **k)


def _routes():
    """the routes since the last call, and whether a small-M launch among them split K in the kernel"""
    seen = sorted(set(ROUTES))
    del ROUTES[:]
    return seen, any(tile >= 0 and s > 1 for tile, s in seen)


def _layers(ops, W, x, layers, H, I, act, eps, tower, attention):
    """clip_layers: `layers` layers over the residual stream x (in place) -> the last fc2 result, not yet added (None without layers)"""
    dl = None
    for l in range(layers):
        w = lambda k, *s: W[f"layers.{l}.{k}"].view(*s)      # noqa: E731
        h = ops.clip_add_ln(x, dl, w("ln1.g", H), w("ln1.b", H), eps, False, tower)
        qkv = _linear(ops, h, w("qkv.w", 3 * H, H), w("qkv.b", 3 * H))
        at = attention(qkv)
        dl = _linear(ops, at, w("out.w", H, H), w("out.b", H), out_f32=True)
        h = ops.clip_add_ln(x, dl, w("ln2.g", H), w("ln2.b", H), eps, False, tower)
        f1 = _linear(ops, h, w("fc1.w", I, H), w("fc1.b", I), out_f32=True)
        g1 = ops.clip_act(f1, act, tower)
        dl = _linear(ops, g1, w("fc2.w", H, I), w("fc2.b", H), out_f32=True)
    return dl


def replay_text(ops, m, ids):
    from mvd_amd.text_encoder import ACTS
    c, W = m.config, m._packed
    B, T = ids.shape
    H, heads = c.hidden_size, c.num_attention_heads
    x = ops.text_embed(ids.reshape(-1).to(torch.int32).contiguous(), W["tok"], W["pos"], T)

    def attention(qkv):
        q = qkv.view(B, T, 3 * H)
        return ops.attention_causal(q[..., :H], q[..., H:2 * H], q[..., 2 * H:], heads, scale=0.0).view(B * T, H)

    dl = _layers(ops, W, x, c.num_hidden_layers, H, c.intermediate_size, ACTS[c.hidden_act], c.layer_norm_eps, "text", attention)
    return ops.clip_add_ln(x, dl, W["final_ln.g"], W["final_ln.b"], c.layer_norm_eps, True, "text").view(B, T, H)


def replay_vision(ops, m, pv):
    from mvd_amd.clip_score import pool_project
    from mvd_amd.text_encoder import ACTS
    c, W = m.config, m._packed
    B, T, H, heads = pv.shape[0], c.num_tokens, c.hidden_size, c.num_attention_heads
    patches = ops.vit_patchify(pv, c.patch_size)
    po = _linear(ops, patches, W["patch.w"].view(H, c.patch_k), None, out_f32=True)
    x = ops.vit_embed_ln(po, W["cls"], W["pos"].view(T, H), W["pre_ln.g"], W["pre_ln.b"], B, c.layer_norm_eps)
    dl = _layers(ops, W, x, c.num_hidden_layers, H, c.intermediate_size, ACTS[c.hidden_act], c.layer_norm_eps, "vision",
                 lambda qkv: ops.clip_attention(qkv, B, heads))
    hid = ops.vit_fold(x, dl) if dl is not None else x.clone()
    raw, nrm = pool_project(x.view(B, T, H), W["proj.w"].view(c.projection_dim, H), delta=None if dl is None else dl.view(B, T, H),
                            ln=(W["post_ln.g"], W["post_ln.b"]), eps=c.layer_norm_eps)
    return hid.view(B, T, H), raw, nrm


def _differs(got, want):
    return f"{int((got != want).sum())} of {want.numel()} elements differ, max-abs {(got - want).abs().max().item():.3g}"


@pytest.mark.parametrize("kind,B,T", [("tiny", 1, 77), ("tiny", 3, 77), ("tiny", 3, 20), ("wide", 1, 77), ("wide", 3, 20), ("no-layers", 3, 77)])
def test_text_tower_equals_its_operators(ops, kind, B, T):
    m = _text(kind)
    ids = RT.prompt_like_ids(TEXT[kind], B, seed=B + T, seq_len=T).cuda()
    m(ids)                                                        # packs the weights, sizes and binds the workspace
    m._ws.view(torch.float32).fill_(float("nan"))
    want = m(ids)[0]
    got = replay_text(ops, m, ids)
    assert torch.isfinite(want).all() and want.shape == got.shape == (B, T, m.config.hidden_size)
    same = torch.equal(got, want)
    routes, split = _routes()
    print(f"\n[clip-replay] text {kind} B={B} T={T}: {'bit-identical' if same else _differs(got, want)}; GEMM (small-M tile, split-K) {routes}")
    assert same
    assert split or kind != "wide", "no small-M launch of the wide tower split K: the tile counters were not exercised"


@pytest.mark.parametrize("kind,B", [("tiny", 1), ("tiny", 3), ("p14", 2), ("wide", 2)])
def test_vision_tower_equals_its_operators(ops, kind, B):
    m = _vision(kind)
    pv = V.seeded_pixel_values(VISION[kind], B, seed=B).cuda()
    m.encode(pv, want_hidden=True)
    m._handle.ws.view(torch.float32).fill_(float("nan"))
    want = m.encode(pv, want_hidden=True)
    got = replay_vision(ops, m, pv)
    names = ("last hidden state", "embeds", "normalised embeds")
    same = [torch.equal(g, w) for g, w in zip(got, want)]
    routes, split = _routes()
    print(f"\n[clip-replay] vision {kind} B={B}: " + "; ".join(f"{n} {'bit-identical' if s else _differs(g, w)}" for n, s, g, w in zip(names, same, got, want))
          + f"; GEMM (small-M tile, split-K) {routes}")
    assert all(torch.isfinite(w).all() for w in want) and all(g.shape == w.shape for g, w in zip(got, want))
    assert all(same)
    assert split or kind != "wide", "no small-M launch of the wide tower split K: the tile counters were not exercised"
