"""The data of tests/test_clip_ops_gpu.py can tell right from wrong -- shown on the CPU, as test_stat_probe_cpu.py and
test_exact_strides_cpu.py do for theirs:

* every spike-probed kernel (add + LayerNorm, the ViT's embed + LayerNorm, the pool kernel's LayerNorm): ``stat_probe.emulate``
  with each of ``FAULTS`` fails ``stat_probe.check`` at the scheduled hot positions, the unfaulted emulation passes, and every
  column of every width is hot in some launch of at most ``BUDGET``;
* the L2 normalisation: a sum of squares that misses the spike misses the 1e-5 bound;
* the index kernels: each mutation (position row ``row`` for ``row % T``, patch order (py, px, c), the class row from patch 0, image
  b reading image b - 1's patches) changes the expected output;
* the activation: torch's fp32 formula rounded to bf16 meets the per-element and the bias bound on the GPU test's inputs; 1.70 for
  1.702 and tanh-GELU for erf-GELU miss the bias bound; GELU written as 0.5 x (1 + erf) -- the form the kernel had -- misses the
  per-element bound in its negative tail;
* the C ABI: the new entries are declared, exported and refuse what their kernels cannot take before any launch."""
import os

import pytest
import torch

from tests import clip_ops_ref as R
from tests import clip_vision_ref as V
from tests import stat_probe as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 0.75
ENTRIES = ("mvd_op_text_add_ln", "mvd_op_vision_add_ln", "mvd_op_text_act", "mvd_op_vision_act", "mvd_op_text_embed", "mvd_op_vit_patchify",
           "mvd_op_vit_embed_ln", "mvd_op_vit_fold", "mvd_op_clip_l2norm", "mvd_op_vae_pointwise", "mvd_debug_clip_linear_ws_bytes",
           "mvd_debug_clip_linear", "mvd_debug_clip_attention")


# ------------------------------------------------------------------------------------------------ spike probes
def _sees_the_faults(H, rows, flip, what):
    slots = R.probe_slots(H, rows)
    assert len(slots) <= P.BUDGET and H <= P.EXHAUSTIVE_MAX
    assert set(slots.reshape(-1).tolist()) == set(range(H)), "a column is never hot"
    lay = P.Rows(rows, H)
    gam, bet = lay.affine(*R.probe_affine(H))
    worst = 0.0
    for i in sorted({0, len(slots) - 1}):
        hot = slots[i]
        first, second = R.probe_pair(H, rows, hot, i, flip)
        col = hot[:, None]
        in_first = first.gather(1, col)[:, 0] == P.spike(H)
        assert bool((in_first != (second.gather(1, col)[:, 0] == P.spike(H))).all()), "the spike sits in exactly one of the two inputs"
        if rows > 1:
            assert bool(in_first.any()) and not bool(in_first.all()), "both inputs carry spikes in one launch"
        s = first + second
        want = P.reference(s, R.EPS, gam, bet)
        ok = P.check(P.emulate(s, hot, None, R.EPS, gam, bet), want, hot, lay, what)
        assert max(ok) <= MARGIN, (what, ok)
        worst = max(worst, *ok)
        for fault in P.FAULTS:
            assert P.passes(P.emulate(s, hot, fault, R.EPS, gam, bet), want, hot, lay) is None, f"{what}: '{fault}' goes unseen"
        # a statistic taken BEFORE the add (of the first input alone) is seen too
        stale = P.emulate(first, hot, None, R.EPS, gam, bet)
        assert P.passes(stale, want, hot, lay) is None, f"{what}: statistics of the first input alone go unseen"
    return worst


@pytest.mark.parametrize("H", R.ADD_LN_H)
def test_add_ln_probe_sees_the_faults(H):
    for flip in (0, 1):         # the text entry's and the vision entry's parity: together every column is hot in x and in delta
        _sees_the_faults(H, R.PROBE_ROWS, flip, f"add+LN {H}")
    a = R.probe_pair(H, R.PROBE_ROWS, R.probe_slots(H)[0], 0, 0)[0]
    b = R.probe_pair(H, R.PROBE_ROWS, R.probe_slots(H)[0], 0, 1)[1]
    assert torch.equal(a == P.spike(H), b == P.spike(H)), "flip moves every spike to the other input"


@pytest.mark.parametrize("H", R.EMBED_LN_PROBE_H)
def test_embed_ln_probe_sees_the_faults(H):
    """B = 1, T = PROBE_ROWS: row 0's spike must sit in cls or pos[0], the patch rows' in patch_out or pos"""
    _sees_the_faults(H, R.PROBE_ROWS, 0, f"embed+LN {H}")


@pytest.mark.parametrize("H", R.POOL_PROBE_H)
def test_pool_ln_probe_sees_the_faults(H):
    _sees_the_faults(H, R.PROBE_ROWS, 0, f"pool LN {H}")


@pytest.mark.parametrize("dim", [4, 66, 2048])
def test_l2norm_spike_sees_a_dropped_element(dim):
    x, hot = R.l2norm_case(5, dim)
    want = R.l2norm(x)
    ok = (R.l2norm(x.float()).float().double() - want).abs().max().item()
    bad = (R.l2norm(x, drop=hot) - want).abs().max().item()
    assert ok <= 1e-5 < bad, (dim, ok, bad)


# ------------------------------------------------------------------------------------------------ index kernels
@pytest.mark.parametrize("T", [1, 20, 77])
def test_text_embed_mutation(T):
    rows = 2 * T + 1
    ids, tok, pos = R.text_embed_case(rows, T, 64)
    want = R.text_embed(ids, tok, pos, T)
    assert want.shape == (rows, 64) and torch.equal(want[T], tok[ids[T].long()] + pos[0])
    assert not torch.equal(R.text_embed(ids, tok, pos, T, "pos_row"), want)
    # the clamp the header documents
    bad = ids.clone()
    bad[1], bad[2] = -1, tok.shape[0]
    got = R.text_embed(bad, tok, pos, T)
    assert torch.equal(got[1], tok[0] + pos[1 % T]) and torch.equal(got[2], tok[-1] + pos[2 % T])


@pytest.mark.parametrize("S,P_", [(32, 8), (28, 14), (224, 32)])
def test_patchify_mutation(S, P_):
    pv = V.seeded_pixel_values(dict(image_size=S), 2, seed=S)
    want = R.patch_rows_bf16(pv, P_)
    k = 3 * P_ * P_
    assert want.shape == (2 * (S // P_) ** 2, (k + 63) // 64 * 64) and bool((want[:, k:] == 0).all())
    assert not torch.equal(R.patch_rows_bf16(pv, P_, "pyx_c"), want)
    # element (c, py, px) of patch (pr, pc) of image 1
    g = S // P_
    c, py, px, pr, pc = 2, P_ - 1, 1, g - 1, 0
    assert want[g * g + pr * g + pc, (c * P_ + py) * P_ + px] == R.rne_bf16(pv[1, c, pr * P_ + py, pc * P_ + px])


@pytest.mark.parametrize("B,T,H", R.EMBED_LN_CASES)
def test_embed_rows_mutations(B, T, H):
    po, cls, pos, _, _ = R.embed_ln_case(B, T, H)
    want = R.embed_rows(po, cls, pos, B)
    assert torch.equal(want[0], cls + pos[0]) and torch.equal(want[(B - 1) * T + 2], po[(B - 1) * (T - 1) + 1] + pos[2])
    assert not torch.equal(R.embed_rows(po, cls, pos, B, "cls_from_patch0"), want)
    if B > 1:
        assert not torch.equal(R.embed_rows(po, cls, pos, B, "prev_image"), want)
        assert all(torch.equal(want[b * T], want[0]) for b in range(B))


# ------------------------------------------------------------------------------------------------ activation
@pytest.mark.parametrize("act", [0, 1])
def test_activation_bounds_tell_right_from_wrong(act):
    x = R.act_inputs()
    assert x.numel() >= 65536 and x.min().item() == -8.0 and x.max().item() == 8.0
    want = R.act64(x, act)
    right = R.rne_bf16(R.act_f32(x, act)).double()
    worst = ((right - want).abs() / R.act_bound(want)).max().item()
    mean, bound, n = R.act_bias(right, want)
    print(f"act {act}: fp32 formula worst |err| / bound {worst:.3f}; bias {mean:+.5f} ulp of +-{bound:.5f} over {n} elements")
    assert worst <= 1.0 and abs(mean) <= bound and n >= 50000
    wrong = R.rne_bf16(R.act_f32(x, act, c=1.70) if act else R.act_f32(x, act, tanh=True)).double()
    m2, _, _ = R.act_bias(wrong, want)
    print(f"act {act}: {'1.70 for 1.702' if act else 'tanh-GELU'}: bias {m2:+.5f} ulp")
    assert abs(m2) > bound
    if act == 0:        # 1 + erf cancels below x = -3: the per-element bound sees it, the bias bound does not have to
        cancels = R.rne_bf16(0.5 * x * (1.0 + torch.erf(x * 0.70710678118654752))).double()
        assert ((cancels - want).abs() / R.act_bound(want)).max().item() > 10.0


def test_activation_extremes():
    x = torch.tensor([0.0, -0.0, 80.0, -80.0, 8.0, -8.0])
    for act in (0, 1):
        y = R.rne_bf16(R.act_f32(x, act))
        assert bool(torch.isfinite(y).all()) and y[2].item() == 80.0 and y[3].item() == 0.0 and y[0].item() == 0.0 and y[1].item() == 0.0


# ------------------------------------------------------------------------------------------------ pointwise
@pytest.mark.parametrize("cin,cout", [(8, 8), (4, 4), (3, 5)])
def test_pointwise_case_is_exact_in_fp32(cin, cout):
    x, w, bias = R.pointwise_case(2, cin, cout, 257)
    want = R.pointwise(x, w, bias)
    # fp32, channel order, as the kernel adds: the same bits as fp64
    a = bias[None, :, None].expand(2, cout, 257).clone()
    for c in range(cin):
        a = a + w[:, c][None, :, None] * x[:, c][:, None, :]
    assert torch.equal(a, want)
    w2 = w.clone()
    w2[cout - 1, cin - 1] += 1
    assert not torch.equal(R.pointwise(x, w2, bias), want)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_entries_are_declared_exported_and_validate_before_launch():
    from mvd_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "mvd_hip.h")).read()
    lib = L.lib()
    for name in ENTRIES:
        assert name + "(" in hdr and name in L.EXPORTED_SYMBOLS and hasattr(lib, name), name
    fake = 0x10000
    err = lambda rc, text: rc < 0 and text in L.last_error()       # noqa: E731
    for tower in ("text", "vision"):
        add_ln = getattr(lib, f"mvd_op_{tower}_add_ln")
        assert err(add_ln(fake, None, fake, fake, 4, 2052, 1e-5, fake, None, None), "H = 2052")
        assert err(add_ln(fake, None, fake, fake, 4, 6, 1e-5, fake, None, None), "H = 6")
        assert err(add_ln(fake, None, fake, fake, 4, 64, 1e-5, fake, fake, None), "exactly one")
        assert err(add_ln(fake, None, fake, fake, 4, 64, 1e-5, None, None, None), "exactly one")
        assert err(add_ln(None, None, fake, fake, 4, 64, 1e-5, fake, None, None), "null")
        assert err(add_ln(fake + 4, None, fake, fake, 4, 64, 1e-5, fake, None, None), "aligned")
        act = getattr(lib, f"mvd_op_{tower}_act")
        assert err(act(fake, 12, 0, fake, None), "multiple of 8") and err(act(fake, 8, 2, fake, None), "act 2") and err(act(None, 8, 0, fake, None), "null")
    assert err(lib.mvd_op_text_embed(fake, fake, fake, 4, 2, 66, 10, fake, None), "multiple of 4")
    assert err(lib.mvd_op_text_embed(fake, fake, fake, 4, 0, 64, 10, fake, None), "bad shape")
    assert err(lib.mvd_op_vit_patchify(fake, 1, 30, 8, fake, None), "bad shape")
    assert err(lib.mvd_op_vit_embed_ln(fake, fake, fake, fake, fake, 1, 5, 2052, 1e-5, fake, None), "H = 2052")
    assert err(lib.mvd_op_vit_embed_ln(None, fake, fake, fake, fake, 1, 5, 64, 1e-5, fake, None), "null")
    assert err(lib.mvd_op_vit_fold(fake, fake, 6, fake, None), "multiple of 4")
    assert err(lib.mvd_op_clip_l2norm(fake, 1, 2049, None), "at most 2048")
    assert err(lib.mvd_op_vae_pointwise(fake, 2, 9, 8, 16, fake, fake, fake, None), "at most 8 channels")
    assert err(lib.mvd_op_vae_pointwise(fake, 2, 8, 9, 16, fake, fake, fake, None), "at most 8 channels")
    assert err(lib.mvd_op_clip_pool_project(fake, None, None, 1, 1, 2052, 2, None, None, 1e-5, fake, 64, fake, fake, None), "bad shape")
    assert err(lib.mvd_op_clip_pool_project(fake, None, None, 1, 1, 64, 2, None, None, 1e-5, fake, 2049, fake, fake, None), "bad shape")
    assert err(lib.mvd_debug_clip_linear(fake, 100, 4, fake, None, 64, fake, 0, None, 0, None, None), "multiples of 64")
    assert lib.mvd_debug_clip_linear_ws_bytes(0, 64, 64, 0) < 0
    assert lib.mvd_debug_clip_linear_ws_bytes(77, 1024, 1024, 1) >= 0
    assert err(lib.mvd_debug_clip_attention(None, fake, 1, 2, 5, None), "bad argument")
