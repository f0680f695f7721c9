"""The CLIP towers' and the VAE's own kernels one by one on the GPU (mvd_amd/ops.py: clip_add_ln, clip_act, text_embed,
vit_patchify, vit_embed_ln, vit_fold, clip_l2norm, vae_pointwise; clip_score.pool_project), against the fp64 references and
with the bounds of tests/clip_ops_ref.py -- every bound is one the project already had (listed there); tests/test_clip_ops_cpu.py
shows on the CPU that these inputs and bounds catch the faults they are meant for.  clip_layer.h is compiled into text.hip and
vision.hip: add + LayerNorm and the activation run through both copies (``tower``).  Every test prints its worst error as a
fraction of its bound before it asserts; DESIGN.md section 9 (rows N5 / N7) records the figures."""
import pytest
import torch

from tests import clip_ops_ref as R
from tests import clip_vision_ref as V
from tests import conditioning_ref as CR
from tests import stat_probe as P

pytestmark = pytest.mark.gpu
TOWERS = ("text", "vision")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mvd_amd import ops as O
    return O


def _padded(t, extra=2):
    """a device copy of the 2-D ``t`` with ``extra`` sentinel rows behind it"""
    buf = torch.full((t.shape[0] + extra, t.shape[1]), R.SENTINEL, dtype=t.dtype, device="cuda")
    buf[:t.shape[0]] = t.cuda()
    return buf


def _sentinel_ok(buf, rows):
    return bool((buf[rows:].float() == R.SENTINEL).all())


# ------------------------------------------------------------------------------------------------ add + LayerNorm
@pytest.mark.parametrize("H", R.ADD_LN_H)
@pytest.mark.parametrize("tower", TOWERS)
def test_add_ln(ops, tower, H):
    worst = 0.0
    for rows in R.ADD_LN_ROWS:
        x, delta, gamma, beta = R.add_ln_case(H, rows)
        g, b = gamma.cuda(), beta.cuda()
        for dl in (None, delta):
            after, want, bound = R.add_ln_ref(x, dl, gamma, beta)
            d = None if dl is None else _padded(dl)
            xb = _padded(x)
            y32 = torch.full((rows + 2, H), R.SENTINEL, device="cuda")
            ops.clip_add_ln(xb, d, g, b, R.EPS, True, tower, rows=rows, out=y32)
            err = (y32[:rows].double().cpu() - want).abs().max().item()
            worst = max(worst, err / bound)
            what = f"{tower} add+LN H={H} rows={rows} delta={'given' if dl is not None else 'null'}"
            assert torch.isfinite(y32).all() and err <= bound, f"{what}: max-abs {err:.3g} > bound {bound:.3g}"
            assert R.same_bits(xb[:rows], after), f"{what}: x afterwards is not fl32(x + delta)" if dl is not None else f"{what}: x was touched"
            assert _sentinel_ok(xb, rows) and _sentinel_ok(y32, rows), f"{what}: rows behind `rows` were written"
            # the same launch again gives the same bits; the bf16 launch is the fp32 result rounded once
            xb2, y2 = _padded(x), torch.full_like(y32, R.SENTINEL)
            ops.clip_add_ln(xb2, d, g, b, R.EPS, True, tower, rows=rows, out=y2)
            assert R.same_bits(y2, y32) and R.same_bits(xb2, xb), f"{what}: two launches differ"
            xb3 = _padded(x)
            y16 = torch.full((rows + 2, H), R.SENTINEL, device="cuda", dtype=torch.bfloat16)
            ops.clip_add_ln(xb3, d, g, b, R.EPS, False, tower, rows=rows, out=y16)
            assert R.same_bits(y16[:rows], R.rne_bf16(y32[:rows])), f"{what}: the bf16 output is not the fp32 output rounded to nearest even"
            assert R.same_bits(xb3, xb) and _sentinel_ok(y16, rows), what
    print(f"\n[clip-ops] {tower} add+LN H={H}: worst |err| / layernorm_bound {worst:.3f} over rows {R.ADD_LN_ROWS}, delta null and given")


@pytest.mark.parametrize("tower", TOWERS)
def test_add_ln_refuses_what_the_kernel_cannot_take(ops, tower):
    from mvd_amd._lib import MvdError
    z = lambda h, dt=torch.float32: torch.zeros(4, h, device="cuda", dtype=dt)      # noqa: E731
    keep = z(64).clone()
    for H, text in ((2052, "H = 2052"), (6, "H = 6")):
        with pytest.raises(MvdError, match=text):
            ops.clip_add_ln(z(H), None, z(H)[0].contiguous(), z(H)[0].contiguous(), tower=tower)
    from mvd_amd import _lib as L
    x, g, y32, y16 = z(64), z(64)[0].contiguous(), z(64), z(64, torch.bfloat16)
    rc = getattr(L.lib(), f"mvd_op_{tower}_add_ln")(x.data_ptr(), None, g.data_ptr(), g.data_ptr(), 4, 64, 1e-5, y16.data_ptr(), y32.data_ptr(), None)
    assert rc < 0 and "exactly one" in L.last_error()
    torch.cuda.synchronize()
    assert torch.equal(x, keep) and torch.equal(y32, keep)


@pytest.mark.parametrize("H", R.ADD_LN_H)
@pytest.mark.parametrize("tower", TOWERS)
def test_add_ln_spike_probe(ops, tower, H):
    """the hot element in x or in delta by (row + launch + tower) parity: over the two towers every column is hot in both"""
    rows, flip = R.PROBE_ROWS, TOWERS.index(tower)
    slots = R.probe_slots(H, rows)
    lay = P.Rows(rows, H)
    gamma, beta = R.probe_affine(H)
    gam, bet = (t.cuda() for t in lay.affine(gamma, beta))
    g, b = gamma.cuda(), beta.cuda()
    worst = [0.0, 0.0]
    for i in range(len(slots)):
        first, second = R.probe_pair(H, rows, slots[i], i, flip)
        x, d = first.cuda(), second.cuda()
        got = ops.clip_add_ln(x, d, g, b, R.EPS, tower == "vision", tower)
        s = (first + second).cuda()
        assert R.same_bits(x, s), f"{tower} add+LN probe H={H}, launch {i}: x afterwards is not fl32(x + delta)"
        r = P.check(got, P.reference(s, R.EPS, gam, bet), slots[i].cuda(), lay, f"{tower} add+LN H={H}, launch {i}")
        worst = [max(worst[0], r[0]), max(worst[1], r[1])]
    print(f"\n[clip-ops] {tower} add+LN spike probe H={H}: {len(slots)} launches, {slots.numel()} positions, worst hot {worst[0]:.3f}, "
          f"worst non-hot {worst[1]:.3f} of the limit")


@pytest.mark.parametrize("tower", TOWERS)
def test_add_ln_mean_100_probe(ops, tower):
    """rows of mean 100 and deviation 0.1 (conditioning_ref.layernorm_probe): E[x^2] - mean^2 would lose every digit of the variance"""
    for c in (256, 1280):
        x = CR.layernorm_probe(3, c)
        gamma, beta = R.affine(c)
        for dl in (None, (0.01 * torch.randn(3, c, generator=R.gen(c, 9))).float()):
            after, want, bound = R.add_ln_ref(x, dl, gamma, beta)
            got = ops.clip_add_ln(x.cuda(), None if dl is None else dl.cuda(), gamma.cuda(), beta.cuda(), R.EPS, True, tower)
            err = (got.double().cpu() - want).abs().max().item()
            print(f"\n[clip-ops] {tower} add+LN mean-100 c={c} delta={'given' if dl is not None else 'null'}: max-abs {err:.3g}, bound {bound:.3g} "
                  f"({err / bound:.3f})")
            assert err <= bound


# ------------------------------------------------------------------------------------------------ ViT embedding + pre-LayerNorm
@pytest.mark.parametrize("B,T,H", R.EMBED_LN_CASES)
def test_vit_embed_ln(ops, B, T, H):
    po, cls, pos, gamma, beta = R.embed_ln_case(B, T, H)
    rows = R.embed_rows(po, cls, pos, B)
    want, bound = CR.layernorm_f32(rows, gamma, beta, R.EPS), CR.layernorm_bound(rows, gamma, beta, R.EPS)
    args = [t.cuda() for t in (po, cls, pos, gamma, beta)]
    got = ops.vit_embed_ln(*args, B, R.EPS)
    err = (got.double().cpu() - want).abs().max().item()
    print(f"\n[clip-ops] vit_embed_ln B={B} T={T} H={H}: max-abs {err:.3g}, layernorm_bound {bound:.3g} ({err / bound:.3f})")
    assert torch.isfinite(got).all() and err <= bound
    tok0 = got.view(B, T, H)[:, 0]
    assert all(R.same_bits(tok0[b], tok0[0]) for b in range(B)), "token 0 differs between images"
    assert R.same_bits(ops.vit_embed_ln(*args, B, R.EPS), got), "two launches differ"


@pytest.mark.parametrize("H", R.EMBED_LN_PROBE_H)
def test_vit_embed_ln_spike_probe(ops, H):
    """B = 1: the hot element of row 0 in cls or pos[0], of a patch row in patch_out or pos"""
    T = R.PROBE_ROWS
    slots = R.probe_slots(H, T)
    lay = P.Rows(T, H)
    gamma, beta = R.probe_affine(H)
    gam, bet = (t.cuda() for t in lay.affine(gamma, beta))
    g, b = gamma.cuda(), beta.cuda()
    worst = [0.0, 0.0]
    for i in range(len(slots)):
        first, second = R.probe_pair(H, T, slots[i], i)
        got = ops.vit_embed_ln(first[1:].contiguous().cuda(), first[0].contiguous().cuda(), second.cuda(), g, b, 1, R.EPS)
        r = P.check(got, P.reference((first + second).cuda(), R.EPS, gam, bet), slots[i].cuda(), lay, f"vit_embed_ln H={H}, launch {i}")
        worst = [max(worst[0], r[0]), max(worst[1], r[1])]
    print(f"\n[clip-ops] vit_embed_ln spike probe H={H}: {len(slots)} launches, {slots.numel()} positions, worst hot {worst[0]:.3f}, "
          f"worst non-hot {worst[1]:.3f} of the limit")


# ------------------------------------------------------------------------------------------------ index kernels
@pytest.mark.parametrize("H", [64, 1280])
@pytest.mark.parametrize("T", [1, 20, 77])
def test_text_embed(ops, T, H):
    rows = 2 * T + 1                                     # 3, 41, 155: never a multiple of the four rows of a workgroup
    ids, tok, pos = R.text_embed_case(rows, T, H)
    if rows > 4:
        ids[2], ids[3] = -1, tok.shape[0]                # pinned to the documented clamp: rows 0 and vocab - 1
    want = R.text_embed(ids, tok, pos, T)
    out = torch.full((rows + 2, H), R.SENTINEL, device="cuda")
    ops.text_embed(ids.cuda(), tok.cuda(), pos.cuda(), T, out=out)
    assert R.same_bits(out[:rows], want), f"text_embed T={T} H={H}: {int((out[:rows].cpu() != want).sum())} elements differ"
    assert _sentinel_ok(out, rows)
    if rows > 4:
        assert R.same_bits(out[2], tok[0] + pos[2 % T]) and R.same_bits(out[3], tok[-1] + pos[3 % T])
    print(f"\n[clip-ops] text_embed rows={rows} T={T} H={H}: bit-exact")


def test_vit_fold(ops):
    n = 4 * (3 * 256 + 5)                                # ragged against 256 float4 per workgroup
    g = R.gen(n)
    x, d = torch.randn(n + 8, generator=g), torch.randn(n + 8, generator=g)
    out = torch.full((n + 8,), R.SENTINEL, device="cuda")
    ops.vit_fold(x.cuda(), d.cuda(), n=n, out=out)
    assert R.same_bits(out[:n], (x + d)[:n]) and bool((out[n:] == R.SENTINEL).all())
    out4 = ops.vit_fold(x[:4].cuda(), d[:4].cuda())
    assert R.same_bits(out4, (x + d)[:4])
    print(f"\n[clip-ops] vit_fold n={n} and n=4: bit-exact")


@pytest.mark.parametrize("S,P_", [(32, 8), (28, 14), (224, 32)])
def test_vit_patchify(ops, S, P_):
    pv = V.seeded_pixel_values(dict(image_size=S), 2, seed=S)
    want = R.patch_rows_bf16(pv, P_)
    got = ops.vit_patchify(pv.cuda(), P_)
    assert R.same_bits(got, want), f"vit_patchify S={S} P={P_}: {int((got.cpu() != want).sum())} elements differ"
    assert bool((got[:, 3 * P_ * P_:] == 0).all())
    print(f"\n[clip-ops] vit_patchify S={S} P={P_}: {tuple(got.shape)} bit-exact, pad columns zero")


# ------------------------------------------------------------------------------------------------ activation
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("tower", TOWERS)
def test_act(ops, tower, act):
    x = R.act_inputs()
    want = R.act64(x, act)
    worst = 0.0
    for n8 in (1, 255, 257, 8192 + 1):
        n = 8 * n8
        out = torch.full((n + 8,), R.SENTINEL, device="cuda", dtype=torch.bfloat16)
        ops.clip_act(x[:n + 8].cuda(), act, tower, n=n, out=out)
        got = out[:n].double().cpu()
        assert bool(torch.isfinite(got).all()) and bool((out[n:].float() == R.SENTINEL).all()), (tower, act, n8)
        ratio = ((got - want[:n]).abs() / R.act_bound(want[:n])).max().item()
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"{tower} act {act} n8={n8}: worst |err| / bound {ratio:.3g}"
    got = ops.clip_act(x.cuda(), act, tower).double().cpu()
    ratio = ((got - want).abs() / R.act_bound(want)).max().item()
    mean, bound, n = R.act_bias(got, want)
    print(f"\n[clip-ops] {tower} act {act}: worst |err| / bound {max(worst, ratio):.3f}; bias {mean:+.5f} ulp of +-{bound:.5f} over {n} elements")
    assert ratio <= 1.0 and abs(mean) <= bound
    ext = torch.tensor([0.0, -0.0, 80.0, -80.0, 1.0, -1.0, 40.0, -40.0])
    y = ops.clip_act(ext.cuda(), act, tower).float().cpu()
    assert bool(torch.isfinite(y).all()) and y[0].item() == 0.0 and y[1].item() == 0.0 and y[2].item() == 80.0 and y[3].item() == 0.0, y.tolist()
    assert bool(((y.double() - R.act64(ext, act)).abs() <= R.act_bound(R.act64(ext, act))).all()), y.tolist()


# ------------------------------------------------------------------------------------------------ pool / project / L2 normalisation
@pytest.mark.parametrize("H", [64, 1280, 2048])
def test_pool_project_edges(ops, H):
    from mvd_amd.clip_score import pool_project
    worst = 0.0
    for proj in (4, 66, 1027, 2048):
        g = R.gen(H, proj)
        B, T = 3, 1
        hid, dl = torch.randn(B, T, H, generator=g), 0.1 * torch.randn(B, T, H, generator=g)
        w = torch.randn(proj, H, generator=g) / H ** 0.5
        gamma, beta = R.affine(H)
        raw, nrm = pool_project(hid.cuda(), w.cuda(), delta=dl.cuda(), ln=(gamma.cuda(), beta.cuda()))
        want, wn = R.pool_project(hid, dl, gamma, beta, w)
        e1 = ((raw.cpu().double() - want).abs().max() / want.abs().max()).item()
        e2 = (nrm.cpu().double() - wn).abs().max().item()
        worst = max(worst, e1, e2)
        assert torch.isfinite(raw).all() and max(e1, e2) <= 1e-5, f"pool/project H={H} proj={proj}: raw {e1:.3g}, normalised {e2:.3g}"
    print(f"\n[clip-ops] pool/project H={H}, proj 4 / 66 / 1027 / 2048, T=1: worst error {worst:.3g} of 1e-5")


@pytest.mark.parametrize("H", R.POOL_PROBE_H)
def test_pool_layernorm_spike_probe(ops, H):
    """the pool kernel's LayerNorm seen through an identity projection (every product and sum exact): token 0 of hidden + delta,
    the token behind it poisoned"""
    from mvd_amd.clip_score import pool_project
    B = R.PROBE_ROWS
    slots = R.probe_slots(H, B)
    lay = P.Rows(B, H)
    gamma, beta = R.probe_affine(H)
    gam, bet = (t.cuda() for t in lay.affine(gamma, beta))
    ln = (gamma.cuda(), beta.cuda())
    eye = torch.eye(H, device="cuda")
    worst = [0.0, 0.0]
    for i in range(len(slots)):
        first, second = R.probe_pair(H, B, slots[i], i)
        hid = torch.full((B, 2, H), float("nan"), device="cuda")
        dl = torch.full((B, 2, H), float("nan"), device="cuda")
        hid[:, 0], dl[:, 0] = first.cuda(), second.cuda()
        raw, _ = pool_project(hid, eye, delta=dl, ln=ln)
        r = P.check(raw, P.reference((first + second).cuda(), R.EPS, gam, bet), slots[i].cuda(), lay, f"pool LN H={H}, launch {i}")
        worst = [max(worst[0], r[0]), max(worst[1], r[1])]
    print(f"\n[clip-ops] pool LayerNorm spike probe H={H}: {len(slots)} launches, {slots.numel()} positions, worst hot {worst[0]:.3f}, "
          f"worst non-hot {worst[1]:.3f} of the limit")


@pytest.mark.parametrize("dim", [4, 66, 2048])
def test_clip_l2norm(ops, dim):
    rows = 5
    x, _ = R.l2norm_case(rows, dim)
    buf = _padded(x, 1)
    ops.clip_l2norm(buf, rows=rows)
    err = (buf[:rows].double().cpu() - R.l2norm(x)).abs().max().item()
    print(f"\n[clip-ops] clip_l2norm dim={dim}: max-abs {err:.3g} of 1e-5")
    assert err <= 1e-5 and _sentinel_ok(buf, rows)


def test_pool_project_refuses_widths_above_its_row_buffer(ops):
    from mvd_amd._lib import MvdError
    from mvd_amd.clip_score import pool_project
    z = lambda *s: torch.zeros(*s, device="cuda")      # noqa: E731
    with pytest.raises(MvdError, match="bad shape"):
        pool_project(z(1, 1, R.LN_MAXH + 4), z(64, R.LN_MAXH + 4))
    with pytest.raises(MvdError, match="bad shape"):
        pool_project(z(1, 1, 64), z(R.LN_MAXH + 1, 64))
    with pytest.raises(MvdError, match="at most 2048"):
        ops.clip_l2norm(z(1, R.LN_MAXH + 1))


# ------------------------------------------------------------------------------------------------ VAE pointwise
@pytest.mark.parametrize("cin,cout", [(8, 8), (4, 4), (3, 5)])
def test_vae_pointwise(ops, cin, cout):
    x, w, bias = R.pointwise_case(2, cin, cout, 257)
    got = ops.vae_pointwise(x.cuda(), w.cuda(), bias.cuda())
    want = R.pointwise(x, w, bias)
    assert R.same_bits(got, want), f"vae pointwise {cin}->{cout}: {int((got.cpu() != want).sum())} elements differ"
    print(f"\n[clip-ops] vae pointwise {cin}->{cout}, B=2, hw=257: bit-exact")


def test_vae_pointwise_refuses_nine_channels(ops):
    from mvd_amd._lib import MvdError
    x, w, bias = torch.zeros(2, 9, 16, device="cuda"), torch.zeros(8, 9, device="cuda"), torch.zeros(8, device="cuda")
    with pytest.raises(MvdError, match="at most 8 channels"):
        ops.vae_pointwise(x, w, bias)
