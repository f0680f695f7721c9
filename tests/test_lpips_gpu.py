"""LPIPS on the MI355X: ``mvd_lpips_features`` / ``mvd_lpips_distance`` / ``mvd_op_lpips_head`` and the Python
surface over them against the fp32 restatement of tests/lpips_ref.py, with the synthetic weights and images defined there.

Bounds (none comes from what the kernels give; lpips_ref.case computes them on the CPU):
* the five taps: rel-L2 against the fp32 tower <= 2 x the rel-L2 of the bf16-storage emulation at that tap (2.4e-3 - 4.0e-3 for
  alex, 2.9e-3 - 5.3e-3 for vgg).  The emulation differs from the GPU path in accumulation order only; the factor 2 covers that;
* the normalised-difference maps g_l = sqrt(w_l) (f^x - f^y), from the GPU's taps through the fp64 head on the host, per pair:
  rel-L2 against the fp32 tower's <= eta_l = 2 eps_l, eps_l the emulation's (<= 1.9e-2 on independent pairs, <= 0.19 on close ones);
* the distance: d_l = |g_l|^2 / hw, so given the previous assert |d_gpu - d| <= sum_l d_l (2 eta_l + eta_l^2) + 1e-5 d
  (1.4 - 2.1 % of d on independent pairs, 20 - 27 % on close ones; test_lpips_cpu.py asserts it stays below 0.3 d);
* the head kernel alone against fp64 on the same inputs: <= 1e-5 relative on independent Gaussian maps (per-element fp32
  arithmetic ~4e-7, fp64 sums).
The GPU's taps are asked for pass by pass, as [x of the pass; y of the pass]: the split-K choice of a convolution depends on the
batch (the N8 note in test_perceptual_gpu.py)."""
import pytest
import torch

import lpips_ref as R

pytestmark = pytest.mark.gpu

CASES = [(net, *s) for net in ("alex", "vgg") for s in R.SHAPES[net]]


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def make(net, pairs=1, **kw):
    """the shapes with three pairs run in passes of 2 + 1"""
    from mvd_amd.lpips import LPIPS
    return LPIPS(net=net, backbone=R.backbone(net), model_path=R.synthetic_lins(net), max_pairs_per_pass=2 if pairs == 3 else 8, **kw)


def gpu_taps(metric, c):
    """the GPU's five taps of x and of y (NCHW, on the CPU), computed pass by pass as the distance call does"""
    pairs, pp = c.x.shape[0], metric.max_pairs_per_pass
    tx, ty = [[] for _ in range(5)], [[] for _ in range(5)]
    for p0 in range(0, pairs, pp):
        n = min(pp, pairs - p0)
        taps = metric.features(torch.cat([c.x[p0:p0 + n], c.y[p0:p0 + n]]).cuda())
        for k, t in enumerate(taps):
            tx[k].append(t[:n].float().cpu())
            ty[k].append(t[n:].float().cpu())
    return [torch.cat(t) for t in tx], [torch.cat(t) for t in ty]


@pytest.mark.parametrize("net,pairs,h,w", CASES)
def test_taps(net, pairs, h, w):
    c = R.case(net, pairs, h, w)
    m = make(net)
    taps = m.features(torch.cat([c.x, c.y]).cuda())
    assert len(taps) == 5
    for k, (got, want) in enumerate(zip(taps, c.taps)):
        assert got.shape == want.shape and got.is_cuda and got.dtype == (torch.float32 if (net, k) == ("vgg", 4) else torch.bfloat16), k
        assert got.permute(0, 2, 3, 1).is_contiguous()                       # an NCHW view of the NHWC buffer
        err = R.rel_l2(got.float().cpu(), want)
        print(f"{net} {(pairs, h, w)} tap {k}: GPU rel-L2 {err:.3e}, emulation {c.emu[k]:.3e}, bound {2 * c.emu[k]:.3e}")
        assert err <= 2 * c.emu[k], (k, err, c.emu[k])


@pytest.mark.parametrize("close", [False, True], ids=["independent", "close"])
@pytest.mark.parametrize("net,pairs,h,w", CASES)
def test_difference_maps_and_distance(net, pairs, h, w, close):
    c = R.case(net, pairs, h, w, close)
    m = make(net, pairs)
    tx, ty = gpu_taps(m, c)
    _, _, g = R.head(tx, ty, c.lins)
    for p in range(pairs):
        for k in range(5):
            err = R.rel_l2(g[k][p], c.g[k][p])
            print(f"{net} {(pairs, h, w)} close={close} pair {p} g_{k}: GPU rel-L2 {err:.3e}, emulation {c.eps[p, k].item():.3e}, bound {2 * c.eps[p, k].item():.3e}")
            assert err <= 2 * c.eps[p, k].item(), (p, k, err)
    got = m(c.x.cuda(), c.y.cuda())
    assert got.shape == (pairs, 1, 1, 1) and got.is_cuda and got.dtype == torch.float32
    for p in range(pairs):
        d, bound = c.d[p].item(), c.bound[p] + 1e-5 * c.d[p].item()
        print(f"{net} {(pairs, h, w)} close={close} pair {p}: GPU d {got[p].item():.6e}, fp32 tower {d:.6e}, |dd| {abs(got[p].item() - d):.3e}, bound {bound:.3e}")
        assert abs(got[p].item() - d) <= bound


def head64(xs, ys, ws, relu):
    """fp64 on the same inputs: xs[l], ys[l] (pairs, pixels, C) -> per layer (pairs, layers)"""
    per = []
    for a, b, w, r in zip(xs, ys, ws, relu):
        a, b = a.double().cpu(), b.double().cpu()
        if r:
            a, b = a.clamp_min(0.0), b.clamp_min(0.0)
        ua = a / (a.pow(2).sum(-1, keepdim=True).sqrt() + 1e-10)
        ub = b / (b.pow(2).sum(-1, keepdim=True).sqrt() + 1e-10)
        per.append((w.double().cpu() * (ua - ub).pow(2)).sum(-1).mean(-1))
    return torch.stack(per, 1)


CHANNELS = (64, 128, 192, 256, 384, 512)


@pytest.mark.parametrize("dtype,relu_in", [(torch.bfloat16, False), (torch.float32, True), (torch.float32, False)], ids=["bf16", "fp32_relu", "fp32"])
@pytest.mark.parametrize("pixels", [1, 9, 4097])
def test_head_kernel_alone(pixels, dtype, relu_in):
    """six layers, one per channel count, in one launch; 4097 pixels cross the 256-pixel chunks; three pairs"""
    from mvd_amd import ops
    g = torch.Generator().manual_seed(pixels)
    pairs = 3
    mk = lambda c: torch.randn(pairs, pixels, c, generator=g).to(dtype).cuda()      # noqa: E731
    xs, ys = [mk(c) for c in CHANNELS], [mk(c) for c in CHANNELS]
    ws = [(torch.randn(c, generator=g).abs() / c).cuda() for c in CHANNELS]
    relu = [relu_in] * len(CHANNELS)
    d, per = ops.lpips_head(xs, ys, ws, relu_in=relu, per_layer=True)
    want = head64(xs, ys, ws, relu)
    err = ((per.double().cpu() - want).abs() / want).max().item()
    print(f"head kernel, {pixels} pixels, {dtype}: max relative error per (pair, layer) {err:.3e}")
    assert err <= 1e-5
    assert ((d.double().cpu() - want.sum(1)).abs() / want.sum(1)).max().item() <= 1e-5
    assert abs(per.double().sum(1).cpu() - d.double().cpu()).max().item() <= 1e-6 * d.max().item()
    d2, _ = ops.lpips_head(xs, ys, ws, relu_in=relu)
    assert torch.equal(d2, d)                                                # without per_layer_out, and twice: the same bits
    # mean_out alone (no per-pair output): the fp64 mean of the same per-pair sums, rounded once
    mean, per2 = ops.lpips_head(xs, ys, ws, relu_in=relu, per_layer=True, mean=True)
    assert mean.dim() == 0 and torch.equal(per2, per)
    assert abs(mean.item() - d.double().mean().item()) <= 1e-6 * d.double().mean().item()
    z, zl = ops.lpips_head(xs, [x.clone() for x in xs], ws, relu_in=relu, per_layer=True)
    assert torch.equal(z, torch.zeros_like(z)) and torch.equal(zl, torch.zeros_like(zl))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32_relu"])
def test_head_zero_pixels(dtype):
    """a pixel whose channels are all zero: on one side a finite value (the other side's sum_c w_c f^_c^2), on both sides exactly 0;
    with the ReLU on the way in, a pixel of negative values is such a pixel"""
    from mvd_amd import ops
    g = torch.Generator().manual_seed(9)
    relu = dtype == torch.float32
    x, y = torch.randn(2, 5, 128, generator=g).to(dtype), torch.randn(2, 5, 128, generator=g).to(dtype)
    dead = -x[0, 2].abs() if relu else torch.zeros(128, dtype=dtype)
    x[0, 2] = dead                       # one side
    x[1, 4] = dead
    y[1, 4] = dead                       # both sides
    w = (torch.randn(128, generator=g).abs() / 128)
    d, per = ops.lpips_head([x.cuda()], [y.cuda()], [w.cuda()], relu_in=[relu], per_layer=True)
    want = head64([x], [y], [w], [relu])
    assert torch.isfinite(d).all() and ((per.double().cpu() - want).abs() / want).max().item() <= 1e-5
    # only zero pixels, on both sides: exactly 0, never NaN
    z = dead.reshape(1, 1, 128).expand(2, 3, 128).contiguous().cuda()
    d0, _ = ops.lpips_head([z], [z.clone()], [w.cuda()], relu_in=[relu])
    assert torch.equal(d0, torch.zeros(2, device="cuda"))
    # one dead pixel against a live one, alone: sum_c w_c f^_c^2 of the live side
    d1, _ = ops.lpips_head([z[:1, :1]], [y[:1, :1].cuda()], [w.cuda()], relu_in=[relu])
    want1 = head64([z[:1, :1]], [y[:1, :1]], [w], [relu])
    assert abs(d1.item() - want1.item()) <= 1e-5 * want1.item() and want1.item() > 0.0


@pytest.mark.parametrize("net,pairs,h,w", CASES)
def test_exact_properties(net, pairs, h, w):
    c = R.case(net, pairs, h, w)
    m = make(net, pairs)
    x, y = c.x.cuda(), c.y.cuda()
    zero, zl = m(x, x.clone(), retPerLayer=True)
    assert torch.equal(zero, torch.zeros(pairs, 1, 1, 1, device="cuda"))
    assert all(torch.equal(t, torch.zeros(pairs, 1, 1, 1, device="cuda")) for t in zl) and len(zl) == 5
    a, b = m(x, y), m(x, y)
    assert torch.equal(a, b) and (a > 0).all()
    d, per = m(x, y, retPerLayer=True)
    assert torch.equal(d, a)                                                 # with and without per_layer_out: the same bits
    assert all(t.shape == (pairs, 1, 1, 1) and t.dtype == torch.float32 and t.is_cuda for t in per)
    s = torch.stack(per).double().sum(0)
    assert ((s - d.double()).abs() <= 1e-6 * d.double()).all()
    eta = 2 * c.eps
    for k in range(5):                                                       # the terms are the layers', in order: d_l (2 eta_l + eta_l^2) each
        lim = c.per[:, k] * (2 * eta[:, k] + eta[:, k] ** 2 + 1e-5)
        assert ((per[k].reshape(-1).double().cpu() - c.per[:, k]).abs() <= lim).all(), k


@pytest.mark.parametrize("net,pairs,h,w", [("alex", 3, 64, 64), ("alex", 2, 96, 80), ("vgg", 3, 48, 32)])
def test_surface(net, pairs, h, w):
    c = R.case(net, pairs, h, w)
    m = make(net, pairs)
    # inputs on a 2^-8 grid: (x + 1) / 2 and 2 t - 1 are exact, so normalize=True must give the same bits
    xq, yq = ((c.x * 256).round() / 256).cuda(), ((c.y * 256).round() / 256).cuda()
    plain = m(xq, yq)
    assert plain.shape == (pairs, 1, 1, 1) and plain.dtype == torch.float32 and plain.is_cuda
    assert torch.equal(m((xq + 1) / 2, (yq + 1) / 2, normalize=True), plain)
    assert torch.equal(m(xq.double(), yq.double()), plain)                   # other dtypes are converted
    assert isinstance(plain.mean().item(), float)
    # one-sample slices, as val.py calls the metric: within the distance bound of the batch call and of the fp32 tower
    batch = m(c.x.cuda(), c.y.cuda())
    for p in range(pairs):
        single = m(c.x[p:p + 1].cuda(), c.y[p:p + 1].cuda()).item()
        d, bound = c.d[p].item(), c.bound[p] + 1e-5 * c.d[p].item()
        print(f"{net} {(pairs, h, w)} pair {p}: batch {batch[p].item():.6e}, single call {single:.6e}, fp32 tower {d:.6e}, bound {bound:.3e}")
        assert abs(single - batch[p].item()) <= bound and abs(single - d) <= bound


def test_mean_over_several_passes():
    """mean_out alone through mvd_lpips_distance, over passes of 2 + 1 pairs: the running total in the workspace head.  Each
    per-pair value is an fp64 sum rounded once to fp32 (6e-8) and so is the mean, hence 1e-6"""
    c = R.case("alex", 3, 64, 64)
    m = make("alex", 3)
    x, y = c.x.cuda(), c.y.cuda()
    per = m(x, y).reshape(-1).double()
    mean = m.mean_distance(x, y)
    assert mean.dim() == 0 and mean.is_cuda and mean.dtype == torch.float32
    assert abs(mean.item() - per.mean().item()) <= 1e-6 * per.mean().item()
    assert torch.equal(m.mean_distance(x, y), mean)
    assert m.mean_distance(x, x.clone()).item() == 0.0
    one = m.mean_distance(x[:1], y[:1])                                       # one pass, one pair: the pair's own value
    assert abs(one.item() - per[0].item()) <= 1e-6 * per[0].item()
    v = make("vgg", 3)
    cv = R.case("vgg", 3, 48, 32)
    pv = v(cv.x.cuda(), cv.y.cuda()).reshape(-1).double()
    assert abs(v.mean_distance(cv.x.cuda(), cv.y.cuda()).item() - pv.mean().item()) <= 1e-6 * pv.mean().item()


def test_shorter_last_pass_with_a_deeper_split():
    """15 pairs of 160 x 160 in passes of 8 + 7: conv2 of the 7-pair pass (M = 5054: 237 tiles) is split two ways along K, that of
    the 8-pair pass (M = 5776) is not, so the shorter pass needs partials the full one does not.  The workspace is bound with
    exactly the bytes the sizing call gives for the full pass, inside a larger buffer of a sentinel byte: nothing beyond it may be
    written, and every pair stays inside its distance bound"""
    import ctypes as C
    from mvd_amd import _lib as L
    pairs, size, guard = 15, 160, 1 << 23
    c = R.case("alex", pairs, size, size)
    m = make("alex", pairs)
    assert m.max_pairs_per_pass == 8
    x, y = c.x.cuda(), c.y.cuda()
    m._sync(x.device)
    need = L.lib().mvd_lpips_workspace_bytes(m._handle.h, 16, size, size)
    assert need > 0 and all(L.lib().mvd_lpips_workspace_bytes(m._handle.h, 2 * n, size, size) <= need for n in range(1, 9))
    buf = torch.full((need + guard,), 0x5A, dtype=torch.uint8, device="cuda")
    L.call("mvd_lpips_bind_workspace", m._handle.h, C.c_void_p(buf.data_ptr()), need)
    m._handle.ws = buf[:need]                                                # (the object finds a workspace of the size it asks for and keeps it)
    got = m(x, y)
    assert m._handle.ws.data_ptr() == buf.data_ptr()
    assert bool((buf[need:] == 0x5A).all()), "a pass wrote beyond the bound workspace"
    for p in range(pairs):
        d, bound = c.d[p].item(), c.bound[p] + 1e-5 * c.d[p].item()
        assert abs(got[p].item() - d) <= bound, (p, got[p].item(), d, bound)
    mean = m.mean_distance(x, y)
    assert abs(mean.item() - got.double().mean().item()) <= 1e-6 * got.double().mean().item()
    assert bool((buf[need:] == 0x5A).all())
    # a workspace that holds fewer pairs than the cap: smaller passes, the same bound; one too small for a pair: refused, nothing launched
    small = L.lib().mvd_lpips_workspace_bytes(m._handle.h, 6, size, size)
    L.call("mvd_lpips_bind_workspace", m._handle.h, C.c_void_p(buf.data_ptr()), small)
    out = torch.empty(pairs, device="cuda")
    L.call("mvd_lpips_distance", m._handle.h, C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), pairs, size, size, 8, C.c_void_p(out.data_ptr()),
           None, None, None)
    assert bool((buf[small:] == 0x5A).all())
    assert all(abs(out[p].item() - c.d[p].item()) <= c.bound[p] + 1e-5 * c.d[p].item() for p in range(pairs))
    L.call("mvd_lpips_bind_workspace", m._handle.h, C.c_void_p(buf.data_ptr()), 4096)
    rc = L.lib().mvd_lpips_distance(m._handle.h, C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), pairs, size, size, 8, C.c_void_p(out.data_ptr()),
                                    None, None, None)
    assert rc == -4 and "too small" in L.last_error()
    L.call("mvd_lpips_bind_workspace", m._handle.h, C.c_void_p(buf.data_ptr()), need)


def test_errors_on_the_device():
    from mvd_amd._lib import MvdError
    m = make("alex")
    x = torch.zeros(1, 3, 32, 32, device="cuda")
    with pytest.raises(MvdError, match="must match"):
        m(x, torch.zeros(1, 3, 32, 48, device="cuda"))
    with pytest.raises(MvdError, match="31 x 31"):
        m(x[:, :, :30], x[:, :, :30])
    assert m(x, x).item() == 0.0
