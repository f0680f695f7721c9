"""The fp32 camera / time conditioning path, operator by operator and row by row, against the float64 references of
tests/conditioning_ref.py.  Every bound is fixed by the reference (or by a float32 emulation of the kernel's own formula, run on
the CPU by tests/test_conditioning_ref_cpu.py) before the kernel runs; none is tuned to the kernel.  The shapes are the smallest
that reach each code path: a second loop trip (half = 129 > 128 threads, 3 * 170 > 256 threads, c = 257 and 1024 > 256), the
scalar / vector / matrix-pipe forms of the linear layers (k = 9, misaligned or unaligned rows, 8 rows and more), ragged tiles,
more than one 32-row tile (40 rows), segment ends on and off the 32-feature tile.

Which form of a linear launcher ran is not reported by the library (there is no ``mvd_debug_last_*`` for the skinny launchers):
the tests derive it from the launchers' rule -- the matrix-pipe form from 8 rows up when the rows are 16-byte aligned (and, grouped,
every inner segment end is a multiple of 32), the vector form otherwise, the scalar form when a row is not 16-byte aligned or
k % 4 != 0 -- and check the rule's visible consequence: with DebugFlag.SKINNY_VECTOR set, a vector-form case returns the same bits
(same kernel), a matrix-pipe case is only held to the bound."""
import pytest
import torch

from tests import conditioning_ref as CR
from tests.exact_util import round_f64_to_bf16, ulp_distance

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture(scope="module")
def ops():
    from mvd_amd import ops as O
    return O


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def err(got, want):
    return (got.detach().cpu().double() - want).abs()


class vector_form:
    """DebugFlag.SKINNY_VECTOR for the block, restored on the way out"""

    def __enter__(self):
        from mvd_amd import _lib as L
        L.lib().mvd_debug_set_flags(int(L.DebugFlag.SKINNY_VECTOR))

    def __exit__(self, *exc):
        from mvd_amd import _lib as L
        L.lib().mvd_debug_set_flags(0)


# ------------------------------------------------------------------------------------------------ timestep_embedding
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("dim", CR.TIMESTEP_DIMS)
def test_timestep_embedding(ops, dim, batch):
    """[cos | sin] of t * 10000^(-i / half) within |ang| (3 + |arg|) 2^-23 + 2^-23 of float64 (a float32 emulation of the formula
    stays at 0.435 of it on the CPU); half = 129 takes a second trip of the 128-thread loop; distinct t per row.
    Measured on the device: worst error / bound 0.435 (dim 320), the emulation's own figure."""
    vals = CR.TIMESTEP_VALUES
    worst = 0.0
    for k in range(len(vals)):
        t = torch.tensor([vals[(k + j) % len(vals)] for j in range(batch)])
        want, ang, arg = CR.timestep_embedding(t, dim)
        got = ops.timestep_embedding(t.cuda(), dim)
        assert got.shape == (batch, dim)
        ratio = err(got, want) / CR.timestep_embedding_bound(ang, arg)
        worst = max(worst, ratio.max().item())
        assert (ratio <= 1.0).all(), (dim, batch, t.tolist(), ratio.max().item())
    print(f"timestep_embedding dim={dim} batch={batch}: worst error / bound = {worst:.3f}")


# ------------------------------------------------------------------------------------------------ camera_features
@pytest.mark.parametrize("batch", [1, 5])
@pytest.mark.parametrize("nfreq", CR.CAMERA_NFREQ)
def test_camera_features(ops, nfreq, batch):
    """General (not orthonormal) 3x3 blocks and non-zero translations, so that sR tR^T, a missing transpose or T = tT - sT R are
    first-order errors.  Entries on the 1/8 grid make R and T exact in fp32: rflat must then be bit-exact, and the Fourier
    features [axis][sin nfreq | cos nfreq] are held to the sinusoid bound on an exact T (emulation on the CPU: 0.424 of it).
    The fourth row of 4x4 cameras is filled with 1e30: it must not matter, 3x4 and 4x4 give the same bits.  Full-precision entries:
    rflat within 4 ulp of the sum of its terms' magnitudes.  Measured on the device: worst error / bound 0.424 (nfreq 170)."""
    src, tgt = CR.random_cameras(batch, 3, seed=batch, grid=True)
    cf = CR.camera_features(src, tgt, nfreq)
    rflat, enc = ops.camera_features(src.cuda(), tgt.cuda(), nfreq)
    assert rflat.shape == (batch, 9) and enc.shape == (batch, 6 * nfreq)
    assert torch.equal(rflat.cpu().double(), cf["rflat"])
    ratio = err(enc, cf["enc"]) / CR.camera_features_bound(cf["ang"], cf["arg"])
    print(f"camera_features nfreq={nfreq} batch={batch}: worst error / bound = {ratio.max().item():.3f}")
    assert (ratio <= 1.0).all(), ratio.max().item()
    sentinel = torch.full((batch, 1, 4), 1e30)
    rflat4, enc4 = ops.camera_features(torch.cat([src, sentinel], 1).cuda(), torch.cat([tgt, -sentinel], 1).cuda(), nfreq)
    assert same(rflat4, rflat) and same(enc4, enc)
    src, tgt = CR.random_cameras(batch, 4, seed=batch)
    cf = CR.camera_features(src, tgt, nfreq)
    rflat, _ = ops.camera_features(src.cuda(), tgt.cuda(), nfreq)
    assert (err(rflat, cf["rflat"]) <= CR.rflat_bound(cf["rflat_mag"])).all()


# ------------------------------------------------------------------------------------------------ layernorm_f32
@pytest.mark.parametrize("c,rows,silu", CR.LN_CASES)
def test_layernorm_f32(ops, c, rows, silu):
    """bound = 4 x the worst error of the two-pass float32 emulation against float64, per case (0.9e-6 to 2.8e-6; measured on the
    device: 0.11 to 0.30 of it)"""
    x, gamma, beta = CR.ln_case(c, rows, silu)
    want = CR.layernorm_f32(x, gamma, beta, 1e-5, silu)
    bound = CR.layernorm_bound(x, gamma, beta, 1e-5, silu)
    got = ops.layernorm_f32(x.cuda(), gamma.cuda(), beta.cuda(), 1e-5, silu)
    e = err(got, want).max().item()
    print(f"layernorm_f32 c={c} rows={rows} silu={silu}: error {e:.3e}, bound {bound:.3e}")
    assert e <= bound, (e, bound)


def test_layernorm_f32_grouped_affine(ops):
    """nseg = 9, rows = 3 * 9: row r takes gamma / beta of segment r % 9, every segment's different from every other's by O(0.1)"""
    x, gamma, beta = CR.ln_case(48, 27, True, nseg=9)
    want = CR.layernorm_f32(x, gamma, beta, 1e-5, True, 9)
    bound = CR.layernorm_bound(x, gamma, beta, 1e-5, True, 9)
    got = ops.layernorm_f32(x.cuda(), gamma.cuda(), beta.cuda(), 1e-5, True, nseg=9)
    assert err(got, want).max().item() <= bound
    for r in (0, 8, 9, 26):      # the same row alone with its segment's affine: same bits (a row is a workgroup)
        alone = ops.layernorm_f32(x[r:r + 1].cuda(), gamma[r % 9].cuda(), beta[r % 9].cuda(), 1e-5, True)
        assert same(alone[0], got[r])


def test_layernorm_f32_mean_100_probe(ops):
    """rows of mean 100, deviation 0.1: a variance taken as E[x^2] - mean^2 in fp32 misses this bound (3.2e-4) by 1000 x (CPU test);
    measured on the device: 7.1e-5"""
    x = CR.layernorm_probe()
    c = x.shape[1]
    gamma, beta = torch.ones(c), torch.zeros(c)
    want = CR.layernorm_f32(x, gamma, beta)
    bound = CR.layernorm_bound(x, gamma, beta)
    got = ops.layernorm_f32(x.cuda(), gamma.cuda(), beta.cuda())
    e = err(got, want).max().item()
    print(f"layernorm_f32 mean-100 probe: error {e:.3e}, bound {bound:.3e}")
    assert e <= bound, (e, bound)


# ------------------------------------------------------------------------------------------------ skinny_linear, the untested forms
def _lin_case(batch, k, n, seed, bias=True):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(batch, k, generator=g)
    w = torch.randn(n, k, generator=g) / k ** 0.5
    b = torch.randn(n, generator=g) if bias else None
    return x, w, b


SENTINEL = 0x7FC12345     # a NaN payload no kernel produces


def _sentinel(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)


@pytest.mark.parametrize("batch", [3, 8])
def test_skinny_linear_k9_and_no_bias(ops, batch):
    """k = 9 (the rotation input: not a multiple of 4, the scalar kernel at every batch) and no bias (the Fourier projection)"""
    x, w, b = _lin_case(batch, 9, 50, batch)
    want = CR.linear(x, w, b)
    assert err(ops.skinny_linear(x.cuda(), w.cuda(), b.cuda()), want).max().item() <= CR.linear_bound(want)
    x, w, _ = _lin_case(batch, 96, 97, batch + 1, bias=False)
    want = CR.linear(x, w)
    assert err(ops.skinny_linear(x.cuda(), w.cuda()), want).max().item() <= CR.linear_bound(want)


@pytest.mark.parametrize("batch", [3, 8])
def test_skinny_linear_strided_and_misaligned_inputs(ops, batch):
    """x a view one float into its buffer (rows not 16-byte aligned: the launcher must leave the 16-byte-load forms), ldx > k
    (ldx a multiple of 4: still the fast forms; not a multiple: the scalar kernel); all right, and the aligned dense call agrees"""
    k, n = 48, 40
    x, w, b = _lin_case(batch, k, n, 10 + batch)
    want = CR.linear(x, w, b)
    bound = CR.linear_bound(want)
    buf = torch.zeros(batch * k + 1, device="cuda")
    buf[1:] = x.reshape(-1).cuda()
    xm = buf[1:].view(batch, k)
    assert xm.data_ptr() % 16 == 4
    assert err(ops.skinny_linear(xm, w.cuda(), b.cuda()), want).max().item() <= bound
    for pad in (8, 3):
        wide = torch.full((batch, k + pad), 1e4, device="cuda")      # what lies between the rows must not be read into the sum
        wide[:, :k] = x.cuda()
        xv = wide[:, :k]
        assert xv.stride(0) == k + pad
        assert err(ops.skinny_linear(xv, w.cuda(), b.cuda()), want).max().item() <= bound, pad


@pytest.mark.parametrize("batch", [3, 8])
def test_skinny_linear_ldy_writes_only_its_half(ops, batch):
    """ldy = 2 n, as the engine writes the two halves of its concatenated layer input: each call fills its columns and leaves
    the other half's sentinel bits alone"""
    k, n = 48, 40
    x, w, b = _lin_case(batch, k, n, 20 + batch)
    want = CR.linear(x, w, b)
    for half in (0, 1):
        cat = _sentinel(batch, 2 * n)
        got = ops.skinny_linear(x.cuda(), w.cuda(), b.cuda(), out=cat[:, half * n:(half + 1) * n])
        assert got.stride(0) == 2 * n
        assert err(cat[:, half * n:(half + 1) * n], want).max().item() <= CR.linear_bound(want)
        other = cat[:, (1 - half) * n:(2 - half) * n]
        assert (bits(other) == SENTINEL).all()
    assert same(got.contiguous(), ops.skinny_linear(x.cuda(), w.cuda(), b.cuda()))


def test_skinny_linear_33_rows_in_the_vector_form(ops):
    """33 rows under DebugFlag.SKINNY_VECTOR: the vector kernel's second 32-row pass holds one row"""
    x, w, b = _lin_case(33, 96, 50, 33)
    want = CR.linear(x, w, b)
    with vector_form():
        got = ops.skinny_linear(x.cuda(), w.cuda(), b.cuda())
    assert err(got, want).max().item() <= CR.linear_bound(want)
    assert err(ops.skinny_linear(x.cuda(), w.cuda(), b.cuda()), want).max().item() <= CR.linear_bound(want)


# ------------------------------------------------------------------------------------------------ skinny_linear_grouped
SEG_TABLES = {
    "on32_ragged": [64, 192, 200],            # inner ends on 32, the last tile ragged
    "off32": [6, 70, 78],                     # inner ends off 32: the vector form even at 8 rows
    "one": [72],
    "sixteen": [32 * (i + 1) for i in range(16)],
}


def grouped_form(seg_end, batch):
    """the launcher's rule (misc.hip mvd_launch_skinny_linear_grouped)"""
    return "mfma" if batch >= 8 and all(e % 32 == 0 for e in seg_end[:-1]) else "vector"


def _grouped_case(k, seg_end, batch, seed=0):
    g = torch.Generator().manual_seed(k + 13 * len(seg_end) + seg_end[0] + seed)
    x = torch.randn(batch, len(seg_end) * k, generator=g)         # every segment's input drawn independently: a wrong one is O(1) off
    w = torch.randn(seg_end[-1], k, generator=g) / k ** 0.5
    b = torch.randn(seg_end[-1], generator=g)
    return x, w, b


@pytest.mark.parametrize("batch", [1, 7, 8, 11, 40])
@pytest.mark.parametrize("table", list(SEG_TABLES))
@pytest.mark.parametrize("k", [48, 512])
def test_skinny_linear_grouped(ops, k, table, batch):
    """xseg = k, ldx = nseg * k (the engine's layout) against float64 at the dense test's 2e-5 max(1, max|want|); the form is derived
    from the launcher's rule (module docstring): a vector-form case is bit-identical with the vector flag set"""
    seg_end = SEG_TABLES[table]
    x, w, b = _grouped_case(k, seg_end, batch)
    want = CR.linear_grouped(x, w, seg_end, b)
    got = ops.skinny_linear_grouped(x.cuda(), w.cuda(), seg_end, b.cuda())
    assert err(got, want).max().item() <= CR.linear_bound(want)
    with vector_form():
        vec = ops.skinny_linear_grouped(x.cuda(), w.cuda(), seg_end, b.cuda())
    assert err(vec, want).max().item() <= CR.linear_bound(want)
    if grouped_form(seg_end, batch) == "vector":
        assert same(vec, got)


# ------------------------------------------------------------------------------------------------ film_params
FILM_DIMS = (4, 32, 8)
FILM_SEG = [8, 72, 88]


def _raw(batch, seed):
    g = torch.Generator().manual_seed(700 + seed)
    raw = 2.0 * torch.randn(batch, FILM_SEG[-1], generator=g)
    raw[:, 0], raw[:, 1], raw[:, 9], raw[:, 73] = 100.0, -100.0, -100.0, 100.0      # saturated sigmoids in every segment's scale half
    return raw


@pytest.mark.parametrize("strength", [0.2, 1.0])
@pytest.mark.parametrize("batch,out_rows", [(2, 2), (2, 4), (3, 6), (1, 5)])
def test_film_params_and_grouped(ops, batch, out_rows, strength):
    """scale = 2 strength sigmoid, shift = strength raw, output row r from raw row r % batch.  The scale is held to 4 fp32 ulp (exp,
    the sum, the quotient: 3 roundings at most half an ulp to one ulp each), the shift -- one product -- to its single rounding,
    bit for bit; raw = +-100 gives exactly 2 strength and 0.  The grouped layout (segment g at out_rows * seg_end[g-1], dims 4, 32,
    8) against the same reference; grouped and ungrouped agree to 1 ulp (on the device: bit-equal, printed)."""
    s32 = torch.tensor(strength, dtype=torch.float32).item()          # the float the kernel receives
    raw = _raw(batch, batch * 10 + out_rows)
    flat = ops.film_params_grouped(raw.cuda(), FILM_SEG, strength, out_rows).cpu()
    assert torch.isfinite(flat).all() and flat.numel() == out_rows * FILM_SEG[-1]
    want_pairs = CR.film_params_grouped(raw, FILM_SEG, s32, out_rows)
    all_equal, o0, off = True, 0, 0
    for (wsc, wsh), o1, dim in zip(want_pairs, FILM_SEG, FILM_DIMS):
        sc, sh = ops.film_params(raw[:, o0:o1].contiguous().cuda(), strength, out_rows)
        gsc = flat[off:off + out_rows * dim].view(out_rows, dim)
        gsh = flat[off + out_rows * dim:off + 2 * out_rows * dim].view(out_rows, dim)
        for got_sc, got_sh in ((sc.cpu(), sh.cpu()), (gsc, gsh)):
            assert torch.isfinite(got_sc).all() and torch.isfinite(got_sh).all()
            assert (err(got_sc, wsc) <= 4.0 * CR.ulp32(wsc) + 2.0 ** -126).all()      # (+ a subnormal result may be flushed)
            assert same(got_sh, wsh.float())
            sat_hi, sat_lo = raw[:, o0:o0 + dim] == 100.0, raw[:, o0:o0 + dim] == -100.0
            sel = torch.arange(out_rows) % batch
            assert (got_sc[sat_hi[sel]] == 2.0 * s32).all() and (got_sc[sat_lo[sel]].abs() <= 2.0 ** -126).all()
            assert sat_hi.any() or sat_lo.any()
            for r in range(out_rows):
                assert same(got_sc[r], got_sc[r % batch]) and same(got_sh[r], got_sh[r % batch])
        assert (err(gsc, sc.cpu().double()) <= CR.ulp32(sc.cpu().double())).all() and same(gsh, sh)
        all_equal = all_equal and same(gsc, sc)
        o0, off = o1, off + 2 * out_rows * dim
    print(f"film_params batch={batch} out_rows={out_rows} strength={strength}: grouped == ungrouped bit for bit: {all_equal}")


# ------------------------------------------------------------------------------------------------ im2col_in
@pytest.mark.parametrize("hw", [(1, 1), (3, 5), (8, 8)])
@pytest.mark.parametrize("C", [1, 3, 4, 7])
def test_im2col_in(ops, C, hw):
    """Without FiLM every one of the 64 columns is bit-exact: the source pixel rounded once to bf16, +0 for padding taps and for
    columns 9 C .. 63.  With FiLM (ld_ss 0 = one scale row for all batch rows, 4, 8): padding taps stay +0 (not ``shift``), interior
    values within 1 bf16 ulp of the float64 x * scale + shift rounded once, and under 1 % of them differ from it at all (both
    fp32 forms stay under it on the CPU; measured on the device: no element of these cases, printed)."""
    h, w = hw
    g = torch.Generator().manual_seed(C * 100 + h * 10 + w)
    x = torch.randn(2, C, h, w, generator=g)
    val, inside = CR.im2col_in(x)
    got = ops.im2col_in(x.cuda())
    assert got.shape == (2, h, w, 64) and got.dtype == torch.bfloat16
    assert same(got, round_f64_to_bf16(val))
    assert (bits(got)[~inside] == 0).all() and (bits(got)[..., 9 * C:] == 0).all()
    for ld_ss in (0, 4, 8):
        xf, scale, shift = CR.im2col_film_case(C, h, w, ld_ss)
        val, inside = CR.im2col_in(xf, scale, shift, ld_ss)
        want = round_f64_to_bf16(val)
        got = ops.im2col_in(xf.cuda(), scale.cuda(), shift.cuda(), ld_ss).cpu()
        assert (bits(got)[~inside] == 0).all()
        dist = ulp_distance(got, want)
        share = (dist[inside] != 0).double().mean().item()
        print(f"im2col_in C={C} {h}x{w} ld_ss={ld_ss}: {100 * share:.2f} % of the interior elements off the single rounding")
        assert dist.max() <= 1 and share < 0.01, (ld_ss, int(dist.max()), share)


# ------------------------------------------------------------------------------------------------ film_nchw_f32
@pytest.mark.parametrize("batch,c,hw", [(2, 4, 1), (3, 64, 6)])
def test_film_nchw_f32(ops, batch, c, hw):
    """within 1 fp32 ulp of the float64 x * scale + shift"""
    g = torch.Generator().manual_seed(batch + c + hw)
    x, sc, sh = torch.randn(batch, c, hw, generator=g), torch.randn(batch, c, generator=g), torch.randn(batch, c, generator=g)
    want = CR.film_nchw_f32(x, sc, sh)
    got = ops.film_nchw_f32(x.cuda(), sc.cuda(), sh.cuda())
    assert (err(got, want) <= CR.ulp32(want)).all()


# ================================================================================================ row semantics
BATCHES_LOW, BATCHES_HIGH = (1, 3, 7), (8, 11, 40)      # one form of the linear layers / the other (the matrix pipe from 8 rows up)


def _check_rows(run):
    """``run(n, replace)`` computes the first n rows (``replace``: {row kept: ...} -> the other rows replaced by 1e4-scale noise).
    Row r's bits are the same in a batch of 1, 3 or 7, the same in a batch of 8, 11 or 40, and the same with noisy neighbours."""
    for group in (BATCHES_LOW, BATCHES_HIGH):
        outs = {n: run(n, None) for n in group}
        for a in group:
            for b in group:
                if a < b:
                    assert same(outs[a], outs[b][:a]), (a, b)
        n, keep = group[-1], group[-1] // 2
        noisy = run(n, keep)
        assert same(noisy[keep], outs[n][keep]), (n, keep)
        assert not same(noisy, outs[n])


def test_rows_are_independent_in_the_linear_layers(ops):
    """skinny_linear (fp32 and bf16 weights) and skinny_linear_grouped: a row's result does not depend on how many rows share the
    launch within one form (1 / 3 / 7 rows, and 8 / 11 / 40), nor on what the other rows hold"""
    g = torch.Generator().manual_seed(41)
    noise = 1e4 * torch.randn(40, 3 * 96, generator=g)

    def mixed(x, n, keep):
        x = x[:n].clone()
        if keep is not None:
            kept = x[keep].clone()
            x = noise[:n, :x.shape[1]].clone()
            x[keep] = kept
        return x.cuda()
    x, w, b = _lin_case(40, 96, 80, 40)
    for wt in (w, w.to(torch.bfloat16)):
        _check_rows(lambda n, keep: ops.skinny_linear(mixed(x, n, keep), wt.cuda(), b.cuda()))
    seg_end = SEG_TABLES["on32_ragged"]
    xg, wg, bg = _grouped_case(96, seg_end, 40)
    _check_rows(lambda n, keep: ops.skinny_linear_grouped(mixed(xg, n, keep), wg.cuda(), seg_end, bg.cuda()))


def test_linear_layers_at_the_7_8_boundary(ops):
    """The same camera gets different bits depending on how many rows share the forward: from 8 rows up the linear layers run on the
    matrix pipe, which sums K in another order.  The same seven rows in a batch of 7 and as the first seven of a batch of 8 differ by
    no more than the dense test's fp32 bound, 2e-5 max(1, max|want|) -- and each is within it of float64."""
    x, w, b = _lin_case(8, 96, 80, 78)
    want = CR.linear(x, w, b)
    y7, y8 = ops.skinny_linear(x[:7].cuda(), w.cuda(), b.cuda()), ops.skinny_linear(x.cuda(), w.cuda(), b.cuda())
    bound = CR.linear_bound(want)
    assert err(y7, want[:7]).max().item() <= bound and err(y8, want).max().item() <= bound
    assert (y7 - y8[:7]).abs().max().item() <= bound
    seg_end = SEG_TABLES["on32_ragged"]
    xg, wg, bg = _grouped_case(48, seg_end, 8)
    want = CR.linear_grouped(xg, wg, seg_end, bg)
    g7 = ops.skinny_linear_grouped(xg[:7].cuda(), wg.cuda(), seg_end, bg.cuda())
    g8 = ops.skinny_linear_grouped(xg.cuda(), wg.cuda(), seg_end, bg.cuda())
    bound = CR.linear_bound(want)
    assert err(g7, want[:7]).max().item() <= bound and err(g8, want).max().item() <= bound
    assert (g7 - g8[:7]).abs().max().item() <= bound
    print(f"7 / 8 boundary: dense rows bit-equal {same(y7, y8[:7])}, grouped rows bit-equal {same(g7, g8[:7])}")


# ------------------------------------------------------------------------------------------------ engines
def _hip_small_cfg():
    from mvd_amd.config import UNetConfig
    return UNetConfig(in_channels=4, out_channels=4, block_out_channels=(64, 128), layers_per_block=1, num_heads=(1, 2),
                      cross_attention_dim=64, norm_num_groups=32, norm_eps=1e-5, sample_size=8)


def _size(eng, rows):
    eng._ensure_workspace(rows, 8, 8, 8, 0, False)


@pytest.fixture(scope="module")
def fixture_engine():
    """the bare camera engine of tests/test_fixtures_gpu._camera_pair("small") with its reference embedding at 40 cameras"""
    from tests.test_fixtures_gpu import _camera_pair
    enc, eng = _camera_pair("small")
    _size(eng, CR.MAX_CAMERAS)
    p, _strength, _names, _dims, src, tgt, proj = CR.camera_case("fixture")
    return enc, eng, src, tgt, proj, CR.camera_embedding(p, src, tgt, proj)


def _small_engine(concat=True):
    from mvd_amd.camera_encoder import CameraEncoder
    from mvd_amd.engine import MVDEngine
    from mvd_amd.packing import pack_camera
    from oracle import mvd as OM
    p, strength, names, dims, src, tgt, proj = CR.camera_case("small")
    enc = CameraEncoder(output_dim=CR.CAM_DIM, hidden_dim=CR.CAM_HIDDEN, modulation_hidden_dims=OM.modulation_hidden_dims(CR.small_cfg()),
                        modulation_strength=strength)
    enc.load_state_dict(p, strict=True)
    eng = MVDEngine(_hip_small_cfg(), CR.CAM_DIM, CR.CAM_HIDDEN, False, strength, device="cuda:0")
    packed = pack_camera(enc.state_dict(), eng.device, 2)
    assert any(k.startswith("cam.modcat.") for k in packed)
    if not concat:      # the per-modulator fallback of the forward's camera path: the concatenated slots are not registered
        packed = {k: v for k, v in packed.items() if not k.startswith("cam.modcat.")}
    eng._register(0, packed)
    enc._engine = eng
    _size(eng, 16)
    return enc, eng


@pytest.fixture(scope="module")
def film_engines():
    """{name: (CameraEncoder mirror, engine, camera_case)}: the small camera engine with every hooked modulator ("small"), the same
    without the concatenated slots ("small_loop"), and the tiny model's engine ("tiny")"""
    from tests.parity_util import build_pair
    res = {"small": _small_engine(True) + (CR.camera_case("small"),), "small_loop": _small_engine(False) + (CR.camera_case("small"),)}
    _ocfg, params, model = build_pair("tiny", 0, CR.CAM_DIM, CR.CAM_HIDDEN)
    eng = model._sync_engine()
    _size(eng, 16)
    case = CR.camera_case("tiny")
    for k, v in case[0].items():          # the derived bounds are about THESE weights
        assert torch.equal(params[f"camera_encoder.{k}"], v), k
    res["tiny"] = (model.camera_encoder, eng, case)
    res["tiny_params"] = params
    return res


def _encode(enc, src, tgt, proj, n, keep=None):
    src, tgt = src[:n].clone(), tgt[:n].clone()
    if keep is not None:
        g = torch.Generator().manual_seed(99)
        ks, kt = src[keep].clone(), tgt[keep].clone()
        src, tgt = 1e4 * torch.randn(src.shape, generator=g), 1e4 * torch.randn(tgt.shape, generator=g)
        src[keep], tgt[keep] = ks, kt
    return enc.encode_cameras(src, tgt, fourier_proj=proj)


def test_encode_cameras_rows_and_batches(fixture_engine):
    """encode_cameras at 8 and 40 cameras (the suite had 2 and 3) against the float64 reference, bound = 8 x the worst difference of
    the float32 torch oracle from it (worst 1.0e-5, bound 8.1e-5; measured on the device: 8.8e-6 at 40 cameras, printed); a camera's embedding has
    the same bits in a batch of 1, 3 or 7, the same in 8, 11 or 40, and with 1e4-scale noise in the other cameras.  The same camera
    gets different bits on the two sides of the 7 / 8 boundary (the matrix-pipe form of the linear layers): both sides are within
    the bound of float64."""
    enc, eng, src, tgt, proj, want = fixture_engine
    bound = CR.conditioning_bounds()["embedding"]
    _check_rows(lambda n, keep: _encode(enc, src, tgt, proj, n, keep))
    for n in (7, 8, 40):
        e = err(_encode(enc, src, tgt, proj, n), want[:n]).max().item()
        print(f"encode_cameras batch={n}: error {e:.3e}, bound {bound:.3e}")
        assert e <= bound, (n, e, bound)
    e7, e8 = _encode(enc, src, tgt, proj, 7), _encode(enc, src, tgt, proj, 8)
    assert (e7 - e8[:7]).abs().max().item() <= 2 * bound
    print(f"encode_cameras 7 / 8 boundary: rows bit-equal {same(e7, e8[:7])}, max difference {(e7 - e8[:7]).abs().max().item():.3e}")


@pytest.mark.parametrize("cam_batch,out_rows", [(1, 1), (1, 2), (3, 6), (8, 16)])
@pytest.mark.parametrize("which", ["small", "small_loop", "tiny"])
def test_engine_film_params(film_engines, which, cam_batch, out_rows):
    """MVDEngine.film_params -- the function the forward's camera path runs: the concatenated modulators (grouped LayerNorm affine,
    grouped linear, grouped FiLM parameters; "small_loop": one modulator at a time, the forward's route without the concatenated
    slots) -- for every hooked modulator against the per-modulator float64 reference; bound = 8 x the float32 torch oracle's worst
    difference from it (worst 2.7e-7, bound 2.2e-6; measured on the device: 1.2e-7 at worst, printed).  Output row r equals row r % cam_batch bit
    for bit, and the stand-alone apply_modulation path (another launch sequence for the same function) returns the same values
    within the bound."""
    enc, eng, (p, strength, names, dims, src, tgt, proj) = film_engines[which]
    bound = CR.conditioning_bounds()["film"]
    emb = CR.camera_embedding(p, src[:cam_batch], tgt[:cam_batch], proj).float()
    got = eng.film_params(emb.cuda(), out_rows)
    assert list(got) == names
    worst = 0.0
    for name in names:
        sc, sh = got[name]
        wsc, wsh = CR.modulator_film(p, name, emb, strength, out_rows)
        assert sc.shape == (out_rows, dims[name]) and sh.shape == sc.shape
        worst = max(worst, err(sc, wsc).max().item(), err(sh, wsh).max().item())
        for r in range(out_rows):
            assert same(sc[r], sc[r % cam_batch]) and same(sh[r], sh[r % cam_batch]), (name, r)
        # apply_modulation on x = 0 and x = 1 gives shift and scale + shift
        x = torch.zeros(cam_batch, dims[name], 1, 2)
        x[..., 1] = 1.0
        y = enc.apply_modulation(x, name, emb).cpu().double()
        assert (y[..., 0, 0] - wsh[:cam_batch]).abs().max().item() <= bound
        assert (y[..., 0, 1] - (wsc + wsh)[:cam_batch]).abs().max().item() <= 2 * bound
    print(f"engine.film_params {which} cam_batch={cam_batch} out_rows={out_rows}: error {worst:.3e}, bound {bound:.3e}")
    assert worst <= bound, (worst, bound)


def test_standalone_film_and_time_entries_check_first():
    """the two stand-alone entry points size their scratch before they launch anything, and a missing weight is an error"""
    import ctypes as C
    from mvd_amd import _lib as L
    _enc, eng = _small_engine()
    tiny_ws = torch.empty(256, dtype=torch.uint8, device="cuda")
    L.call("mvd_engine_bind_workspace", eng._h, C.c_void_p(tiny_ws.data_ptr()), tiny_ws.numel(), None, 0)
    eng._ws, eng._ws_key = tiny_ws, None
    with pytest.raises(L.MvdError, match="workspace too small"):
        eng.film_params(torch.zeros(3, CR.CAM_DIM))
    with pytest.raises(L.MvdError, match="workspace too small"):
        eng.time_projection(torch.zeros(3))
    _size(eng, 4)
    with pytest.raises(L.MvdError, match="missing weight slot"):      # a bare camera engine holds no UNet weights: no silent fallback
        eng.time_projection(torch.zeros(3))
    with pytest.raises(L.MvdError, match="bad argument"):
        eng.film_params(torch.zeros(3, CR.CAM_DIM), out_rows=2)


def test_engine_film_params_rows_and_the_7_8_boundary(film_engines):
    """FiLM parameters of a camera: the same bits in a batch of 1, 3 or 7 cameras, the same in 8, 11 or 40, and with 1e4-scale noise
    in the other embeddings; across the 7 / 8 boundary (matrix-pipe form from 8 rows up) both sides stay within the float64
    reference's bound."""
    enc, eng, (p, strength, names, dims, src, tgt, proj) = film_engines["tiny"]
    _size(eng, CR.MAX_CAMERAS)
    bound = CR.conditioning_bounds()["film"]
    emb = CR.camera_embedding(p, src, tgt, proj).float()
    noise = 1e4 * torch.randn(emb.shape, generator=torch.Generator().manual_seed(5))

    def run(n, keep):
        e = emb[:n].clone()
        if keep is not None:
            e = noise[:n].clone()
            e[keep] = emb[keep]
        out = eng.film_params(e.cuda())
        return torch.cat([torch.cat([out[name][0], out[name][1]], dim=1) for name in names], dim=1)
    _check_rows(run)
    f7, f8 = run(7, None), run(8, None)
    want = torch.cat([torch.cat(CR.modulator_film(p, name, emb[:8], strength), dim=1) for name in names], dim=1)
    assert err(f7, want[:7]).max().item() <= bound and err(f8, want).max().item() <= bound
    print(f"engine.film_params 7 / 8 boundary: rows bit-equal {same(f7, f8[:7])}, max difference {(f7 - f8[:7]).abs().max().item():.3e}")


def test_engine_time_projection(film_engines):
    """MVDEngine.time_projection (the forward's time path: sinusoid, two bf16-weight MLP layers, SiLU stored as bf16, the stacked
    time_emb_proj GEMM) on the tiny model at batch 1, 3 and 8, t in {0, 321, 999}.  The reference holds the engine's storage
    precision (bf16-rounded weights, SiLU(emb) rounded to bf16), so what remains is accumulation order: bound = 8 x the float32
    torch oracle's worst difference on identical stored activations (CPU: worst 8.7e-8), plus one bf16 ulp times |W| for each
    activation that fp32 error can round the other way (conditioning_ref.time_bound; a tenth of them at t = 999, whose fp32 angle
    is 1e-4 off in any evaluation -- the allowance, up to 2e-3, is most of the bound).  Measured on the device: worst error / bound
    0.07.  Rows of equal t are equal bit for bit.  Slices are matched to resnets in the module
    order of the oracle's parameter names."""
    _enc, eng, _case = film_engines["tiny"]
    params = film_engines["tiny_params"]
    base = {k[len("base_unet."):]: v for k, v in params.items() if k.startswith("base_unet.")}
    pb, c0, ts = CR.time_case()
    keys = CR.resnet_keys(base.keys())
    for k in keys:      # the derived bounds are about THESE weights
        assert torch.equal(base[f"{k}.time_emb_proj.weight"].to(torch.bfloat16).float(), pb[f"{k}.time_emb_proj.weight"]), k
    for t in ts:
        want = CR.time_projection(pb, t, c0)
        bounds, figs = CR.time_bound(pb, t, c0)
        got = eng.time_projection(t.cuda())
        assert len(got) == len(keys)
        worst = 0.0
        for i, k in enumerate(keys):
            assert got[i].shape == (t.shape[0], base[f"{k}.time_emb_proj.bias"].shape[0]), k
            ratio = err(got[i], want[i]) / bounds[i]
            worst = max(worst, ratio.max().item())
            assert (ratio <= 1.0).all(), (k, t.tolist(), ratio.max().item())
        full = torch.cat([got[i] for i in range(len(keys))], dim=1)
        for r in range(t.shape[0]):      # rows of equal t are equal bit for bit, whatever their place in the batch
            assert same(full[r], full[r % 3]), r
        print(f"engine.time_projection batch={t.shape[0]}: worst error / bound = {worst:.3f} ({figs})")
