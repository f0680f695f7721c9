"""Inputs and ORACLE results for O objects x V views in one forward (N15), shared by tests/test_objects_cpu.py and
tests/test_objects_gpu.py.

Plain helper module (like views_util.py), no fixtures; nothing here touches the code under test."""
import functools
from types import SimpleNamespace

import torch


def row(O, V, j, o, v):
    """main-batch row of (guidance half j, object o, view v): the pipeline's order [uncond x O V | cond x O V], object-major"""
    return j * O * V + o * V + v


def element_of(q, O, g):
    """K/V element (object-major, o g + j) that batch group q = j O + o reads: MvdAttnArgs::kv_objects"""
    return (q % O) * g + q // O


def object_views(p, O, V, g):
    """(q (g O V, nq, C), k, v (O g, nk, C), want (g O V, nq, C)) of the routing problem p (exact_util.routing_problem) over
    O g elements with V * nq queries each: the K/V stay as they are, element o g + j; the queries and the wanted rows go from
    element-major order to the batch's [j][o][v]"""
    E, n, C = p.q.shape
    assert E == O * g and n % V == 0

    def to_batch(x):
        return x.reshape(O, g, V, n // V, C).permute(1, 0, 2, 3, 4).reshape(g * O * V, n // V, C).contiguous()

    return to_batch(p.q), p.k, p.v, to_batch(p.want)


@functools.lru_cache(maxsize=8)
def objects_case(O, V, g, hw=16, img_ref_scale=0.3, amp=1.0, wrong=False, seed=0):
    """O objects seen from V cameras each, g rows per view (1, or 2 under guidance), inputs built as parity_util.make_inputs
    builds them: ``sample`` (g O V, 4, h, w) = ``[latents] * g`` with latents row o V + v, ``text`` (g O, 7, xdim) =
    [negative x O | positive x O], ``lat`` (O, ...) with the rows of objects 1.. multiplied by ``amp`` (sources that differ in
    scale move batch-coupled statistics), ``src`` / ``tgt`` (O V, 4, 4), ``proj``, ``t``.

    ``want``: the O V independent oracle calls of batch g with a one-row reference, rows scattered to r = j O V + o V + v -- the
    definition of the object forward.  ``wrong=True`` adds what else could be computed, each with its rel-L2 distance to
    ``want``: one ordinary batch-g O V oracle call with every row's own source, the sources repeated to O V rows (``rep_v``,
    ``d_rep_v``) or to g O V rows (``rep_gv``, ``d_rep_gv``), and the independent calls with object o answered from object
    o + 1's reference (``swapped``, ``d_swapped``)."""
    from oracle import mvd as OM
    from oracle import sd21_unet as OU
    from tests.parity_util import make_inputs, rel_l2
    cfg = OU.UNetConfig.tiny()
    params = OM.init_mvd_params(cfg, 0, cam_dim=96, cam_hidden=48)
    n = O * V
    inp = make_inputs(cfg, max(2 * n, g * O), hw, 7, seed=seed, cam_dim=96)
    sample = torch.cat([inp["sample"][:n]] * g)
    text = inp["text"][:g * O]
    lat = inp["lat"][:O].clone()
    lat[1:] *= amp
    src, tgt = inp["src"][:n], inp["tgt"][:n]
    t = torch.tensor(321)
    kw = dict(fourier_proj=inp["proj"], img_ref_scale=img_ref_scale, cam_modulation_strength=0.2)

    def independent(ref_of):
        out = torch.empty_like(sample)
        for o in range(O):
            for v in range(V):
                rows = [row(O, V, j, o, v) for j in range(g)]
                c = o * V + v
                out[rows] = OM.multiview_unet_forward(params, cfg, sample[rows], t, text[[j * O + o for j in range(g)]], src[c:c + 1],
                                                      tgt[c:c + 1], lat[ref_of(o):ref_of(o) + 1], **kw)
        return out

    want = independent(lambda o: o)
    c = SimpleNamespace(cfg=cfg, params=params, O=O, V=V, g=g, sample=sample, text=text, lat=lat, src=src, tgt=tgt, proj=inp["proj"], t=t,
                        want=want)
    if wrong:
        text_rows = text.repeat_interleave(V, 0)            # row j O V + o V + v gets text row j O + o
        cams = dict(source_camera=src.repeat(g, 1, 1), target_camera=tgt.repeat(g, 1, 1))
        per_view = lat.repeat_interleave(V, 0)              # (O V, ...): row o V + v holds object o's source
        for name, rows in (("rep_v", per_view), ("rep_gv", per_view.repeat(g, 1, 1, 1))):
            out = OM.multiview_unet_forward(params, cfg, sample, t, text_rows, source_image_latents=rows, **cams, **kw)
            setattr(c, name, out)
            setattr(c, "d_" + name, rel_l2(out, want))
        c.swapped = independent(lambda o: (o + 1) % O)
        c.d_swapped = rel_l2(c.swapped, want)
    return c
