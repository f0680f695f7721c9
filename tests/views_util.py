"""Inputs and ORACLE results for V views of one object (N14), shared by tests/test_views_cpu.py and tests/test_views_gpu.py.

Plain helper module (like parity_util.py), no fixtures; nothing here touches the code under test."""
import functools
from types import SimpleNamespace

import torch


@functools.lru_cache(maxsize=8)
def views_case(V, g, hw=16, img_ref_scale=0.3, wrong=False, seed=0):
    """One object seen from V cameras, g rows per view (1, or 2 under guidance), inputs built as parity_util.make_inputs builds
    them (seed 0 is its default): ``sample`` (g V, 4, h, w) in the pipeline's order [uncond x V | cond x V] = ``[latents] * g``,
    ``text`` (g, 7, xdim), ``lat`` (1, ...), ``src`` / ``tgt`` (V, 4, 4), ``proj``, ``t``.

    ``want``: the V independent oracle calls of batch g with the one-row reference, rows scattered to r = j V + v -- the
    definition of the shared forward.  ``wrong=True`` adds the two ways today's interface can batch the views, one batch-gV
    oracle call with the source repeated V (``rep_v``) or g V (``rep_gv``) times, and their rel-L2 distances to ``want``
    (``d_rep_v``, ``d_rep_gv``)."""
    from oracle import mvd as OM
    from oracle import sd21_unet as OU
    from tests.parity_util import make_inputs, rel_l2
    cfg = OU.UNetConfig.tiny()
    params = OM.init_mvd_params(cfg, 0, cam_dim=96, cam_hidden=48)
    inp = make_inputs(cfg, 2 * V, hw, 7, seed=seed, cam_dim=96)
    sample = torch.cat([inp["sample"][:V]] * g)
    text = inp["text"][:g]
    lat = inp["lat"][:1]
    src, tgt = inp["src"][:V], inp["tgt"][:V]
    t = torch.tensor(321)
    kw = dict(fourier_proj=inp["proj"], img_ref_scale=img_ref_scale, cam_modulation_strength=0.2)
    want = torch.empty_like(sample)
    for v in range(V):
        rows = [j * V + v for j in range(g)]
        want[rows] = OM.multiview_unet_forward(params, cfg, sample[rows], t, text, src[v:v + 1], tgt[v:v + 1], lat, **kw)
    c = SimpleNamespace(cfg=cfg, params=params, V=V, g=g, sample=sample, text=text, lat=lat, src=src, tgt=tgt, proj=inp["proj"], t=t,
                        want=want)
    if wrong:
        text_rows = text.repeat_interleave(V, 0)            # row j V + v gets text row j
        cams = dict(source_camera=src.repeat(g, 1, 1), target_camera=tgt.repeat(g, 1, 1))
        for name, n in (("rep_v", V), ("rep_gv", g * V)):
            out = OM.multiview_unet_forward(params, cfg, sample, t, text_rows, source_image_latents=lat.repeat(n, 1, 1, 1), **cams, **kw)
            setattr(c, name, out)
            setattr(c, "d_" + name, rel_l2(out, want))
    return c
