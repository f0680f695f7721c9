"""Inputs and ORACLE results for ragged turntables -- O objects with V_o views each in one forward (N16) -- shared by
tests/test_ragged_cpu.py, tests/test_ragged_gpu.py and tests/test_exact_attention_mapped_gpu.py.

Plain helper module (like objects_util.py), no fixtures; nothing here touches the code under test."""
import functools
from types import SimpleNamespace

import torch


def offsets(counts):
    """first view index of every object inside a guidance half, and R"""
    offs, r = [], 0
    for v in counts:
        offs.append(r)
        r += v
    return offs, r


def row(counts, j, o, v):
    """main-batch row of (guidance half j, object o, view v): [uncond x R | cond x R], object-major inside a half"""
    offs, R = offsets(counts)
    return j * R + offs[o] + v


def object_of(counts):
    """object of every view index c = 0 .. R - 1"""
    return [o for o, n in enumerate(counts) for _ in range(n)]


def adapter_table(counts, g):
    """K/V element (object-major, o g + j) that main-batch row r = j R + c reads"""
    return [o * g + j for j in range(g) for o in object_of(counts)]


def text_table(counts, g):
    """text row (j O + o) that main-batch row r = j R + c reads"""
    return [j * len(counts) + o for j in range(g) for o in object_of(counts)]


def uniform_object_of(counts):
    """the object every view index is booked to when the uniform map of V = R // O views per object is forced onto the ragged
    batch (kv_group = V, kv_objects = O): c // V"""
    _, R = offsets(counts)
    V = R // len(counts)
    return [min(c // V, len(counts) - 1) for c in range(R)]


def ragged_views(p, counts, g, nq):
    """(q (g R, nq, C), k, v (O g, nk, C), want (g R, nq, C)) of the routing problem p (exact_util.routing_problem) over O g
    elements with max(counts) * nq queries each: the K/V stay as they are, element o g + j; batch row (j, o, v) takes queries
    [v nq, (v + 1) nq) of element o g + j and wants their rows (attention is per query, so a subset of an element's queries
    keeps its wanted rows)"""
    E, n, C = p.q.shape
    assert E == len(counts) * g and n == max(counts) * nq
    qs, ws = [], []
    for j in range(g):
        for o, V in enumerate(counts):
            for v in range(V):
                qs.append(p.q[o * g + j, v * nq:(v + 1) * nq])
                ws.append(p.want[o * g + j, v * nq:(v + 1) * nq])
    return torch.stack(qs).contiguous(), p.k, p.v, torch.stack(ws).contiguous()


def view_rows(R, g, c):
    """the g main-batch rows of view index c"""
    return [j * R + c for j in range(g)]


def per_row(got, want):
    """rel-L2 of every main-batch row"""
    from tests.parity_util import rel_l2
    return [rel_l2(got[r], want[r]) for r in range(want.shape[0])]


@functools.lru_cache(maxsize=8)
def ragged_case(counts, g, hw=16, img_ref_scale=0.3, amp=1.0, wrong=False, seed=0):
    """O objects, object o seen from counts[o] cameras, g rows per view (1, or 2 under guidance); inputs built as
    parity_util.make_inputs builds them: ``sample`` (g R, 4, h, w) = ``[latents] * g`` with latents row c, ``text`` (g O, 7, xdim) =
    [negative x O | positive x O], ``lat`` (O, ...) with the rows of objects 1.. multiplied by ``amp``, ``src`` / ``tgt`` (R, 4, 4)
    (``src`` row c is object o's source camera: one per object), ``proj``, ``t``.  ``hw``: an int, or an (H, W) pair.

    ``want``: the R independent oracle calls of batch g with a one-row reference, rows scattered to r = j R + c -- the definition
    of the ragged forward.  ``wrong=True`` adds what else could be computed, each with its rel-L2 distance to ``want``:
    ``rep`` / ``d_rep``: one ordinary oracle call of the g R rows with every view's own source repeated to R rows (what the
    validation run's batch computes today); ``uniform`` / ``d_uniform``: the independent calls with every view answered from
    the REFERENCE of the object the uniform map books it to (uniform_object_of; its own text rows -- the nearer of the two
    possible faults); ``misrouted``: the view indices that map gets wrong, ``d_misrouted``: per such view the rel-L2 over its g rows."""
    from oracle import mvd as OM
    from oracle import sd21_unet as OU
    from tests.parity_util import make_inputs, rel_l2
    cfg = OU.UNetConfig.tiny()
    params = OM.init_mvd_params(cfg, 0, cam_dim=96, cam_hidden=48)
    O = len(counts)
    _, R = offsets(counts)
    obj = object_of(counts)
    inp = make_inputs(cfg, max(2 * R, g * O), hw, 7, seed=seed, cam_dim=96)
    sample = torch.cat([inp["sample"][:R]] * g)
    text = inp["text"][:g * O]
    lat = inp["lat"][:O].clone()
    lat[1:] *= amp
    src = inp["src"][:O][obj].clone()
    tgt = inp["tgt"][:R]
    t = torch.tensor(321)
    kw = dict(fourier_proj=inp["proj"], img_ref_scale=img_ref_scale, cam_modulation_strength=0.2)

    def independent(ref_of):
        out = torch.empty_like(sample)
        for c in range(R):
            rows = [j * R + c for j in range(g)]
            o, ref = obj[c], ref_of[c]
            out[rows] = OM.multiview_unet_forward(params, cfg, sample[rows], t, text[[j * O + o for j in range(g)]], src[c:c + 1],
                                                  tgt[c:c + 1], lat[ref:ref + 1], **kw)
        return out

    want = independent(obj)
    c = SimpleNamespace(cfg=cfg, params=params, counts=counts, O=O, R=R, g=g, sample=sample, text=text, lat=lat, src=src, tgt=tgt,
                        proj=inp["proj"], t=t, want=want)
    if wrong:
        text_rows = torch.cat([text[[j * O + o for o in obj]] for j in range(g)])     # row j R + c gets text row j O + o
        c.rep = OM.multiview_unet_forward(params, cfg, sample, t, text_rows, source_camera=src.repeat(g, 1, 1),
                                          target_camera=tgt.repeat(g, 1, 1), source_image_latents=lat[obj], **kw)
        c.d_rep = rel_l2(c.rep, want)
        uni = uniform_object_of(counts)
        c.misrouted = [i for i in range(R) if uni[i] != obj[i]]
        c.uniform = independent(uni)
        c.d_uniform = rel_l2(c.uniform, want)
        c.d_misrouted = [rel_l2(c.uniform[view_rows(R, g, i)], want[view_rows(R, g, i)]) for i in c.misrouted]
    return c
