#!/usr/bin/env python3
"""The launch schedule of every batch layout, as the engine's own per-shape profile records it:
which kernel class ran at which (M, N, K, tag), how often, in order of first appearance.  Times are dropped, so two records are
equal exactly when the two builds launch the same kernels at the same shapes.

Tiny configuration, 16 x 16 latents, text length 7, camera + image conditioning, one forward each of
  plain            B = 2
  views            V = 3, g = 2
  objects          O = 2 x V = 2, g = 2
  ragged_3_2_1     view counts (3, 2, 1), g = 2
  ragged_2_2       view counts (2, 2), g = 1 -- equal counts: the objects forward
  objects_2x2_g1   O = 2 x V = 2, g = 1 -- what ragged_2_2 must equal
through ``MVDEngine.forward`` with ``set_profiling`` / ``profile_shapes``.  ``python tools/record_layout_launch_tables.py OUT.json`` writes the
record (tests/golden/layout_launch_tables.json was written by the commit before the layouts became one value).  Needs the GPU."""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# name -> (sample rows B, text rows, reference rows, camera rows, forward keywords)
FORWARDS = {
    "plain": (2, 2, 2, 2, {}),
    "views": (6, 2, 1, 3, dict(views=3)),
    "objects": (8, 4, 2, 4, dict(views=2, objects=2)),
    "ragged_3_2_1": (12, 6, 3, 6, dict(views=(3, 2, 1))),
    "ragged_2_2": (4, 2, 2, 4, dict(views=(2, 2))),
    "objects_2x2_g1": (4, 2, 2, 4, dict(views=2, objects=2)),
}
_ROW = re.compile(r"cls=(-?\d+) M=(-?\d+) N=(-?\d+) K=(-?\d+) tag=(-?\d+) launches=(\d+) ")


def parse(table: str):
    """[[cls, M, N, K, tag, launches], ..] of a ``profile_shapes`` table, in its order"""
    rows = [[int(v) for v in _ROW.match(line).groups()] for line in table.splitlines()]
    assert rows, "profile_shapes returned no launches"
    return rows


def record(hw: int = 16, text_len: int = 7):
    import torch
    from mvd_amd.config import UNetConfig
    from mvd_amd.engine import MVDEngine
    from mvd_amd.mvd_unet import MultiViewUNet
    from mvd_amd.utils import orbit_cameras
    if not torch.cuda.is_available():
        raise SystemExit("record_layout_launch_tables: needs a GPU")
    torch.manual_seed(0)
    cfg = UNetConfig.tiny()
    model = MultiViewUNet(None, unet_config=cfg, cam_output_dim=96, cam_hidden_dim=48)     # (the weights: shapes only matter here)
    eng = MVDEngine(cfg, 96, 48, cam_modulation_strength=0.2, device="cuda:0")
    eng.load_base(model.base_unet.state_dict(), adapter=True, ref_scale=0.3)
    eng.load_camera(model.camera_encoder.state_dict())
    eng.load_image_encoder(model.image_encoder.unet.state_dict())
    g = torch.Generator().manual_seed(1)
    proj = (torch.randn(96, 96, generator=g) / 96 ** 0.5).cuda()
    tables = {}
    for name, (B, Bt, Br, Bc, kw) in FORWARDS.items():
        x = torch.randn(B, cfg.in_channels, hw, hw, generator=g).cuda()
        text = torch.randn(Bt, text_len, cfg.cross_attention_dim, generator=g).cuda()
        lat = (0.18215 * torch.randn(Br, cfg.in_channels, hw, hw, generator=g)).cuda()
        src, tgt = orbit_cameras(Bc).cuda(), orbit_cameras(Bc, elevation_deg=15.0, start_deg=20.0).cuda()
        eng.set_profiling(1)
        eng.forward(x, torch.full((B,), 500.0, device="cuda"), text, source_camera=src, target_camera=tgt, fourier_proj=proj,
                    source_latents=lat, encoder_text=text[-Br:].contiguous(), **kw)
        torch.cuda.synchronize()
        tables[name] = parse(eng.profile_shapes())
        eng.set_profiling(0)
    return tables


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "layout_launch_tables.json")
    tables = record()
    with open(out, "w") as f:
        f.write("{\n" + ",\n".join(f'"{k}": [\n' + ",\n".join(json.dumps(r) for r in v) + "]" for k, v in tables.items()) + "}\n")
    print({k: (len(v), sum(r[5] for r in v)) for k, v in tables.items()})
