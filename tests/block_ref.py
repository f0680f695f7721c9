"""Teacher-forced reference of the main UNet pass, one block at a time (tests/test_block_parity_cpu.py, test_block_parity_gpu.py).

The engine's main-pass taps (``mvd_engine_set_taps``) hold every block's output.  ``block_want`` runs the ORACLE's function of one
block on that block's own inputs as the engine produced them (its bits, as fp32) and on the conditioning of the case, so that
a block is judged on its own branch and the error of the blocks in front of it stays out:

    || got - want ||  <=  tol * || want - x ||  +  1.25 * || bf16(want) - want ||          (tests/branch_check.py)

``x`` is the block's residual input where it has one of the output's shape (transformers, resnets that keep the channel count)
and 0 elsewhere (conv_in, the samplers, FiLM, resnets with a shortcut convolution, the tail).

Conditioning (``Cond``): the oracle's fp32 time embedding of every row's timestep, the bf16-rounded text, the oracle's camera
embedding and, for the adapter, the encoder feature maps the ENGINE kept (``keep_features``): the reference pass's own error is
not this test's subject.  Q2 normalisation runs over all the reference rows a block's call sees, Q4 re-chunking follows
``oracle.mvd.image_cross_attention`` (which ``adapter_branch`` restates with a row selection; test (a) of the CPU file holds it to
the oracle's forward).

A batch is a list of ``Group``s: the rows that one oracle call computes together.  The ordinary forward is one group of all rows;
the views / objects / ragged forwards are, by definition, independent calls of g rows with a one-row reference each.

``wrong=`` names a wiring fault (``VARIANTS``); ``block_want`` then returns what an engine with that fault would compute, or None
where the fault does not apply to the block.

Token merging and token downsampling (``Cond(tome=, todo=)``): a transformer block that the setting makes eligible
(``unet_params.tome_blocks`` / ``todo_blocks``, held against what the option oracle records) is the OPTION ORACLE's function
(tests/tome_ref.py, tests/todo_ref.py) of the block input -- token merging under the slot tables given (the engine's own decisions,
``MVDEngine.tome_tables()``), token downsampling by its definition.  The adapter's "self" branch stays ``adapter_branch``: on the
merged rows under token merging, on the full rows and the un-pooled reference under token downsampling.  ``OPTION_VARIANTS`` are
the faults of ONE block under an option, expressed through the oracles' own wrong-on-purpose switches.  DeepCache needs nothing
here: a shallow forward's blocks are the same functions, the first re-run up-block resnet reading the stored tensor
(``check_taps(extra=)``).

Plain helper module, no fixtures; nothing here touches the code under test."""
import contextlib
import re
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from oracle import mvd as OM
from oracle import sd21_unet as U

SLACK = 1.25        # branch_check.py's own value
# branch tolerance by block kind (see the docstring of tests/test_block_parity_gpu.py for the measurements behind them)
TOL = {"conv_in": 1e-2, "resnet": 1e-2, "resnet_sc": 1e-2, "attention": 1e-2, "downsampler": 1e-2, "upsampler": 1e-2, "film": 1e-2,
       "tail": 1e-2}

VARIANTS = ("adapter_self_dropped", "adapter_cross_dropped", "adapter_self_other_ref", "adapter_cross_other_ref",
            "adapter_procs_swapped", "adapter_self_out_bias0", "adapter_cross_out_bias0", "text_other_row", "temb_other_row",
            "temb_neighbour_slice", "cat_swapped", "skip_post_film", "film_other_row", "film_neighbour", "freeu_dropped")
# faults of one eligible transformer block under token merging / token downsampling: "<option>_<the oracle's switch>", and
# ``tome_stale_table``: the slot table of the nearest eligible block of the same map in front of this one
OPTION_VARIANTS = {"tome": ("tome_stale_table", "tome_roll_tables", "tome_zero_merged", "tome_merge_cross", "tome_neighbour_row"),
                   "todo": ("todo_corner", "todo_also_ref", "todo_factor_off", "todo_swap_method")}


def bf16(x):
    return x.to(torch.bfloat16).to(torch.float32)


def kind_of(name, ins=None, out=None):
    if name == "conv_in":
        return "conv_in"
    if name == "conv_out":
        return "tail"
    if name.startswith("film."):
        return "film"
    if ".attentions." in name:
        return "attention"
    if ".downsamplers." in name:
        return "downsampler"
    if ".upsamplers." in name:
        return "upsampler"
    assert ".resnets." in name, name
    if ins is not None and (len(ins) > 1 or ins[0].shape[1] != out.shape[1]):
        return "resnet_sc"
    return "resnet"


def feature_of(name):
    """tap name of a transformer -> the feature / hook name of the encoder maps"""
    m = re.fullmatch(r"(down|up)_blocks\.(\d+)\.attentions\.(\d+)", name)
    return f"{m.group(1)}_block_{m.group(2)}_attn_{m.group(3)}" if m else "mid_block_attn_0"


def Group(rows, text_rows=None, ref_rows=None):
    return SimpleNamespace(rows=list(rows), text_rows=list(rows if text_rows is None else text_rows), ref_rows=ref_rows)


class Cond:
    """The conditioning of one forward.  ``t`` (B,) timesteps; ``text`` the text rows as the forward's caller passes them to the
    ENGINE's main pass (one per row, or per guidance half and object in a layout forward); ``cams`` = (src, tgt, proj) or None;
    ``feats`` {feature: (Br, C, H, W)} or None; ``groups``: see the module docstring (default: one group of all rows, every
    reference row).  ``tome`` / ``todo``: the setting (the keywords of ``enable_tome`` / ``enable_todo``) or None, with
    ``latent_hw``; ``tome_tables``: {feature: slot (B, H*W)}, None for the definition's own decisions."""

    def __init__(self, cfg, params, batch, t, text, cams=None, feats=None, groups=None, freeu=None, img_ref_scale=0.3, strength=0.2,
                 round_text=True, tome=None, todo=None, tome_tables=None, latent_hw=None):
        self.cfg, self.B = cfg, batch
        self.tome, self.todo, self.tables, self.latent_hw = tome, todo, tome_tables, latent_hw
        self.merging, self.pooling = {}, {}
        if tome is not None or todo is not None:
            from mvd_amd.config import UNetConfig as HostConfig
            from mvd_amd.unet_params import todo_blocks, tome_blocks
            assert (tome is None or todo is None) and latent_hw is not None
            host = HostConfig(block_out_channels=tuple(cfg.block_out_channels), layers_per_block=cfg.layers_per_block,
                              num_heads=tuple(cfg.num_heads))
            h, w = latent_hw
            if tome is not None:
                self.merging = tome_blocks(host, h, w, tome["ratio"], tome.get("max_downsample", 1))
            else:
                self.pooling = todo_blocks(host, h, w, todo.get("factor", 2), todo.get("factor_level_2", 1))
        self.p = OM._sub(params, "base_unet.")
        self.p_cam = OM._sub(params, "camera_encoder.") if cams is not None else None
        self.scale, self.strength, self.freeu = img_ref_scale, strength, freeu
        t = torch.as_tensor(t, dtype=torch.float32).reshape(-1).expand(batch)
        temb = U.timestep_embedding(t, cfg.block_out_channels[0])
        temb = F.linear(temb, self.p["time_embedding.linear_1.weight"], self.p["time_embedding.linear_1.bias"])
        temb = F.linear(F.silu(temb), self.p["time_embedding.linear_2.weight"], self.p["time_embedding.linear_2.bias"])
        self.temb_act = F.silu(temb)
        self.text = bf16(text) if round_text else text      # (unrounded: only to hold the composition to the oracle's forward)
        self.emb = None
        if cams is not None:
            src, tgt, proj = cams
            emb = OM.camera_embedding(self.p_cam, src, tgt, proj)
            self.emb = emb[[b % emb.shape[0] for b in range(batch)]]          # row b takes camera b % Bc
        self.feats = feats
        nref = next(iter(feats.values())).shape[0] if feats else 0
        self.groups = groups if groups is not None else [Group(range(batch), range(batch), list(range(nref)) if feats else None)]
        # every resnet's slice of the fused time projection, in module order (what the engine's temb_off indexes)
        self.resnets = [k[:-len(".time_emb_proj.weight")] for k in self.p if k.endswith(".time_emb_proj.weight")]

    # ------------------------------------------------------------------ resnets
    def _temb_table(self, temb_act):
        return torch.cat([F.linear(temb_act, self.p[f"{k}.time_emb_proj.weight"], self.p[f"{k}.time_emb_proj.bias"]) for k in self.resnets], 1)

    def resnet(self, key, x, rows, wrong=None):
        temb = self.temb_act
        if wrong == "temb_other_row":
            if self.B < 2:
                return None
            temb = temb.roll(1, 0)
        p = self.p
        if wrong == "temb_neighbour_slice":
            # the slice an off-by-one resnet index reads: this resnet's width at the next resnet's offset (the last: the one before)
            idx = self.resnets.index(key)
            widths = [self.p[f"{k}.conv1.bias"].shape[0] for k in self.resnets]
            nb = idx + 1 if idx + 1 < len(widths) else idx - 1
            off, w = sum(widths[:nb]), widths[idx]
            if off + w > sum(widths):
                off = sum(widths) - w
            tp = self._temb_table(temb)[:, off:off + w]
            p = dict(p)
            p[f"{key}.time_emb_proj.weight"] = torch.zeros_like(p[f"{key}.time_emb_proj.weight"])
            p[f"{key}.time_emb_proj.bias"] = torch.zeros_like(p[f"{key}.time_emb_proj.bias"])
            out = [_resnet_with_tproj(p, key, x[i:i + 1], tp[r:r + 1], self.cfg) for i, r in enumerate(rows)]
            return torch.cat(out)
        return U.resnet_block(p, key, x, temb[rows], self.cfg.norm_num_groups, self.cfg.norm_eps)

    # ------------------------------------------------------------------ transformers
    def transformer(self, name, x, rows, wrong=None):
        """x: the block input of main rows ``rows`` (a subset of the batch, in order)"""
        cfg, feature = self.cfg, feature_of(name)
        heads = x.shape[1] // 64
        ad = self.feats is not None
        if wrong is not None and wrong.startswith("adapter") and not ad:
            return None
        text_all = self.text
        if wrong == "text_other_row":
            if text_all.shape[0] < 2:
                return None
            text_all = text_all.roll(1, 0)
        option = wrong is not None and wrong.startswith(("tome_", "todo_"))
        if option and feature not in (self.merging if wrong.startswith("tome_") else self.pooling):
            return None
        if wrong == "todo_corner" and self.todo.get("method", "nearest") == "area":         # (a mean has no corner)
            return None
        tables = None
        if feature in self.merging and self.tables is not None:
            tables = self.tables[feature]
            if wrong == "tome_stale_table":
                names = list(self.merging)
                same = [n for n in names[:names.index(feature)] if self.merging[n][:2] == self.merging[feature][:2]]
                if not same:
                    return None
                tables = self.tables[same[-1]]
            tables = tables.long().cpu().reshape(self.B, -1)
        elif wrong == "tome_stale_table":
            return None
        out = torch.empty_like(x)
        pos = {r: i for i, r in enumerate(rows)}
        for grp in self.groups:
            sel = [i for i, r in enumerate(grp.rows) if r in pos]           # rows of the group's call that are asked for
            if not sel:
                continue
            here = [pos[grp.rows[i]] for i in sel]
            text = text_all[[grp.text_rows[i] for i in sel]]
            hook = None
            if ad:
                ref_all = self.feats[feature]
                if wrong in ("adapter_self_other_ref", "adapter_cross_other_ref"):
                    if ref_all.shape[0] < 2:
                        return None
                ref = ref_all[grp.ref_rows]
                ref_wrong = ref_all.roll(1, 0)[grp.ref_rows]
            if wrong == "tome_roll_tables" and len(sel) < 2:
                return None
            rec = {}
            with self._option(feature, tables, [grp.rows[i] for i in sel], wrong if option else None, rec) as pool:
                if ad:
                    hook = self._adapter_hook(feature, heads, len(grp.rows), sel, ref, ref_wrong, wrong, pool)
                out[here] = U.transformer_2d(self.p, name, x[here], text, heads, cfg.norm_num_groups, hook, feature)
            self._check_record(feature, rec, tuple(x.shape[-2:]), wrong)
        return out

    def _option(self, feature, tables, rows, wrong, rec):
        """the option oracle's context around one block call of batch rows ``rows`` (yields todo_oracle's ``pool_ref`` or None)"""
        sw = {wrong[5:]: True} if wrong is not None and wrong != "tome_stale_table" else {}
        if self.tome is not None:
            from tests.tome_ref import tome_oracle
            tb = None if tables is None else {feature: tables[rows]}
            return tome_oracle(**self.tome, tables=tb, record=rec, latent_hw=self.latent_hw, **sw)
        if self.todo is not None:
            from tests.todo_ref import todo_oracle
            return todo_oracle(**self.todo, record=rec, latent_hw=self.latent_hw, **sw)
        return contextlib.nullcontext()

    def _check_record(self, feature, rec, hw, wrong):
        """what the oracle did to the block is what ``tome_blocks`` / ``todo_blocks`` say of it"""
        assert set(rec) == ({feature} if feature in self.merging or feature in self.pooling else set()), (feature, sorted(rec))
        if feature in self.merging:
            from tests.tome_ref import geometry
            H, W, r = self.merging[feature]
            dst, src = geometry(H, W)
            slot = rec[feature]
            assert hw == (H, W) and ((slot >= 0) & (slot < H * W - r)).all() and ((slot[:, src] < dst.numel()).sum(dim=1) == r).all(), feature
        if feature in self.pooling and wrong != "todo_factor_off":
            assert hw == self.pooling[feature][:2] and rec[feature] == self.pooling[feature][3], (feature, rec, self.pooling[feature])

    def _adapter_hook(self, feature, heads, Bh, sel, ref, ref_wrong, wrong, pool=None):
        def hook(_feature, kind, hidden, attn_out):
            if wrong == f"adapter_{kind}_dropped":
                return attn_out
            wkind = kind
            if wrong == "adapter_procs_swapped":
                wkind = "cross" if kind == "self" else "self"
            w = OM._sub(self.p, OM._processor_key(feature, wkind) + ".")
            if wrong == f"adapter_{kind}_out_bias0":
                w = dict(w)
                w["to_out_ref.0.bias"] = torch.zeros_like(w["to_out_ref.0.bias"])
            r = ref_wrong if wrong == f"adapter_{kind}_other_ref" else ref
            if pool is not None:                # (todo_also_ref, inside the self hook: the pooled reference; else r itself)
                r = pool(r)
            return attn_out + self.scale * adapter_branch(w, hidden, r, heads, Bh, sel)
        return hook

    # ------------------------------------------------------------------ FiLM
    def film(self, mod, x, rows, wrong=None):
        emb = self.emb
        if wrong == "film_other_row":
            if self.B < 2:
                return None
            emb = emb.roll(1, 0)
        if wrong == "film_neighbour":
            dims = OM.modulation_hidden_dims(self.cfg)
            names = [n for n in dims if n != "mid"]
            i = names.index(mod)
            same = sorted((abs(j - i), n) for j, n in enumerate(names) if n != mod and dims[n] == dims[mod])
            if not same:
                return None
            mod = same[0][1]
        return OM.apply_modulation(self.p_cam, mod, x, emb[rows], self.strength)


def _resnet_with_tproj(p, key, x, tproj, cfg):
    """resnet_block with the time projection given (the block's own projection weights zeroed by the caller)"""
    h = F.silu(U._gn(x, p, f"{key}.norm1", cfg.norm_num_groups, cfg.norm_eps))
    h = F.conv2d(h, p[f"{key}.conv1.weight"], p[f"{key}.conv1.bias"], padding=1)
    h = h + tproj[:, :, None, None]
    h = F.silu(U._gn(h, p, f"{key}.norm2", cfg.norm_num_groups, cfg.norm_eps))
    h = F.conv2d(h, p[f"{key}.conv2.weight"], p[f"{key}.conv2.bias"], padding=1)
    if f"{key}.conv_shortcut.weight" in p:
        x = F.conv2d(x, p[f"{key}.conv_shortcut.weight"], p[f"{key}.conv_shortcut.bias"])
    return x + h


def adapter_branch(w, hidden, ref_nchw, heads, Bh, sel, dim_head=64):
    """``oracle.mvd.image_cross_attention`` for rows ``sel`` of a call whose hidden batch is Bh: Q2 statistics over all rows of
    ``ref_nchw``, the reference tokens re-chunked by Bh (Q4), chunk i answering hidden row i.  ``hidden``: (len(sel), N, C)."""
    ref = OM.normalize_reference(ref_nchw)
    Br, C, H, W = ref.shape
    assert (Br * H * W) % Bh == 0, (Br, H, W, Bh)
    tok = ref.permute(0, 2, 3, 1).reshape(Bh, -1, C)[sel]
    n = len(sel)
    q = F.linear(hidden, w["to_q_ref.weight"]).view(n, -1, heads, dim_head).transpose(1, 2)
    k = F.linear(tok, w["to_k_ref.weight"]).view(n, -1, heads, dim_head).transpose(1, 2)
    v = F.linear(tok, w["to_v_ref.weight"]).view(n, -1, heads, dim_head).transpose(1, 2)
    o = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(n, -1, heads * dim_head)
    return F.linear(o, w["to_out_ref.0.weight"], w["to_out_ref.0.bias"])


def block_want(cond, name, ins, rows=None, wrong=None, taps=None, inputs=None):
    """(want, x): the oracle's output of block ``name`` on the input tensors ``ins`` (rows ``rows`` of the batch; None: all), and
    the residual input (None: 0).  ``wrong``: see ``VARIANTS`` -- returns (None, None) where the fault does not apply.
    ``taps`` / ``inputs`` ({name: tensor of all rows}, {name: input names}): needed by ``skip_post_film`` only."""
    cfg, p = cond.cfg, cond.p
    rows = list(range(cond.B)) if rows is None else list(rows)
    NA = (None, None)
    applies = {"conv_in": ("film_other_row", "film_neighbour"),
               "film": ("film_other_row", "film_neighbour"),
               "attention": tuple(v for v in VARIANTS if v.startswith("adapter")) + ("text_other_row",) + OPTION_VARIANTS["tome"] + OPTION_VARIANTS["todo"],
               "resnet": ("temb_other_row", "temb_neighbour_slice", "cat_swapped", "skip_post_film", "freeu_dropped")}
    kind = kind_of(name)
    if wrong is not None and wrong not in applies.get(kind, ()):
        return NA
    if name == "conv_in":
        x = ins[0]
        if cond.emb is not None:
            x = cond.film("output", x, rows, wrong)
        elif wrong is not None:
            return NA
        if x is None:
            return NA
        return F.conv2d(x, p["conv_in.weight"], p["conv_in.bias"], padding=1), None
    if name == "conv_out":
        h = F.silu(U._gn(ins[0], p, "conv_norm_out", cfg.norm_num_groups, cfg.norm_eps))
        return F.conv2d(h, p["conv_out.weight"], p["conv_out.bias"], padding=1), None
    if kind == "film":
        if cond.emb is None:
            return NA
        w = cond.film(name[len("film."):], ins[0], rows, wrong)
        return (w, None) if w is not None else NA
    if kind == "downsampler":
        return F.conv2d(ins[0], p[f"{name}.conv.weight"], p[f"{name}.conv.bias"], stride=2, padding=1), None
    if kind == "upsampler":
        h = F.interpolate(ins[0], scale_factor=2.0, mode="nearest")
        return F.conv2d(h, p[f"{name}.conv.weight"], p[f"{name}.conv.bias"], padding=1), None
    if kind == "attention":
        w = cond.transformer(name, ins[0], rows, wrong)
        return (w, ins[0]) if w is not None else NA
    # resnets
    ins = list(ins)
    if wrong in ("cat_swapped", "skip_post_film") and len(ins) < 2:
        return NA
    if wrong == "skip_post_film":
        # Q6: the hook modulates what goes down, never the skips -- the fault reads the modulated tensor where the skip is the
        # block output the hook modulated
        skip_name = inputs[name][1]
        post = [n for n in taps if n.startswith("film.down_") and inputs[n][0] == skip_name]
        if not post:
            return NA
        ins[1] = taps[post[0]][rows]
    freeu = len(ins) == 2 and cond.freeu is not None and name.startswith(("up_blocks.0.", "up_blocks.1."))
    if wrong == "freeu_dropped" and not freeu:
        return NA
    if freeu and wrong != "freeu_dropped":      # (the taps hold the plain pair; the resnet reads the re-weighted one)
        from tests.freeu_ref import apply_freeu
        ins = list(apply_freeu(int(name.split(".")[1]), ins[0], ins[1], **cond.freeu))
    if wrong == "cat_swapped":
        ins = ins[::-1]
    x = torch.cat(ins, 1) if len(ins) > 1 else ins[0]
    w = cond.resnet(name, x, rows, wrong if wrong in ("temb_other_row", "temb_neighbour_slice") else None)
    if w is None:
        return NA
    return w, (x if len(ins) == 1 and x.shape[1] == w.shape[1] else None)


def branch_error(got, want, x, tol, slack=SLACK):
    """(error, bound, branch norm): || got - want || and tol || want - x || + slack || bf16(want) - want ||, in absolute terms"""
    got, want = got.double(), want.double()
    bnorm = (want - x.double()).norm().item() if x is not None else want.norm().item()
    rnd = (want.to(torch.bfloat16).double() - want).norm().item()
    return (got - want).norm().item(), tol * bnorm + slack * rnd, bnorm


def check_taps(cond, taps, inputs, sample, out, rows=None, tol=None, what="", sliced=False, only=None, extra=None, need=None):
    """Every tap of one forward against ``block_want`` on the taps that feed it.  ``taps`` {name: (B, C, H, W) fp32} in execution
    order; ``inputs`` {name: input names} (the oracle's trace gives them; ``sample`` names the sample); ``out``: the forward's
    output, the tap ``conv_out``.  ``rows``: the rows to compare (default: all); ``sliced``: the tensors hold these rows only; ``only``: the blocks to check
    (default: all); ``extra``: {name: tensor} that blocks may read and that are not themselves checked (the stored deep feature of a
    DeepCache shallow forward, whose ``taps`` / ``inputs`` hold the blocks it runs); ``need``: a dict that receives {kind: (the
    tolerance the worst block of the kind needs, (error - slack * rounding term) / ||branch||, its name, its error / ||branch||)},
    the transformer blocks that token merging / token downsampling changes under a kind of their own.  Returns {kind: (worst error / bound, name, error / branch)}; raises on the first block beyond
    its bound, by name."""
    tol = TOL if tol is None else tol
    rows_ = list(range(cond.B)) if rows is None else list(rows)
    tensors = dict(extra or {})
    tensors.update(taps)
    tensors["sample"], tensors["conv_out"] = sample, out
    worst = {}
    pick = (lambda x: x) if sliced else (lambda x: x[rows_])
    assert list(taps) == [n for n in inputs if n != "conv_out"], f"{what}: taps {list(taps)} are not the blocks {list(inputs)}"
    for name in list(taps) + ["conv_out"]:
        if only is not None and name not in only:
            continue
        got = pick(tensors[name])
        if name == "conv_norm_out.in":
            assert torch.equal(got, pick(tensors[inputs[name][0]])), f"{what}: {name} is not the tensor of {inputs[name][0]}"
            continue
        ins = [pick(tensors[n]) for n in inputs[name]]
        want, x = block_want(cond, name, ins, rows_)
        kind = kind_of(name, ins, want)
        assert torch.isfinite(got).all(), f"{what}: {name}: non-finite output"
        err, bound, bnorm = branch_error(got, want, x, tol[kind])
        assert bnorm > 0, f"{what}: {name}: the reference branch is zero"
        if need is not None:
            changed = kind == "attention" and (feature_of(name) in cond.merging or feature_of(name) in cond.pooling)
            key = kind + (" (merged)" if cond.merging else " (pooled)") if changed else kind
            needs = (err - (bound - tol[kind] * bnorm)) / bnorm
            if key not in need or needs > need[key][0]:
                need[key] = (needs, name, err / bnorm)
        assert err <= bound, (f"{what}: first failing block {name} ({kind}): branch error {err / bnorm:.4g} of ||branch|| > bound "
                              f"{bound / bnorm:.4g} (tol {tol[kind]:g})")
        if kind not in worst or err / bound > worst[kind][0]:
            worst[kind] = (err / bound, name, err / bnorm)
    return worst


def eligible_and_readers(cond, inputs):
    """the transformer blocks that ``cond``'s option changes and the blocks that read their outputs directly"""
    own = {n for n in inputs if ".attentions." in n and (feature_of(n) in cond.merging or feature_of(n) in cond.pooling)}
    return own | {n for n, ins in inputs.items() if own & set(ins)}


def shallow_blocks(cfg, inputs, branch):
    """(names, deep): the blocks of ``inputs`` that a DeepCache shallow forward of ``branch`` runs, in order -- conv_in, layers
    0..branch of down_blocks.0, the last branch + 2 layers of the last up block, what follows them -- and the name of the tensor the
    refresh forward stores: the hidden input of ``deepcache_ref.deep_key``"""
    from tests.deepcache_ref import deep_key
    n, j0 = cfg.num_levels, cfg.layers_per_block - 1 - branch
    keep = {"conv_in", f"film.up_{n - 1}", "conv_norm_out.in", "conv_out"}
    keep |= {f"down_blocks.0.{k}.{j}" for j in range(branch + 1) for k in ("resnets", "attentions")}
    keep |= {f"up_blocks.{n - 1}.{k}.{j}" for j in range(j0, cfg.layers_per_block + 1) for k in ("resnets", "attentions")}
    return [x for x in inputs if x in keep], inputs[deep_key(cfg, branch)][0]


def report(what, worst, need=None):
    print(f"{what}: worst branch error per block kind, as a fraction of its bound")
    for kind, (frac, name, rel) in sorted(worst.items()):
        print(f"  {kind:<12} {frac:6.3f} of the bound ({rel:.3e} of ||branch||) at {name}")
    for kind, (tol, name, rel) in sorted((need or {}).items()):
        print(f"  {kind:<18} needs tol {tol:9.2e} (error {rel:.3e} of ||branch||) at {name}")


# ---------------------------------------------------------------------------------------------- the cases of the two test files
def make_case(name, cfg, params, batch, hw, text_len, *, cam=True, img=True, ref_batch=None, layout=None, freeu=None, seed=0,
              cam_dim=96, tome=None, todo=None):
    """Inputs of one forward, built as parity_util.make_inputs builds them, with one timestep per row.  ``layout``: None, or
    ("views", V, g) / ("objects", O, V, g) / ("ragged", counts, g) -- ``batch`` is then ignored.  ``ref_batch`` (ordinary
    forward): rows of the reference, default ``batch``; half of it is the guidance form."""
    from tests import objects_util, ragged_util
    from tests.parity_util import make_inputs
    groups, kw, O = None, {}, 0
    if layout is not None:
        assert img
        if layout[0] == "views":
            _, V, g = layout
            O, R = 1, V
            groups = [Group([j * V + v for j in range(g)], range(g), [0]) for v in range(V)]
            kw = dict(views=V)
        elif layout[0] == "objects":
            _, O, V, g = layout
            R = O * V
            groups = [Group([objects_util.row(O, V, j, o, v) for j in range(g)], [j * O + o for j in range(g)], [o])
                      for o in range(O) for v in range(V)]
            kw = dict(views=V, objects=O)
        else:
            _, counts, g = layout
            O, (_, R), obj = len(counts), ragged_util.offsets(counts), ragged_util.object_of(counts)
            groups = [Group(ragged_util.view_rows(R, g, c), [j * O + obj[c] for j in range(g)], [obj[c]]) for c in range(R)]
            kw = dict(views=tuple(counts))
        batch = g * R
    inp = make_inputs(cfg, max(batch, 2), hw, text_len, seed=seed, cam_dim=cam_dim)
    # one timestep per row, neighbours far apart (another row's time projection is then a different vector, not a near copy)
    t = torch.tensor([(981, 21, 501, 261, 741, 141, 621, 381)[b % 8] for b in range(batch)], dtype=torch.float32)
    c = SimpleNamespace(name=name, cfg=cfg, params=params, B=batch, sample=inp["sample"][:batch], t=t, freeu=freeu, kw=kw, groups=groups,
                        cams=(inp["src"][:batch], inp["tgt"][:batch], inp["proj"]) if cam else None, lat=None, text=inp["text"][:batch], tome=tome, todo=todo)
    if layout is not None:
        c.text, c.lat = inp["text"][:g * O], inp["lat"][:O]
    elif img:
        c.lat = inp["lat"][:ref_batch or batch]
    return c


def case_cond(c, feats, round_text=True, tome_tables=None, t=None):
    """the conditioning of case ``c`` around the encoder maps ``feats`` (the engine's kept ones; the oracle's own on the CPU);
    ``tome_tables``: the slot tables of the forward (token merging); ``t``: other timesteps than the case's"""
    return Cond(c.cfg, c.params, c.B, c.t if t is None else t, c.text, c.cams, feats, c.groups, c.freeu, round_text=round_text,
                tome=getattr(c, "tome", None), todo=getattr(c, "todo", None), tome_tables=tome_tables, latent_hw=tuple(c.sample.shape[-2:]))


def oracle_forward(c, _in_freeu=False, tables_out=None, fault=None):
    """(out, taps, inputs, feats) of case ``c`` by the ORACLE's forward: one call, or -- a layout forward -- the independent
    calls of its definition, rows scattered.  ``taps`` {name: tensor} without ``conv_out``; ``inputs`` {name: input names}.
    A case with ``tome`` / ``todo`` runs under the option oracle; ``tables_out``: a dict that receives the slot tables token
    merging used, {feature: (B, H*W)}.  ``fault`` = (block name, variant of ``OPTION_VARIANTS``, Cond): that one block computes
    the variant, the rest of the forward is right (what a single-block fault does to the OUTPUT)."""
    if c.freeu is not None and not _in_freeu:
        from tests.freeu_ref import freeu_oracle
        with freeu_oracle(**c.freeu):
            return oracle_forward(c, True, tables_out, fault)
    option, rec = contextlib.nullcontext(), {}
    if getattr(c, "tome", None) is not None:
        from tests.tome_ref import tome_oracle
        option = tome_oracle(**c.tome, record=rec)
    elif getattr(c, "todo", None) is not None:
        from tests.todo_ref import todo_oracle
        option = todo_oracle(**c.todo)
    with option, _one_block_fault(fault):
        return _oracle_forward(c, rec, tables_out)


@contextlib.contextmanager
def _one_block_fault(fault):
    """``oracle.sd21_unet.transformer_2d`` answers block ``fault[0]`` with ``Cond.transformer(wrong=fault[1])`` on the rows of the
    call (found by the call's input: the case's rows in order, or -- a layout forward -- the rows of the group being computed)"""
    if fault is None:
        yield
        return
    block, variant, cond = fault
    inner = U.transformer_2d
    calls = {"n": 0}

    def transformer(p, key, x, text, heads, groups, attn_hook, hook_name):
        if key != block or attn_hook is None and cond.feats is not None:          # (the encoder pass has no adapter hook)
            return inner(p, key, x, text, heads, groups, attn_hook, hook_name)
        rows = cond.groups[calls["n"]].rows if len(cond.groups) > 1 else list(range(cond.B))
        calls["n"] += 1
        U.transformer_2d = inner
        try:
            return cond.transformer(block, x, rows, variant)
        finally:
            U.transformer_2d = transformer
    U.transformer_2d = transformer
    try:
        yield
    finally:
        U.transformer_2d = inner


def _oracle_forward(c, rec, tables_out):
    kw = dict(img_ref_scale=0.3, cam_modulation_strength=0.2)
    if c.cams is not None:
        kw["fourier_proj"] = c.cams[2]

    def call(rows, text, ref):
        trace, feats = {}, {}
        src = tgt = None
        if c.cams is not None:
            cr = [r % c.cams[0].shape[0] for r in rows]
            src, tgt = c.cams[0][cr], c.cams[1][cr]
        out = OM.multiview_unet_forward(c.params, c.cfg, c.sample[rows], c.t[rows], text, src, tgt, ref, features_out=feats, trace=trace, **kw)
        return out, trace, feats

    if c.groups is None:
        out, trace, feats = call(list(range(c.B)), c.text, c.lat)
        if tables_out is not None:
            tables_out.update(rec)
        inputs = {n: i for n, (_, i) in trace.items()}
        taps = {n: x for n, (x, _) in trace.items() if n != "conv_out"}
        return out, taps, inputs, (feats or None)
    out, taps, inputs, feats = None, {}, {}, {}
    for grp in c.groups:
        o, trace, f = call(grp.rows, c.text[grp.text_rows], c.lat[grp.ref_rows])
        if out is None:
            out = torch.empty(c.B, *o.shape[1:])
            nref = c.lat.shape[0]
        out[grp.rows] = o
        for n, (x, i) in trace.items():
            if n == "conv_out":
                inputs[n] = i
                continue
            taps.setdefault(n, torch.empty(c.B, *x.shape[1:]))[grp.rows] = x
            inputs[n] = i
        for n, x in f.items():
            feats.setdefault(n, torch.empty(nref, *x.shape[1:]))[grp.ref_rows] = x
        if tables_out is not None:
            for n, s in rec.items():
                tables_out.setdefault(n, torch.zeros(c.B, s.shape[1], dtype=torch.long))[grp.rows] = s
    return out, taps, inputs, feats


ADAPTER_OUT_GAIN = dict(weight=3.0, bias=5.0)


def tiny_params():
    """The seeded weights of the tiny cases: the suite's usual ones (parity_util.build_pair) with every adapter out-projection
    ``to_out_ref`` scaled up.  With the plain seeded weights the adapter is a small part of a transformer's branch, and three of
    the wiring faults sit nearer than three bounds (measured on the CPU, worst block of all cases: ``to_out_ref`` bias left out
    1.4 x the bound, the two processors exchanged 1.5 x, another row's reference 2.0 x on the 8 x 24 maps); the gain makes the
    engine's adapter wiring as visible as the rest, and a wrong engine is held to the same tolerance."""
    cfg = U.UNetConfig.tiny()
    params = OM.init_mvd_params(cfg, 0, cam_dim=96, cam_hidden=48)
    for k in params:
        if ".processor.to_out_ref.0." in k:
            params[k] = params[k] * ADAPTER_OUT_GAIN[k.rsplit(".", 1)[1]]
    return cfg, params


def tiny_cases(cfg, params):
    """the tiny cases of tests/test_block_parity_gpu.py (cases 1-7 of its table), by name"""
    mk = lambda name, *a, **k: (name, make_case(name, cfg, params, *a, **k))      # noqa: E731
    from tests.freeu_ref import SD21
    return dict([
        mk("uniform_b1_cam_img", 1, 16, 7), mk("uniform_b3_cam_img", 3, 16, 7),
        mk("uniform_b3_cam", 3, 16, 7, img=False), mk("uniform_b3_img", 3, 16, 7, cam=False), mk("uniform_b3_plain", 3, 16, 7, cam=False, img=False),
        mk("wide_b3_cam_img", 3, (8, 24), 77),
        mk("guidance_4_on_2", 4, 16, 7, cam=False, ref_batch=2),
        mk("views_v2_g2", 0, 16, 7, cam=False, layout=("views", 2, 2)),
        mk("objects_o2_v2_g2", 0, 16, 7, cam=False, layout=("objects", 2, 2, 2)),
        mk("ragged_2_1_g2", 0, 16, 7, cam=False, layout=("ragged", (2, 1), 2)),
        mk("freeu_b2_img", 2, 16, 7, cam=False, freeu=dict(SD21)),
    ])


AREA22 = dict(factor=2, factor_level_2=2, method="area")


def option_cases(cfg, params):
    """the tiny token-merging / token-downsampling cases of tests/test_block_parity_options_gpu.py, by name: the smallest shapes
    at which level 0 merges and level 1 still has a 2 x 2 map"""
    from tests.freeu_ref import SD21
    from tests.todo_ref import PARITY_SETTING as TODO
    from tests.tome_ref import PARITY_SETTING as TOME
    mk = lambda name, *a, **k: (name, make_case(name, cfg, params, *a, **k))      # noqa: E731
    return dict([
        mk("tome_b2", 2, 16, 7, tome=dict(TOME)), mk("tome_b2_md2", 2, 16, 7, tome=dict(ratio=0.5, max_downsample=2)),
        mk("tome_wide_b2", 2, (8, 24), 7, tome=dict(TOME)),
        mk("todo_b2", 2, 16, 7, todo=dict(TODO)), mk("todo_b2_area22", 2, 16, 7, todo=dict(AREA22)),
        mk("todo_wide_b2", 2, (8, 24), 7, todo=dict(TODO)),
        mk("tome_views_v2_g2", 0, 16, 7, cam=False, layout=("views", 2, 2), tome=dict(TOME)),
        mk("todo_objects_o2_v2_g2", 0, 16, 7, cam=False, layout=("objects", 2, 2, 2), todo=dict(TODO)),
        mk("todo_freeu_b2", 2, 16, 7, cam=False, freeu=dict(SD21), todo=dict(AREA22)),
    ])


_INPUTS = {}


def input_names(cfg, cam):
    """{block: names of its inputs} of a forward of ``cfg``'s topology with camera conditioning ``cam``: the oracle's trace of a
    small forward of the tiny configuration (the names depend on the topology alone, which the two configurations share)"""
    tiny = U.UNetConfig.tiny()
    assert (cfg.num_levels, cfg.layers_per_block) == (tiny.num_levels, tiny.layers_per_block)
    if cam not in _INPUTS:
        params = OM.init_mvd_params(tiny, 0, cam_dim=96, cam_hidden=48)
        _INPUTS[cam] = oracle_forward(make_case("names", tiny, params, 1, 8, 2, cam=cam, img=False))[2]
    return _INPUTS[cam]
