"""The block-by-block parity check (tests/block_ref.py, tests/test_block_parity_gpu.py) can see what it is for -- shown on the
CPU, on the ORACLE's own trace of the tiny cases the GPU file runs:

(a) the blocks of ``block_ref.block_want``, chained from the sample, reproduce the oracle's forward (so the reference of every
    block, the names of its inputs and the restated adapter branch are the oracle's);
(b) for every block of every case, each wiring fault of ``block_ref.VARIANTS`` that applies to it lies at least 3 x the block
    kind's bound away from the right output -- a condition, not a measurement: an engine with that fault lands at least twice the
    bound outside it.  The nearest fault per case is printed;
(c) each such fault, written over the block's tensor in a bf16-rounded copy of the trace (a stand-in for the engine's taps),
    fails the bound; the unmutated copy passes, and ``check_taps`` names the mutated block."""
import functools

import pytest
import torch

import oracle
from tests import block_ref as R

CASES = ("uniform_b1_cam_img", "uniform_b3_cam_img", "uniform_b3_cam", "uniform_b3_img", "uniform_b3_plain", "wide_b3_cam_img",
         "guidance_4_on_2", "views_v2_g2", "objects_o2_v2_g2", "ragged_2_1_g2", "freeu_b2_img")
MARGIN = 3.0


@functools.lru_cache(maxsize=1)
def _cases():
    torch.set_num_threads(oracle.host_threads())
    return R.tiny_cases(*R.tiny_params())


@functools.lru_cache(maxsize=None)
def _traced(name):
    """(case, out, taps, inputs, feats, tensors) of the oracle's forward; computed once, never modified"""
    c = _cases()[name]
    out, taps, inputs, feats = R.oracle_forward(c)
    tensors = dict(taps)
    tensors["sample"], tensors["conv_out"] = c.sample, out
    return c, out, taps, inputs, feats, tensors


def test_case_list_is_the_gpu_file_s():
    assert tuple(_cases()) == CASES


def test_trace_leaves_the_oracle_s_forward_as_it_is():
    from oracle import mvd as OM
    c = _cases()["uniform_b3_cam_img"]
    kw = dict(fourier_proj=c.cams[2], img_ref_scale=0.3, cam_modulation_strength=0.2)
    plain = OM.multiview_unet_forward(c.params, c.cfg, c.sample, c.t, c.text, c.cams[0], c.cams[1], c.lat, **kw)
    _, out, taps, inputs, _, _ = _traced("uniform_b3_cam_img")
    assert torch.equal(plain, out)
    # execution order, every block once, inputs that exist, two inputs exactly at the up-block resnets
    names = list(taps)
    assert names[0] == "conv_in" and names[-1] == "conv_norm_out.in" and len(set(names)) == len(names)
    n_res = sum(".resnets." in n for n in names)
    n_att = sum(".attentions." in n for n in names)
    assert (n_res, n_att, sum(n.startswith("film.") for n in names)) == (22, 16, 8), names
    for i, n in enumerate(names):
        assert all(s == "sample" or s in names[:i] for s in inputs[n]), (n, inputs[n])
        assert (len(inputs[n]) == 2) == (n.startswith("up_blocks.") and ".resnets." in n), (n, inputs[n])
    assert inputs["film.up_0"] == ("up_blocks.0.upsamplers.0",) and inputs["up_blocks.0.resnets.0"] == ("mid_block.resnets.1", "down_blocks.3.resnets.1")
    assert inputs["up_blocks.3.resnets.2"][1] == "conv_in" and inputs["up_blocks.1.resnets.0"][0] == "film.up_0"
    # Q6: the skips are the unmodulated block outputs
    assert inputs["up_blocks.0.resnets.2"][1] == "down_blocks.2.downsamplers.0" and inputs["mid_block.resnets.0"] == ("film.down_3",)


@pytest.mark.parametrize("name", CASES)
def test_chained_blocks_reproduce_the_oracle_forward(name):
    c, out, taps, inputs, feats, _ = _traced(name)
    cond = R.case_cond(c, feats, round_text=False)
    mine = {"sample": c.sample}
    for n in list(taps) + ["conv_out"]:
        if n == "conv_norm_out.in":
            mine[n] = mine[inputs[n][0]]
            continue
        mine[n], _ = R.block_want(cond, n, [mine[s] for s in inputs[n]])
    for n, x in taps.items():
        torch.testing.assert_close(mine[n], x, rtol=1e-4, atol=1e-4 * x.abs().max().item(), msg=lambda m: f"{name}: {n}: {m}")
    torch.testing.assert_close(mine["conv_out"], out, rtol=1e-4, atol=1e-4 * out.abs().max().item())


@functools.lru_cache(maxsize=None)
def _faults(name):
    """{(block, variant): (distance, bound, branch norm, kind)} of every fault that applies, against the bf16-text reference"""
    c, out, taps, inputs, feats, tensors = _traced(name)
    cond = R.case_cond(c, feats)
    res = {}
    for n in list(taps) + ["conv_out"]:
        if n == "conv_norm_out.in":
            continue
        ins = [tensors[s] for s in inputs[n]]
        want, x = R.block_want(cond, n, ins)
        kind = R.kind_of(n, ins, want)
        for v in R.VARIANTS:
            w, _ = R.block_want(cond, n, ins, wrong=v, taps=tensors, inputs=inputs)
            if w is None:
                continue
            assert w.shape == want.shape, (n, v)
            err, bound, bnorm = R.branch_error(w, want, x, R.TOL[kind])
            gerr, _, _ = R.branch_error(R.bf16(w), want, x, R.TOL[kind])       # (c): as an engine would hold it
            res[(n, v)] = (err, bound, bnorm, kind, gerr)
    return res


# which faults must have somewhere to apply, by case (a fault that never applies would prove nothing)
def _expected(c):
    ex = {"temb_neighbour_slice", "cat_swapped"}
    if c.B > 1:
        ex |= {"temb_other_row", "text_other_row"}
    if c.lat is not None:
        ex |= {v for v in R.VARIANTS if v.startswith("adapter") and "other_ref" not in v}
        if c.lat.shape[0] > 1:
            ex |= {"adapter_self_other_ref", "adapter_cross_other_ref"}
    if c.freeu is not None:
        ex |= {"freeu_dropped"}
    if c.cams is not None:
        ex |= {"skip_post_film", "film_neighbour"} | ({"film_other_row"} if c.B > 1 else set())
    return ex


@pytest.mark.parametrize("name", CASES)
def test_every_wiring_fault_is_three_bounds_away(name):
    c = _cases()[name]
    faults = _faults(name)
    seen = {v for _, v in faults}
    assert _expected(c) <= seen, (name, sorted(_expected(c) - seen))
    nearest = {}
    for (n, v), (err, bound, bnorm, kind, _) in faults.items():
        if v not in nearest or err / bound < nearest[v][0]:
            nearest[v] = (err / bound, err / bnorm, kind, n)
    print(f"\n{name}: nearest block per wiring fault (distance / bound of its kind; distance / ||branch||)")
    for v, (frac, rel, kind, n) in sorted(nearest.items(), key=lambda kv: kv[1][0]):
        print(f"  {v:<26} {frac:7.2f} x bound  {rel:.3f} of the branch  {kind:<10} {n}")
    short = {k: f"{e / b:.2f}" for k, (e, b, _, _, _) in faults.items() if e < MARGIN * b}
    assert not short, f"{name}: faults nearer than {MARGIN} x the bound: {short}"


@pytest.mark.parametrize("name", CASES)
def test_every_wiring_fault_fails_the_bound(name):
    c, out, taps, inputs, feats, _ = _traced(name)
    for (n, v), (_, bound, _, _, gerr) in _faults(name).items():
        assert gerr > bound, (name, n, v, gerr / bound)


@pytest.mark.parametrize("name,block,variant", [("uniform_b3_cam_img", "up_blocks.2.attentions.0", "adapter_cross_other_ref"),
                                                ("uniform_b3_cam_img", "film.up_1", "film_other_row"),
                                                ("ragged_2_1_g2", "down_blocks.1.resnets.0", "temb_neighbour_slice"),
                                                ("guidance_4_on_2", "mid_block.attentions.0", "adapter_self_out_bias0")])
def test_check_taps_passes_the_rounded_trace_and_names_a_mutated_block(name, block, variant):
    c, out, taps, inputs, feats, tensors = _traced(name)
    cond = R.case_cond(c, feats)
    engine = {n: R.bf16(x) for n, x in taps.items()}             # a stand-in for the engine's taps: the oracle's, in bf16
    worst = R.check_taps(cond, engine, inputs, c.sample, out, what=name)
    assert set(worst) >= {"conv_in", "resnet", "resnet_sc", "attention", "downsampler", "upsampler", "tail"}
    assert all(frac <= 1.0 for frac, _, _ in worst.values())
    # rows may be checked alone: the same bound per block
    R.check_taps(cond, engine, inputs, c.sample, out, rows=[0, c.B - 1], what=name)
    ins = [(c.sample if s == "sample" else engine[s]) for s in inputs[block]]
    w, _ = R.block_want(cond, block, ins, wrong=variant, taps={**engine, "sample": c.sample}, inputs=inputs)
    mutated = dict(engine)
    mutated[block] = R.bf16(w)
    with pytest.raises(AssertionError, match=f"first failing block {block.replace('.', '[.]')} "):
        R.check_taps(cond, mutated, inputs, c.sample, out, what=name)
