"""The options of the main UNet pass (DESIGN.md section 9 "main-pass options"; ``MainOpts`` in csrc/engine.hip is the C++ side): FreeU,
token merging, token downsampling, the taps and DeepCache as one value, their checks, and the engine calls that lead from one value
to another."""
import math
from typing import NamedTuple, Optional

TODO_METHODS = ("nearest", "area")          # method of mvd_engine_set_todo / mvd_op_todo_downsample, by index


class _Fields(NamedTuple):
    freeu: Optional[tuple] = None       # (s1, s2, b1, b2)
    tome: Optional[tuple] = None        # (ratio, max_downsample); a ratio of 0 merges nothing: None
    tome_keep: bool = False             # the blocks' slot tables are kept (test plumbing); nothing without ``tome``
    todo: Optional[tuple] = None        # (factor, factor_level_2, method); factors (1, 1) touch nothing: None
    taps: bool = False                  # the main pass's block outputs are kept (test plumbing)
    deepcache: Optional[int] = None     # the branch


class MainOptions(_Fields):
    """What the engine's main pass is set to; ``MainOptions()`` is everything off.  Normalised on construction, so that two values
    are equal exactly when the engine runs the same forward under them."""
    __slots__ = ()

    def __new__(cls, freeu=None, tome=None, tome_keep=False, todo=None, taps=False, deepcache=None):
        freeu = None if freeu is None else tuple(float(v) for v in freeu)
        tome = None if tome is None or not float(tome[0]) > 0.0 else (float(tome[0]), int(tome[1]))
        todo = None if todo is None or (todo[0] <= 1 and todo[1] <= 1) else (int(todo[0]), int(todo[1]), todo[2])
        return super().__new__(cls, freeu, tome, bool(tome_keep) and tome is not None, todo, bool(taps),
                               None if deepcache is None else int(deepcache))

    def _replace(self, **fields):
        return MainOptions(**{**self._asdict(), **fields})


def transitions(have: MainOptions, want: MainOptions):
    """The ``(method name, args, kwargs)`` calls on an ``MVDEngine`` that take it from ``have`` to ``want``: none for an option that
    does not differ, one for an option that does.  Token merging and token downsampling are alternatives and the engine refuses
    one while the other is set: whichever is being switched off goes first."""
    calls = []
    if want.freeu != have.freeu:
        calls.append(("clear_freeu", (), {}) if want.freeu is None else ("set_freeu", want.freeu, {}))
    if want.todo is None and have.todo is not None:
        calls.append(("clear_todo", (), {}))
    if (want.tome, want.tome_keep) != (have.tome, have.tome_keep):
        calls.append(("clear_tome", (), {}) if want.tome is None else ("set_tome", want.tome, {"keep_tables": want.tome_keep}))
    if want.todo is not None and want.todo != have.todo:
        calls.append(("set_todo", want.todo, {}))
    if want.taps != have.taps:
        calls.append(("set_taps", (want.taps,), {}))
    if want.deepcache != have.deepcache:
        calls.append(("clear_deepcache", (), {}) if want.deepcache is None else ("set_deepcache", (want.deepcache,), {}))
    return calls


def check_freeu(s1, s2, b1, b2):
    """(s1, s2, b1, b2) as floats; ValueError unless all four are positive and finite."""
    vals = tuple(float(v) for v in (s1, s2, b1, b2))
    if not all(math.isfinite(v) and v > 0.0 for v in vals):
        raise ValueError(f"FreeU: s1, s2, b1, b2 must be positive and finite, got {vals}")
    return vals


def check_tome(ratio, max_downsample=1):
    """(ratio, max_downsample); ValueError unless 0 <= ratio <= 0.75 and max_downsample is one of 1, 2, 4, 8 (tomesd's)."""
    ratio = float(ratio)
    if not 0.0 <= ratio <= 0.75:
        raise ValueError(f"token merging: ratio must lie in [0, 0.75] (a quarter of the tokens are dst and stay), got {ratio}")
    if isinstance(max_downsample, bool) or max_downsample not in (1, 2, 4, 8):
        raise ValueError(f"token merging: max_downsample must be one of 1, 2, 4, 8, got {max_downsample!r}")
    return ratio, int(max_downsample)


def check_todo(factor=2, factor_level_2=1, method="nearest"):
    """(factor, factor_level_2, method); ValueError unless both factors are integers in [1, 4] and the method is "nearest" or "area"."""
    for name, f in (("factor", factor), ("factor_level_2", factor_level_2)):
        if isinstance(f, bool) or not isinstance(f, int) or not 1 <= f <= 4:
            raise ValueError(f"token downsampling: {name} must be an integer in [1, 4] (1: untouched), got {f!r}")
    if method not in TODO_METHODS:
        raise ValueError(f"token downsampling: method must be one of {TODO_METHODS}, got {method!r}")
    return int(factor), int(factor_level_2), method


def check_alternatives(tome, todo, who: str):
    """ValueError from ``who`` ("enable_tome" / "enable_todo", with the setting it is about to make) when ``tome`` and ``todo`` would
    both be on: token merging and token downsampling are alternatives."""
    if MainOptions(tome=tome).tome is not None and MainOptions(todo=todo).todo is not None:
        raise ValueError("enable_tome: token downsampling is enabled and the two are alternatives -- disable_todo() first" if who == "enable_tome"
                         else "enable_todo: token merging is enabled and the two are alternatives -- disable_tome() first")


def check_deepcache(cache_interval, cache_branch_id, layers_per_block: int):
    """``(cache_interval, cache_branch_id)`` as two ints, or ValueError: the interval >= 1, the branch in [0, layers_per_block)."""
    try:
        ok = float(cache_interval) == int(cache_interval) and float(cache_branch_id) == int(cache_branch_id)
    except (TypeError, ValueError):
        ok = False
    if not ok or isinstance(cache_interval, bool) or isinstance(cache_branch_id, bool):
        raise ValueError(f"DeepCache: cache_interval and cache_branch_id must be integers, got {cache_interval!r}, {cache_branch_id!r}")
    interval, branch = int(cache_interval), int(cache_branch_id)
    if interval < 1:
        raise ValueError(f"DeepCache: cache_interval must be >= 1, got {interval}")
    if not 0 <= branch < layers_per_block:
        raise ValueError(f"DeepCache: cache_branch_id must lie in [0, {layers_per_block}) (layers_per_block), got {branch}")
    return interval, branch


def _block_maps(cfg, height, width):
    """``(feature name, H, W, down)`` of every transformer block with a map at a latent of ``height`` x ``width``:
    ``down = ceil(sqrt(N0 // N))``, tomesd's measure of how much coarser than the latent the block is."""
    for _, name, _, _ in cfg.transformers():
        part = name.split("_")          # down_block_{i}_attn_{j} | mid_block_attn_0 | up_block_{i}_attn_{j}
        level = int(part[2]) if part[0] == "down" else cfg.num_levels - 1 - (int(part[2]) if part[0] == "up" else 0)
        H, W = height >> level, width >> level
        if H >= 1 and W >= 1:
            q = (height * width) // (H * W)
            yield name, H, W, (math.isqrt(q - 1) + 1 if q > 0 else 0)


def tome_blocks(cfg, height, width, ratio, max_downsample=1):
    """``{feature name: (H, W, r)}`` of the transformer blocks that merge at a latent of ``height`` x ``width``: tomesd's rule
    ``down <= max_downsample`` with ``r = min(#src, int(N * ratio)) > 0``."""
    out = {}
    for name, H, W, down in _block_maps(cfg, height, width):
        r = min(H * W - (H // 2) * (W // 2), int(H * W * float(ratio)))
        if H >= 2 and W >= 2 and down <= max_downsample and r > 0:
            out[name] = (H, W, r)
    return out


def todo_blocks(cfg, height, width, factor=2, factor_level_2=1):
    """``{feature name: (H, W, f, Nk)}`` of the transformer blocks whose self-attention reads downsampled keys at a latent of
    ``height`` x ``width``: ``down`` 1 takes ``factor``, 2 ``factor_level_2``, deeper blocks none; a block with ``f == 1``,
    ``H // f < 1`` or ``W // f < 1`` is untouched.  ``Nk = (H // f) * (W // f)``."""
    out = {}
    for name, H, W, down in _block_maps(cfg, height, width):
        f = factor if down == 1 else factor_level_2 if down == 2 else 1
        if f > 1 and H // f >= 1 and W // f >= 1:
            out[name] = (H, W, f, (H // f) * (W // f))
    return out
