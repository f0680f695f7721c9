"""The main-pass options value (``mvd_amd/main_options.py``): its normalisations, and ``transitions(have, want)`` between EVERY pair of
the enumerated states, run against a simulated engine that refuses token merging while token downsampling is set and the reverse,
as ``mvd_engine_set_tome`` / ``mvd_engine_set_todo`` do.  No GPU and no library."""
import itertools

from mvd_amd.main_options import MainOptions, transitions

FREEU = (None, (0.9, 0.2, 1.4, 1.6))
TOME = ((None, False), ((0.5, 1), False), ((0.5, 1), True), ((0.3, 2), False))        # (tome, tome_keep)
TODO = (None, (2, 1, "nearest"), (2, 2, "area"))
TAPS = (False, True)
DEEPCACHE = (None, 0, 1)
STATES = [MainOptions(freeu, tome, keep, todo, taps, deepcache)
          for freeu, (tome, keep), todo, taps, deepcache in itertools.product(FREEU, TOME, TODO, TAPS, DEEPCACHE)
          if tome is None or todo is None]

# the option a call changes (token merging's two fields are one option: set_tome carries both), and the fields that make it up
OPTION = {"set_freeu": "freeu", "clear_freeu": "freeu", "set_tome": "tome", "clear_tome": "tome", "set_todo": "todo", "clear_todo": "todo",
          "set_taps": "taps", "set_deepcache": "deepcache", "clear_deepcache": "deepcache"}
FIELDS = {"freeu": ("freeu",), "tome": ("tome", "tome_keep"), "todo": ("todo",), "taps": ("taps",), "deepcache": ("deepcache",)}


class Refused(Exception):
    pass


class SimEngine:
    """``MVDEngine``'s nine methods on a plain record of what the C engine holds, with engine.hip's cross-check"""

    def __init__(self, have: MainOptions):
        self.state = have._asdict()

    def set_freeu(self, s1, s2, b1, b2):
        self.state["freeu"] = (s1, s2, b1, b2)

    def clear_freeu(self):
        self.state["freeu"] = None

    def set_tome(self, ratio=0.5, max_downsample=1, keep_tables=False):
        todo = self.state["todo"]
        if ratio > 0 and todo is not None and (todo[0] > 1 or todo[1] > 1):
            raise Refused("set_tome: token downsampling is set")
        self.state["tome"], self.state["tome_keep"] = (ratio, max_downsample), keep_tables

    def clear_tome(self):
        self.state["tome"], self.state["tome_keep"] = None, False

    def set_todo(self, factor=2, factor_level_2=1, method="nearest"):
        tome = self.state["tome"]
        if (factor > 1 or factor_level_2 > 1) and tome is not None and tome[0] > 0:
            raise Refused("set_todo: token merging is set")
        self.state["todo"] = (factor, factor_level_2, method)

    def clear_todo(self):
        self.state["todo"] = None

    def set_taps(self, enable=True):
        self.state["taps"] = enable

    def set_deepcache(self, branch=0):
        self.state["deepcache"] = branch

    def clear_deepcache(self):
        self.state["deepcache"] = None


def test_the_enumerated_states():
    assert len(STATES) == 72 == len(set(STATES))
    assert MainOptions() in STATES


def test_transitions_between_every_pair_of_states():
    pairs = 0
    for have, want in itertools.product(STATES, STATES):
        calls = transitions(have, want)
        eng = SimEngine(have)
        for name, args, kw in calls:
            getattr(eng, name)(*args, **kw)                      # (a Refused fails the test with the pair's call in the traceback)
        assert MainOptions(**eng.state) == want, (have, want, calls)
        differ = {opt for opt, fields in FIELDS.items() if any(getattr(have, f) != getattr(want, f) for f in fields)}
        changed = [OPTION[name] for name, _, _ in calls]
        assert sorted(changed) == sorted(differ), (have, want, calls)      # one call per option that differs, none for any other
        if have == want:
            assert calls == []
        pairs += 1
    assert pairs == 5184


def test_the_one_being_switched_off_goes_first():
    merging, downsampling = MainOptions(tome=(0.5, 1)), MainOptions(todo=(2, 1, "nearest"))
    assert [c[0] for c in transitions(merging, downsampling)] == ["clear_tome", "set_todo"]
    assert [c[0] for c in transitions(downsampling, merging)] == ["clear_todo", "set_tome"]


def test_normalisations():
    off = MainOptions()
    assert off == (None, None, False, None, False, None)
    assert MainOptions(tome=(0.0, 8)) == off and MainOptions(todo=(1, 1, "area")) == off and MainOptions(tome_keep=True) == off
    assert MainOptions(tome=(0.0, 8), tome_keep=True) == off
    assert MainOptions(tome=(0.5, 1), tome_keep=True).tome_keep is True
    assert MainOptions(tome=(0.5, 1))._replace(tome=None, todo=(1, 2, "area")) == MainOptions(todo=(1, 2, "area"))
    assert MainOptions(tome=(0.5, 2), tome_keep=1)._replace(tome=(0.0, 2)) == off               # _replace normalises as well
    assert MainOptions(freeu=[1, 2, 3, 4]).freeu == (1.0, 2.0, 3.0, 4.0) and MainOptions(deepcache=0).deepcache == 0
