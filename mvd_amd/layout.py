"""The batch layout of a forward (csrc/ragged.h is the C++ side): an ordinary forward, V views of one
object, O objects x V views, or O objects with V_o views each, parsed once per layer from the public ``views=`` / ``objects=``."""
import numbers
from typing import NamedTuple

from ._lib import MvdError


class ViewLayout(NamedTuple):
    views: int = 0                  # the uniform V (0: an ordinary forward, or view counts)
    objects: int = 0                # O > 1 objects x ``views`` views (0: one object)
    counts: tuple = ()               # ragged: V_o per object.  Equal counts stay counts: making them uniform is the C entry's job

    @classmethod
    def parse(cls, views=None, objects=None, who: str = "forward") -> "ViewLayout":
        """``views``: ``None``, an integral value or a sequence of counts (``objects`` then ``None`` or their number).  ``who``:
        "forward" (the denoiser, ``MultiViewUNet.forward``) -- one view is no layout, objects without views have one view each;
        "engine" (``MVDEngine.forward``) -- ``views = 1`` is a shared forward of one view, objects need views; "key" (a record's
        key) -- as the engine reads them, and nothing is rejected."""
        pre = "engine.forward: " if who == "engine" else ""
        if views is not None and not isinstance(views, numbers.Integral):
            counts = tuple(int(v) for v in views)
            if who != "key" and (not counts or min(counts) < 1):
                raise MvdError(f"{pre}views={counts}: every object needs at least one view")
            if who != "key" and objects is not None and int(objects) != len(counts):
                raise MvdError(f"{pre}views={counts}: objects must be None or {len(counts)}, got {objects}")
            return cls(counts=counts)
        V = int(views) if views else 0
        O = int(objects) if objects and int(objects) > 1 else 0
        if who == "engine" and O and not V:
            raise MvdError(f"engine.forward: objects = {O} needs views")
        if who == "forward":
            V = max(V, 1) if O else (V if V > 1 else 0)
        return cls(V, O)

    @property
    def rows(self) -> int:          # views in a guidance half: the sample holds g of these (0: an ordinary forward)
        return sum(self.counts) if self.counts else self.views * max(self.objects, 1)

    @property
    def sources(self) -> int:       # reference rows (and prompts) expected: one per object (0: an ordinary forward, which takes any)
        return len(self.counts) or self.objects or (1 if self.views else 0)

    def g(self, B: int) -> int:     # rows per view of a batch of B (1, or 2 under guidance, are supported); 0: the views do not divide B
        return (0 if B % self.rows else B // self.rows) if self.rows else 1

    def text_rows(self, B: int) -> int:     # one text row per guidance half and object
        if self.counts:
            return B // self.rows * self.sources
        return B // self.views if self.views else B

    def kwargs(self) -> dict:       # the ``views=`` / ``objects=`` keywords of the next layer down
        return {"views": self.counts} if self.counts else {k: v for k, v in zip(("views", "objects"), self) if v}

    def key(self) -> tuple:         # what a record of a forward ends in (``MVDEngine._ref_key``; the workspace key leads with views or 0)
        return (self.counts,) if self.counts else tuple(v for v in self[:2] if v)
