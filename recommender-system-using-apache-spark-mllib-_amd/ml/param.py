"""Param: the key of a param map (pyspark.ml.param.Param, reduced to what model selection
needs).  A Param names one parameter of one estimator class; it is hashable and equal by
(parent, name), so ``{als.rank: 8}`` and ``{ALS.rank: 8}`` are the same map."""
from __future__ import annotations

__all__ = ["Param"]


class Param:
    def __init__(self, parent: str, name: str, doc: str = ""):
        self.parent = str(parent)
        self.name = str(name)
        self.doc = doc

    def __eq__(self, other):
        return isinstance(other, Param) and (self.parent, self.name) == (other.parent, other.name)

    def __hash__(self):
        return hash((self.parent, self.name))

    def __repr__(self):
        return f"Param(parent={self.parent!r}, name={self.name!r})"

    def __str__(self):
        return f"{self.parent}__{self.name}"  # pyspark's form
