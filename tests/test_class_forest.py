"""Dry-run lowering of tree ensembles with 17 to 256 classes (``runtime/class_forest.py``): the plan
``compile_plan`` picks, what is still refused, the state round trip. Kernel: test_gpu_class_forest.py."""

import hashlib
import re

import pytest
import torch

from flink_jpmml_amd.bench.synth import gbdt_pmml, random_forest_pmml
from flink_jpmml_amd.ops import _lib
from flink_jpmml_amd.runtime import plans as PL
from flink_jpmml_amd.runtime.class_forest import ClassForestPlan
from flink_jpmml_amd.runtime.compiled import CompiledPmml

CPU = torch.device("cpu")


def single_tree(txt: str) -> str:
    """The first TreeModel of a forest document as the document's model."""
    end = "    </TreeModel>\n"
    return txt[: txt.index(" <MiningModel")] + txt[txt.index("    <TreeModel"): txt.index(end) + len(end)] + "</PMML>\n"


def document(kind: str, C: int) -> str:
    if kind == "chain":
        return gbdt_pmml(n_trees=2, depth=3, n_features=6, objective="multiclass", n_classes=C, seed=C)
    txt = random_forest_pmml(n_trees=5, depth=3, n_features=6, n_classes=C, seed=C, distributions=kind == "average",
                             method="average" if kind == "average" else "majorityVote")
    return single_tree(txt) if kind == "tree" else txt


def lower(txt: str, **opts):
    with PL.lowering_dry_run():
        return PL.compile_plan(CompiledPmml.from_string(txt), CPU, **opts)


@pytest.mark.parametrize("kind", ["forest", "average", "tree", "chain"])
def test_twenty_classes_lower_to_the_class_tile_plan_and_sixteen_stay(kind, monkeypatch):
    plan = lower(document(kind, 20))
    assert type(plan) is ClassForestPlan and plan.layout == "classes" and (plan.C, plan.Cp) == (20, 32)
    # probability leaves are DENSE; the chain's intercepts start the accumulators
    assert plan.dense == (kind in ("average", "tree")) and (plan.acc_init is not None) == (kind == "chain")
    assert plan.batch_launch_args(0, 1, 6, 6, 0, 0) is None and plan.grouped_args(6) is None
    assert type(lower(document(kind, 16))) is PL.TreePlan
    monkeypatch.setattr(_lib, "load", lambda: None)  # from_state binds the library: not needed to compare tensors
    twin = PL.DevicePlan.from_state(*plan.export_state(), CPU)
    assert type(twin) is ClassForestPlan
    for k in ClassForestPlan._STATE:
        a, b = getattr(plan, k), getattr(twin, k)
        assert torch.equal(a, b) if isinstance(a, torch.Tensor) else a == b, k


def test_what_is_still_refused():
    big = random_forest_pmml(n_trees=2, depth=2, n_features=4, n_classes=257, seed=1)
    for txt in (big, single_tree(big)):
        with pytest.raises(PL.NotLowerable, match="257 class slots: the tree kernels accumulate at most 16"):
            lower(txt)
    with pytest.raises(PL.NotLowerable):
        lower(document("forest", 20), precision="fp8")
    # a third child under the root: not a binary split, and the predicate-VM layout stays at 16 classes
    third = '<Node id="900" score="0"><SimplePredicate field="f0" operator="lessThan" value="-50"/></Node>\n'
    wide, n = re.subn(r'(<Node id="1" defaultChild="\d+"><True/>\n)', r"\1" + third, document("tree", 20), count=1)
    assert n == 1
    with pytest.raises(PL.NotLowerable, match="20 class slots"):
        lower(wide)


def test_generator_defaults_are_unchanged():
    """SHA-256 of a default-option document, recorded before the generator took its two options."""
    sha = hashlib.sha256(random_forest_pmml(n_trees=7, depth=4, n_features=5, n_classes=4, seed=11).encode())
    assert sha.hexdigest() == "d0450a4b80f7e8ab4dc330cfc9c6fe8b08cb77e307e27eec6d93169c43b63229"
