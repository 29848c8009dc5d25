"""CPU side of the GENERAL-layout probes (tests/_general_cases.py; GPU twin: test_gpu_general.py).
For every case the float64 oracle, the plain reference walker and the kernel's numpy twin
(``runtime/general_tree.py::emulate_general``) agree on every row: validity identical, scores bit
for bit as fp32. What the rows reach is a condition, not a measurement: every leaf opcode x
negation x outcome, every compound operator x outcome, every exit kind the strategy allows, and
the full-stack 32-operand ``and`` with a deciding operand. Every named mutant of the packed
tables changes the twin's result, so a kernel with that error cannot pass the GPU file."""

import numpy as np
import pytest
import torch

from tests import _general_cases as G

from flink_jpmml_amd.runtime import plans as PL
from flink_jpmml_amd.runtime.compiled import CompiledPmml
from flink_jpmml_amd.runtime.general_tree import MAX_STACK, MIX_STACK, pack_general

F32 = np.float32


@pytest.mark.parametrize("key", G.ALL_CASES, ids=[G.case_id(k) for k in G.ALL_CASES])
def test_oracle_reference_and_twin_agree(key):
    cs = G.case(*key)
    ref, vref, probs = cs.oracle
    # the reference walker == the oracle
    assert np.array_equal(cs.valid, vref), f"validity differs on {(cs.valid != vref).sum()} rows"
    assert np.array_equal(cs.score[vref].astype(F32), ref[vref].astype(F32))
    if cs.family == "dist":
        assert np.array_equal(cs.probs[vref], probs[vref])
    # the kernel's twin == the oracle
    s, v, acc = cs.emulate()
    assert np.array_equal(v, vref), f"twin validity differs on {(v != vref).sum()} rows"
    assert np.array_equal(s[vref].astype(F32), ref[vref].astype(F32))
    if cs.family == "dist":
        assert np.array_equal(acc[vref].astype(F32), probs[vref].astype(F32))
    assert vref.any() and not vref.all()  # every case here can produce nulls


@pytest.mark.parametrize("key", G.ALL_CASES, ids=[G.case_id(k) for k in G.ALL_CASES])
def test_rows_reach_every_outcome_and_exit(key):
    cs = G.case(*key)
    w = cs.walker
    assert not [k for k in G.LEAF_OUTCOMES if not w.leaf[k]]
    assert not [k for k in G.COMPOUND_OUTCOMES if not w.compound[k]]
    allowed = G.allowed_exits(cs.strategy, cs.no_true, cs.family)
    assert not [k for k in allowed if not w.exits[k]]
    assert set(w.exits) <= set(allowed)
    # the 32-operand and: TRUE on some rows, FALSE through its first (deepest stack entry) and
    # through its last operand alone on others
    assert w.and32["true"] and w.and32["first_decides"] and w.and32["last_decides"]
    if cs.family not in ("single", "vcol"):
        assert (cs.nodes[:, 1:] >= 0).any(axis=0).all()  # every tree scores some row


@pytest.mark.parametrize("name", list(G.MUTANTS))
def test_every_mutant_changes_the_twin(name):
    cs, g = G.mutant(name)
    s0, v0, _ = cs.emulate()
    for lo in range(0, G.ROWS, 256):  # stops at the first rows that differ
        rows = slice(lo, lo + 256)
        s, v, _ = cs.emulate(g, rows)
        if not (np.array_equal(v, v0[rows]) and np.array_equal(s[v], s0[rows][v])):
            return
    raise AssertionError(f"mutant {name} changes no row of {cs.name}: the probe is blind there")


def _lowered(cs):
    with PL.lowering_dry_run():
        plan = PL.compile_plan(cs.compiled, "cpu")
    return plan, getattr(plan, "inner", plan)  # a derive pass (set splits, leaf columns) wraps the tree plan


@pytest.mark.parametrize("key", G.ALL_CASES, ids=[G.case_id(k) for k in G.ALL_CASES])
def test_every_case_lowers_to_the_general_layout(key):
    cs = G.case(*key)
    _, inner = _lowered(cs)
    assert type(inner).__name__ == "TreePlan" and inner.layout == "general"
    assert inner.n_trees >= len(cs.trees)
    assert (inner.vcol is not None) == (cs.family == "vcol")
    if cs.F > 64:  # features stay in global memory: predicates and leaf columns hold column indices
        if cs.family == "vcol":  # the derive pass hands over the columns the trees read, in order of first use
            assert 64 < inner.n_features and 0 <= int(inner.vcol.max()) < inner.n_features
        else:
            assert inner.n_features == cs.F
        preds = inner.preds.cpu().numpy().view(np.uint32).reshape(-1, 4)
        fields = preds[np.isin(preds[:, 0] & 0xFF, (3, 4, 5, 6, 7)), 1]
        assert fields.size and 8 <= int(fields.max()) < inner.n_features
        assert cs.family == "vcol" or int(fields.max()) >= 64
    else:
        assert inner.n_features <= 64


# --------------------------------------------------------------------------- limits


def _stack_doc(n: int) -> str:
    b = G.Builder(5, "single")
    ops = [G.S(b.q[i % 4], "lessThan", "1e39") for i in range(n)]
    root = G.Node(0, "r", G.TRUE, 0, score=1, children=[G.Node(1, "a", G.C("and", *ops), 1, score=2)])
    return b.document([root], "none", "returnNullPrediction", False)


def test_predicate_stack_limit():
    assert MAX_STACK == 32
    c = CompiledPmml.from_string(_stack_doc(32))
    spec = PL.TreePlan._general_spec(c)
    assert len(pack_general(spec.trees, spec.weights, spec.P, c.schema)["preds"]) == 32 + 1 + 1 + 2
    c = CompiledPmml.from_string(_stack_doc(33))
    spec = PL.TreePlan._general_spec(c)
    with pytest.raises(PL.NotLowerable):
        pack_general(spec.trees, spec.weights, spec.P, c.schema)
    with pytest.raises(PL.NotLowerable), PL.lowering_dry_run():
        PL.TreePlan(c, torch.device("cpu"), layout="general")


def _chain_doc(widths) -> str:
    """A weightedConfidence tree that is one chain: level i has ``widths[i]`` children, the first
    continues the chain. The mixture walk's DFS bound is 1 + sum(widths - 1)."""
    from tests.test_native_walk import _header, _ms

    dist = '<ScoreDistribution value="1" recordCount="2"/><ScoreDistribution value="2" recordCount="1"/>'
    count = [0]

    def node(level: int, pred: str) -> str:
        count[0] += 1
        nid = count[0]
        score = "1"
        if level == len(widths):
            return f'<Node id="n{nid}" score="{score}" recordCount="3">{pred}{dist}</Node>'
        kids = "".join(node(level + 1 if j == 0 else len(widths), f'<SimplePredicate field="f{j % 4}" '
                            f'operator="lessThan" value="{j}"/>') for j in range(widths[level]))
        return f'<Node id="n{nid}" score="{score}" recordCount="3">{pred}{dist}{kids}</Node>'

    tgt = '<DataField name="y" optype="categorical" dataType="string"><Value value="1"/><Value value="2"/>' \
          '<Value value="3"/></DataField>'
    return (_header(tgt) + '<TreeModel functionName="classification" missingValueStrategy="weightedConfidence">'
            f'{_ms()}{node(0, "<True/>")}</TreeModel></PMML>')


def test_mixture_stack_limit():
    assert MIX_STACK == 64
    c = CompiledPmml.from_string(_chain_doc([4] * 21))  # 1 + 21 * 3 = 64
    spec = PL.TreePlan._general_spec(c)
    assert pack_general(spec.trees, spec.weights, spec.P, c.schema)["mix_mass"] is not None
    c = CompiledPmml.from_string(_chain_doc([4] * 20 + [3, 3]))  # 1 + 60 + 4 = 65
    with pytest.raises(PL.NotLowerable):
        PL.TreePlan._general_spec(c)


def test_more_tree_categories_than_class_slots():
    """The packer refuses a mixture tree with more categories than the kernel has class slots."""
    c = G.mixture_case(*G.MIXTURES[0])[0]
    spec = PL.TreePlan._general_spec(c)
    assert spec.P == 3 and pack_general(spec.trees, spec.weights, 3, c.schema)["mix_tab"][0, 2] == 3
    with pytest.raises(PL.NotLowerable):
        pack_general(spec.trees, spec.weights, 2, c.schema)


# --------------------------------------------------------------------------- sibling mixtures


@pytest.mark.parametrize("key", G.MIXTURES, ids=[f"{m}-{n}-seed{s}" for s, n, m in G.MIXTURES])
def test_mixture_probes_fork_everywhere_and_labels_are_clear(key):
    """Conditions on the oracle alone: forks open at the root, at depth and inside an open
    mixture; there are valid and (for these seeds' null strategies) enough clear rows."""
    c, X, ref, vref, probs = G.mixture_case(*key)
    forks = G.mixture_forks(c, X)
    assert forks["root"] and forks["depth"] and forks["inside"], dict(forks)
    clear = G.mixture_clear(probs, vref)
    assert vref.any() and 2 * int(clear.sum()) >= int(vref.sum())


@pytest.mark.parametrize("key", G.MIXTURES, ids=[f"{m}-{n}-seed{s}" for s, n, m in G.MIXTURES])
def test_mixture_twin_on_boundary_inputs(key):
    from flink_jpmml_amd.runtime.general_tree import emulate_general

    c, X, ref, vref, probs = G.mixture_case(*key)
    spec = PL.TreePlan._general_spec(c)
    packed = pack_general(spec.trees, spec.weights, spec.P, c.schema)
    assert packed["mix_mass"] is not None
    acc = emulate_general(packed, X, spec.P, len(spec.trees))
    valid = ~np.isnan(acc).any(axis=1)
    assert np.array_equal(valid, vref)
    p = acc[valid] * spec.epi.get("a", 1.0)
    np.testing.assert_allclose(p, probs[valid], rtol=0, atol=G.MIX_ATOL)
    clear = G.mixture_clear(probs, vref)
    labels = np.array([float(x) for x in spec.labels])[np.argmax(np.nan_to_num(acc), axis=1)]
    assert np.array_equal(labels[clear], ref[clear])
