"""The host lowering of :class:`TreePlan`, pinned on the CPU: for a grid of documents and options,
what the constructor decides (every ``_STATE`` value, every packed tensor by SHA-256) and every
argument block the plan hands to a launcher, field by field, against ``golden/tree_plan_pins.json``.

The fixture was recorded from the constructor before it was split into per-layout builders and is
never regenerated from later code: a change to this file's expectations is a change of behaviour.
``python tests/test_tree_plan_pins.py`` writes the fixture; pytest only reads it.

Pointer fields are recorded by what they point at (a state tensor's name, ``X`` / ``score`` /
``valid`` / ``probs`` / ``score2`` / ``valid2`` / ``_partial``, or null), floats as ``float.hex()``.
An argument block is the list of its values in ``_fields_`` order (nested structs flattened,
``epi.mode`` ...).

The file stores each record in full but sparsely (``_pack`` / ``_unpack``, lossless): a block as
the fields that differ from the case's previous block of that struct (the first: from the
commonest values, ``__args__``), a batch size or a launch call as what differs from the one before
it (the first: from ``__first__``), a plan's meta as the keys that differ from the commonest value
(``__meta__``), ``__none__`` only where it is not the None-valued keys in ``__state__`` order, and
each SHA-256 as an index into ``__sha256__``."""

import ctypes
import functools
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.test_general_tree import general_tree_doc  # noqa: E402
from tests.test_gpu_boundary import MISSING, PATHS, tree_case  # noqa: E402

from flink_jpmml_amd.bench.synth import gbdt_pmml, random_forest_pmml  # noqa: E402
from flink_jpmml_amd.ops import _lib as L  # noqa: E402
from flink_jpmml_amd.runtime import plans as PL  # noqa: E402
from flink_jpmml_amd.runtime.compiled import CompiledPmml  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tree_plan_pins.json")
ROWS = 300
FAKE = {0x1000: "X", 0x2000: "score", 0x3000: "valid"}  # batch_launch_args takes raw addresses
ENTRY_POINTS = ("pmml_tree_launch", "pmml_tree_hybrid_launch", "pmml_tree_lds_launch", "pmml_tree_general_launch")


# --------------------------------------------------------------------------- the grid


@functools.lru_cache(maxsize=None)
def _compiled(key: str):
    return CompiledPmml.from_string(DOCS[key]())


DOCS = {
    "small": lambda: gbdt_pmml(n_trees=19, depth=5, n_features=8, seed=1),
    "deep": lambda: gbdt_pmml(n_trees=70, depth=11, n_features=8, seed=1, p_split=0.6),
    "deep12": lambda: gbdt_pmml(n_trees=70, depth=12, n_features=8, seed=1, p_split=0.6),
    "deep-f80": lambda: gbdt_pmml(n_trees=70, depth=11, n_features=80, seed=1, p_split=0.6),
    "deep-rf": lambda: random_forest_pmml(n_trees=70, depth=11, n_features=8, n_classes=3, seed=1, p_split=0.6),
    "seventy": lambda: gbdt_pmml(n_trees=70, depth=6, n_features=8, seed=1),
    "chain3": lambda: gbdt_pmml(n_trees=12, depth=5, n_features=10, objective="multiclass", n_classes=3, seed=3),
    "chain12": lambda: gbdt_pmml(n_trees=10, depth=4, n_features=12, objective="multiclass", n_classes=12, seed=2),
    "forest3": lambda: random_forest_pmml(n_trees=40, depth=6, n_features=12, n_classes=3, seed=1),
    "forest6": lambda: random_forest_pmml(n_trees=30, depth=5, n_features=12, n_classes=6, seed=3),
    "f100": lambda: gbdt_pmml(n_trees=30, depth=6, n_features=100, seed=100),
    "f200": lambda: gbdt_pmml(n_trees=30, depth=6, n_features=200, seed=200),
    "f300": lambda: gbdt_pmml(n_trees=3, depth=2, n_features=300, seed=7),
    "general-reg": lambda: general_tree_doc(4, "defaultChild", "returnLastPrediction", n_trees=5),
    "general-cls": lambda: general_tree_doc(4, "defaultChild", "returnLastPrediction", n_trees=5,
                                            classification=True),
}

PROBS, SECOND = dict(probs=True), dict(second=True)
# (b) id -> (document, plan options, launch options of the second launch)
EXTRA = {
    "chain3-slots": ("chain3", {}, PROBS),
    "chain12-slots": ("chain12", {}, PROBS),
    "chain3-narrow-stumps": ("chain3", dict(layout="perfect", variant="narrow"), PROBS),
    "chain12-narrow-stumps": ("chain12", dict(layout="perfect", variant="narrow"), {}),
    "chain3-pointer-compact": ("chain3", dict(layout="pointer", node_format="compact"), {}),
    "forest3-vote8": ("forest3", {}, PROBS),
    "forest6-mode-class": ("forest6", {}, PROBS),
    "f100-rows128": ("f100", {}, SECOND),
    "f200-rows64": ("f200", {}, {}),
    "f300-feat-map": ("f300", {}, {}),
    "fp8": ("small", dict(precision="fp8"), SECOND),
    "tree-shard-1-of-3": ("small", dict(tree_shard=(1, 3)), {}),
    "auto-depth12": ("deep12", {}, dict(splits=4)),
    "pointer-f80": ("deep-f80", dict(layout="pointer"), {}),
    "hybrid-head6": ("deep", dict(layout="hybrid", head_depth=6), dict(splits=4)),
    "hybrid-wide-uskip": ("deep", dict(layout="hybrid", hybrid_tail="wide", pointer_load="uskip"), {}),
    "max-chunk-16": ("seventy", dict(max_chunk_trees=16), {}),
    "max-chunk-16-narrow": ("seventy", dict(max_chunk_trees=16, variant="narrow"), {}),
    "ltop-ilp6": ("deep", dict(layout="pointer", pointer_load="ltop", pointer_ilp=6), {}),
    "node-format-auto": ("deep", dict(layout="pointer", node_format="auto"), {}),
    "node-format-auto-rf": ("deep-rf", dict(layout="pointer", node_format="auto"), PROBS),
    "dfs-peel": ("deep", dict(layout="pointer", node_order="dfs"), {}),
    "pointer-rf-onehot": ("deep-rf", dict(layout="pointer"), PROBS),
    "general-regression": ("general-reg", {}, SECOND),
    "general-classification": ("general-cls", {}, PROBS),
}
# (c) one invalid value per validated option
INVALID = {
    "bad-nan-mode": dict(nan_mode="on"),
    "bad-pointer-ilp": dict(pointer_ilp=5),
    "bad-pointer-ilp-3": dict(pointer_ilp=3),
    "bad-pointer-schedule": dict(pointer_schedule="greedy"),
    "bad-pointer-load": dict(pointer_load="scalar"),
    "bad-hybrid-tail": dict(hybrid_tail="bfs"),
    "bad-pointer-leaf": dict(pointer_leaf="pair"),
    "bad-xcd-split": dict(xcd_split="auto"),
    "bad-precision": dict(precision="bf16"),
    "bad-head-depth": dict(layout="hybrid", head_depth=5),
    "bad-tree-shard": dict(tree_shard=(3, 3)),
}


def _cases():
    out = {}
    for name, depth, F, opts, launch, models, _ in PATHS:  # (a)
        for model in models:
            for missing in MISSING:
                out[f"{name}-{model}-{missing}"] = (lambda m=model, d=depth, f=F, s=missing: tree_case(m, d, f, s)[1],
                                                    opts, launch)
    for cid, (doc, opts, launch) in EXTRA.items():
        out[cid] = (lambda d=doc: _compiled(d), opts, launch)
    for cid, opts in INVALID.items():
        out[cid] = (lambda: _compiled("small"), opts, {})
    return out


CASES = _cases()


# --------------------------------------------------------------------------- canonical forms


def canon(v):
    if isinstance(v, (bool, np.bool_)):
        return bool(v)
    if isinstance(v, (float, np.floating)):
        return float(v).hex()
    if isinstance(v, (int, np.integer)):
        return int(v)
    if isinstance(v, dict):
        return {str(k): canon(x) for k, x in sorted(v.items(), key=lambda kv: str(kv[0]))}
    if isinstance(v, (list, tuple)):
        return [canon(x) for x in v]
    if v is None or isinstance(v, str):
        return v
    raise TypeError(f"no canonical form for {type(v).__name__}")


def lowering(plan) -> dict:
    meta, tensors = plan.export_state()
    assert set(meta) - {"__class__", "__tensors__", "__none__"} | set(tensors) == set(plan._STATE)
    out = {"meta": canon({k: v for k, v in meta.items() if k != "__tensors__"}), "tensors": {}}
    for k, t in sorted(tensors.items()):
        shape, dtype = meta["__tensors__"][k]
        raw = t.contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()
        out["tensors"][k] = [dtype, list(shape), hashlib.sha256(raw).hexdigest()]
    return out


def _flat_names(cls, prefix=""):
    out = []
    for n, t in cls._fields_:
        out += _flat_names(t, prefix + n + ".") if issubclass(t, ctypes.Structure) else [prefix + n]
    return out


STRUCTS = (L.TreeArgs, L.HybridArgs, L.LdsTreeArgs, L.GenTreeArgs)
FIELDS = {c.__name__: _flat_names(c) for c in STRUCTS}


def block(st, names: dict) -> list:
    """The struct's values in ``_fields_`` order; pointers by the name of what they point at."""
    out = []
    for n, t in st._fields_:
        v = getattr(st, n)
        if isinstance(v, ctypes.Structure):
            out += block(v, names)
        elif t is ctypes.c_void_p:
            assert not v or v in names, f"{type(st).__name__}.{n} points at nothing the plan owns"
            out.append(names[v] if v else None)
        elif isinstance(v, bytes):
            out.append(v.hex())
        else:
            out.append(canon(v))
    return out


class Recorder:
    """Stands in for the kernel library: every attribute is a function that records its call."""

    def __init__(self, names):
        self.names, self.calls = names, []

    def __getattr__(self, entry):
        def call(stream, ref, *scalars):
            st = ref._obj
            self.calls.append({"entry": entry, "stream": stream, "scalars": [int(x) for x in scalars],
                               "struct": type(st).__name__, "args": block(st, self.names())})
            return 0

        return call


class Stream:
    cuda_stream = 0


def record(compiled, opts: dict, launch_opts: dict) -> dict:
    try:
        with PL.lowering_dry_run():
            plan = PL.TreePlan(compiled, torch.device("cpu"), **opts)
    except PL.NotLowerable as e:
        return {"lowering": f"NotLowerable: {e}"}
    except ValueError as e:
        return {"lowering": f"ValueError: {e}"}
    out = {"lowering": lowering(plan)}
    F = compiled.n_features
    C = max(1, int(plan.C))
    X, score = torch.zeros((ROWS, F)), torch.zeros(ROWS)
    valid = torch.zeros(ROWS, dtype=torch.uint8)
    extra = {"probs": torch.zeros((ROWS, C)), "score2": torch.zeros(ROWS),
             "valid2": torch.zeros(ROWS, dtype=torch.uint8)}
    private = []

    def names():
        m = dict(FAKE)
        for k, t in [("X", X), ("score", score), ("valid", valid), *extra.items()]:
            m[t.data_ptr()] = k
        for t in [plan._partial, *private]:
            if t is not None:
                m[t.data_ptr()] = "_partial"
        for k in plan._STATE:  # state tensors last: they win over nothing, and the first of equals wins
            t = getattr(plan, k)
            if isinstance(t, torch.Tensor) and t.data_ptr():
                m.setdefault(t.data_ptr(), k)
        return m

    def partial_numel():
        return None if plan._partial is None else int(plan._partial.numel())

    out["batch"] = {}
    for n in (1, 300, 5000):
        got = plan.batch_launch_args(0x1000, n, F, F, 0x2000, 0x3000)
        out["batch"][str(n)] = None if got is None else {
            "args": block(got[0], names()), "launch": canon(got[1]), "partial_numel": partial_numel()}
    got = plan.grouped_args(max(F, 8))
    out["grouped"] = None if got is None else {"args": block(got[0], names()), "depth": got[1],
                                               "key": canon(got[2]), "tile_rows": got[3]}
    run = plan.row_launcher(X, score, valid)
    if run is None:
        out["row"] = None
    else:
        private.append(run.keep[1])
        out["row"] = {"args": block(run.keep[0], names()),
                      "partial_numel": None if run.keep[1] is None else int(run.keep[1].numel())}
    plan.lib = Recorder(names)
    plan.launch(X, score, valid, stream=Stream())
    if launch_opts:
        kw = {}
        if "splits" in launch_opts:
            kw["splits"] = launch_opts["splits"]
        if launch_opts.get("probs"):
            kw["probs"] = extra["probs"]
        if launch_opts.get("second"):
            kw["score2"], kw["valid2"] = extra["score2"], extra["valid2"]
        plan.launch(X, score, valid, stream=Stream(), **kw)
    assert all(c["entry"] in ENTRY_POINTS for c in plan.lib.calls)
    out["launch"] = {"calls": plan.lib.calls, "partial_numel": partial_numel()}
    return json.loads(json.dumps(out))


# --------------------------------------------------------------------------- the test


def _blocks(rec, fn) -> None:
    """Replace every argument block of a record by ``fn(struct, block)``, in a fixed order."""
    if isinstance(rec, dict):
        if "args" in rec:
            rec["args"] = fn(rec.get("struct", "TreeArgs"), rec["args"])
        for k in sorted(rec):
            if k != "args":
                _blocks(rec[k], fn)
    elif isinstance(rec, list):
        for v in rec:
            _blocks(v, fn)


def _derived_none(meta: dict, state) -> list:
    return [k for k in state if k in meta and meta[k] is None]


def _commonest(values: list):
    texts = [json.dumps(v, sort_keys=True) for v in values]
    return json.loads(max(sorted(set(texts)), key=texts.count))


def _repeats(r: dict) -> list:
    """Lists of dicts that mostly repeat their predecessor: the batch sizes, the launch calls."""
    return [[r["batch"][n] for n in ("1", "300", "5000")], r["launch"]["calls"]]


def _pack(cases: dict) -> dict:
    cases = json.loads(json.dumps(cases))
    state = list(PL.TreePlan._STATE)
    fix = {"__fields__": FIELDS, "__state__": state}
    lowered = [r for r in cases.values() if not isinstance(r["lowering"], str)]
    for r in lowered:
        meta = r["lowering"]["meta"]
        if meta["__none__"] == _derived_none(meta, state):
            del meta["__none__"]
    keys = sorted({k for r in lowered for k in r["lowering"]["meta"]})
    common = fix["__meta__"] = {k: _commonest([r["lowering"]["meta"][k] for r in lowered if k in r["lowering"]["meta"]])
                                for k in keys}
    shas = fix["__sha256__"] = sorted({t[2] for r in lowered for t in r["lowering"]["tensors"].values()})
    seen = {}
    _blocks(lowered, lambda struct, args: seen.setdefault(struct, []).append(args) or args)
    first = fix["__args__"] = {s: [_commonest(col) for col in zip(*blocks)] for s, blocks in sorted(seen.items())}
    for r in lowered:
        meta = r["lowering"]["meta"]
        r["lowering"]["meta"] = {"+": {k: v for k, v in meta.items() if k not in common or common[k] != v},
                                 "-": sorted(k for k in common if k not in meta)}
        for t in r["lowering"]["tensors"].values():
            t[2] = shas.index(t[2])
        prev = {}

        def sparse(struct, args):
            base = prev.get(struct, first[struct])
            prev[struct] = args
            return {n: v for n, v, b in zip(FIELDS[struct], args, base) if v != b}

        _blocks(r, sparse)
        for seq in _repeats(r):
            for before, cur in reversed(list(zip(seq, seq[1:]))):
                if isinstance(before, dict) and isinstance(cur, dict):
                    for k in [k for k in cur if k in before and before[k] == cur[k]]:
                        del cur[k]
    heads = [[seq[0] for seq in (_repeats(r)[i] for r in lowered) if isinstance(seq[0], dict)] for i in (0, 1)]
    fix["__first__"] = [{k: _commonest([h[k] for h in hs]) for k in sorted(hs[0])} for hs in heads]
    for r in lowered:
        for seq, usual in zip(_repeats(r), fix["__first__"]):
            if isinstance(seq[0], dict):
                for k in [k for k in seq[0] if usual[k] == seq[0][k]]:
                    del seq[0][k]
    fix["cases"] = cases
    return fix


def _unpack(fix: dict) -> dict:
    fix = json.loads(json.dumps(fix))
    for r in fix["cases"].values():
        if isinstance(r["lowering"], str):
            continue
        sp = r["lowering"]["meta"]
        meta = {k: v for k, v in fix["__meta__"].items() if k not in sp["-"]}
        meta.update(sp["+"])
        meta.setdefault("__none__", _derived_none(meta, fix["__state__"]))
        r["lowering"]["meta"] = meta
        for t in r["lowering"]["tensors"].values():
            t[2] = fix["__sha256__"][t[2]]
        for seq, usual in zip(_repeats(r), fix["__first__"]):
            if isinstance(seq[0], dict):
                for k in usual:
                    seq[0].setdefault(k, usual[k])
            for before, cur in zip(seq, seq[1:]):
                if isinstance(before, dict) and isinstance(cur, dict):
                    for k in before:
                        cur.setdefault(k, before[k])
        prev = {}

        def dense(struct, sp):
            args = list(prev.get(struct, fix["__args__"][struct]))
            for n, v in sp.items():
                args[fix["__fields__"][struct].index(n)] = v
            prev[struct] = args
            return args

        _blocks(r, dense)
    return json.loads(json.dumps(fix))


@functools.lru_cache(maxsize=None)
def _golden():
    with open(GOLDEN) as fh:
        return _unpack(json.load(fh))


def _named(rec, fields):
    """Argument blocks as {field: value} (for a readable failure)."""
    if isinstance(rec, dict):
        if "args" in rec and isinstance(rec["args"], list):
            names = fields[rec.get("struct", "TreeArgs")]
            rec = dict(rec, args=dict(zip(names, rec["args"])) if len(names) == len(rec["args"]) else rec["args"])
        return {k: _named(v, fields) for k, v in rec.items()}
    if isinstance(rec, list):
        return [_named(v, fields) for v in rec]
    return rec


def _differences(a, b, path=""):
    if isinstance(a, dict) and isinstance(b, dict):
        out = []
        for k in sorted(set(a) | set(b)):
            if k not in a or k not in b:
                out.append(f"{path}/{k}: {'missing' if k not in a else a[k]!r} != {'missing' if k not in b else b[k]!r}")
            else:
                out += _differences(a[k], b[k], f"{path}/{k}")
        return out
    if isinstance(a, list) and isinstance(b, list) and len(a) == len(b):
        return [d for i, (x, y) in enumerate(zip(a, b)) for d in _differences(x, y, f"{path}[{i}]")]
    return [] if a == b else [f"{path}: {a!r} != {b!r}"]


def test_the_grid_is_the_fixture_and_the_structs_are_its_fields():
    g = _golden()
    assert g["__fields__"] == FIELDS and g["__state__"] == list(PL.TreePlan._STATE)
    assert sorted(g["cases"]) == sorted(CASES)
    assert len([c for c in CASES if c.split("-")[-1] in MISSING]) == 92
    refused = [c for c, r in g["cases"].items() if isinstance(r["lowering"], str)]
    assert sorted(c for c in refused if c.startswith("pointer-rank3")) == [
        "pointer-rank3-gbdt-nullPrediction", "pointer-rank3-rf-nullPrediction"]
    assert sorted(c for c in refused if c.startswith("bad-")) == sorted(INVALID)


@pytest.mark.parametrize("cid", sorted(CASES))
def test_lowering_and_argument_blocks_equal_the_pinned_ones(cid):
    build, opts, launch_opts = CASES[cid]
    got, want = record(build(), opts, launch_opts), _golden()["cases"][cid]
    if got != want:
        f = _golden()["__fields__"]
        diff = _differences(_named(got, FIELDS), _named(want, f))
        pytest.fail(f"{cid}: {len(diff)} difference(s) from the pinned record (got != pinned):\n" + "\n".join(diff[:40]))


def _write_fixture() -> None:
    cases = {cid: record(build(), opts, launch_opts) for cid, (build, opts, launch_opts) in sorted(CASES.items())}
    fix = _pack(cases)
    assert _unpack(fix)["cases"] == json.loads(json.dumps(cases))
    packed = fix.pop("cases")
    head = [json.dumps(k) + ": " + json.dumps(v, sort_keys=True, separators=(",", ":")) for k, v in sorted(fix.items())]
    lines = [json.dumps(cid) + ": " + json.dumps(packed[cid], sort_keys=True, separators=(",", ":")) for cid in sorted(packed)]
    with open(GOLDEN, "w") as fh:
        fh.write("{" + ",\n".join(head) + ',\n"cases": {\n' + ",\n".join(lines) + "\n}}\n")
    print(f"wrote {len(cases)} cases, {os.path.getsize(GOLDEN)} bytes: {GOLDEN}")


if __name__ == "__main__":
    _write_fixture()
