"""Association rules on the device: ``rules.hip`` alone, the whole ``OutputPlan.launch`` and the host
path, on two synthetic documents over rows resident in HBM.

* ``small``: 64 items, 256 rules, 8 slot fields; ``consequent`` of rank 1 … 3 and the rank-1
  ``confidence`` in one scan group (``recommendation`` by confidence);
* ``large``: 1024 items, 4096 rules, 16 slot fields; ``ruleId`` of rank 1 … 8 (``recommendation`` by
  confidence) and ``consequent`` of rank 1 … 8 (``exclusiveRecommendation`` by lift): two scan groups.

Every slot field is a string field over the item values. Antecedents hold one or two items of a hot
pool (32 / 64 items), consequents one item. Three row sets per document: ``many`` (every slot holds a
hot item: the scan ends early), ``none`` (every slot holds an item no antecedent names: no rule
matches, the full-scan worst case) and ``mixed`` (the two alternating wave by wave, 64 rows each).

Timed with device events over ``REPEAT`` rounds after ``WARMUP``, the row sets alternating launch by
launch; the median is reported. The host path (``predict_batch_outputs`` without a device: the Python
loop of ``models/association.py``) is timed on ``HOST_ROWS[name]`` rows of the ``mixed`` set and
reported per row with the number of rows it was timed on. Run from the repository root on a machine
with a GPU::

    python profiles/rules/measure.py [rows] > results.json
"""

import json
import sys
import time

import numpy as np

ROWS = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
HOST_ROWS = {"small": 20_000, "large": 500}  # large: 4096 rules x 16 fields per row in Python
WARMUP, REPEAT = 3, 10

SHAPES = {
    "small": dict(n_items=64, n_rules=256, slots=8, hot=32,
                  fields=[("c%d" % r, "consequent", "recommendation", r, "confidence") for r in (1, 2, 3)]
                  + [("conf", "confidence", "recommendation", 1, "confidence")]),
    "large": dict(n_items=1024, n_rules=4096, slots=16, hot=64,
                  fields=[("id%d" % r, "ruleId", "recommendation", r, "confidence") for r in range(1, 9)]
                  + [("c%d" % r, "consequent", "exclusiveRecommendation", r, "lift") for r in range(1, 9)]),
}


def document(n_items, n_rules, slots, hot, fields, seed=1):
    """The document, the hot items and a cold item (in no antecedent)."""
    rng = np.random.default_rng(seed)
    values = "".join(f'<Value value="i{k}"/>' for k in range(n_items))
    dd = "".join(f'<DataField name="s{j}" optype="categorical" dataType="string">{values}</DataField>'
                 for j in range(slots))
    ms = "".join(f'<MiningField name="s{j}"/>' for j in range(slots))
    of = "".join(f'<OutputField name="{n}" feature="ruleValue" ruleFeature="{f}" algorithm="{a}" rank="{r}" '
                 f'rankBasis="{b}"' + (' dataType="double"/>' if f == "confidence" else "/>")
                 for n, f, a, r, b in fields)
    pool = rng.permutation(n_items)[:hot]
    cold = int(next(k for k in range(n_items) if k not in set(pool.tolist())))
    items = "".join(f'<Item id="{k}" value="i{k}"/>' for k in range(n_items))
    sets, index, rules = [], {}, []

    def itemset(members):
        key = tuple(sorted(int(m) for m in members))
        if key not in index:
            index[key] = len(sets)
            sets.append(key)
        return index[key]

    for k in range(n_rules):
        a = itemset(rng.choice(pool, size=int(rng.integers(1, 3)), replace=False))
        c = itemset([rng.integers(0, n_items)])
        rules.append(f'<AssociationRule id="r{k}" support="{rng.integers(1, 100) / 100}" '
                     f'confidence="{rng.integers(1, 100) / 100}" lift="{rng.integers(1, 400) / 100}" '
                     f'antecedent="{a}" consequent="{c}"/>')
    st = "".join(f'<Itemset id="{k}" numberOfItems="{len(s)}">' + "".join(f'<ItemRef itemRef="{i}"/>' for i in s)
                 + "</Itemset>" for k, s in enumerate(sets))
    text = ('<?xml version="1.0"?><PMML version="4.3" xmlns="http://www.dmg.org/PMML-4_3"><Header/>'
            f'<DataDictionary numberOfFields="{slots}">{dd}</DataDictionary>'
            f'<AssociationModel functionName="associationRules" numberOfTransactions="1000" minimumSupport="0.01" '
            f'minimumConfidence="0.01" numberOfItems="{n_items}" numberOfItemsets="{len(sets)}" '
            f'numberOfRules="{n_rules}"><MiningSchema>{ms}</MiningSchema><Output>{of}</Output>'
            f'{items}{st}{"".join(rules)}</AssociationModel></PMML>')
    return text, pool, cold


def row_sets(rows, slots, pool, cold, seed=2):
    rng = np.random.default_rng(seed)
    many = rng.choice(pool, size=(rows, slots)).astype(np.float32)
    none = np.full((rows, slots), float(cold), dtype=np.float32)
    wave = (np.arange(rows) // 64) % 2 == 0
    return {"many": many, "none": none, "mixed": np.where(wave[:, None], many, none)}


def timed_alternating(fns: dict) -> dict:
    """Every function once per round, round after round: neighbours in time share the device's state."""
    import torch

    for _ in range(WARMUP):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(REPEAT):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v))}
            for k, v in ms.items()}


def main() -> None:
    import torch

    from flink_jpmml_amd.api.pmml_model import PmmlModel
    from flink_jpmml_amd.ops.rules import geometry, rules_launch, template_r

    assert torch.cuda.is_available(), "this measurement needs a GPU"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "rows": ROWS, "warmup": WARMUP, "repeat": REPEAT, "cases": {}}
    for name, shape in SHAPES.items():
        text, pool, cold = document(**shape)
        model = PmmlModel.from_string(text)
        plan = model.compiled.output_plan(dev, association_rules=True)
        T = plan.rules
        host_sets = row_sets(ROWS, shape["slots"], pool, cold)
        X = {k: torch.from_numpy(v).to(dev) for k, v in host_sets.items()}
        score, valid = plan.alloc_outputs(ROWS)
        matrix = plan.alloc_matrix(ROWS)
        entry = {"items": T.n_items, "rules": T.n_rules, "fields": T.n_feat, "columns": len(T.cols),
                 "scan_groups": len(T.groups), "R": template_r(T.k),
                 "rows_per_workgroup": geometry(T.n_feat, T.n_items), "basket": "registers" if T.n_items <= 128 else "LDS"}
        fns = {}
        for k in X:
            fns[f"kernel_{k}"] = lambda k=k: rules_launch(X[k], matrix, T, prep=plan.prep)
            fns[f"plan_launch_{k}"] = lambda k=k: plan.launch(X[k], score, valid, outputs=matrix)
        entry.update(timed_alternating(fns))
        plan.launch(X["mixed"], score, valid, outputs=matrix)
        torch.cuda.synchronize()
        n_host = HOST_ROWS[name]
        got = matrix[:n_host].cpu().numpy()
        t0 = time.perf_counter()
        _, _, host = model.predict_batch_outputs(host_sets["mixed"][:n_host])
        dt = time.perf_counter() - t0
        entry["host_rows_timed"] = n_host
        entry["host_microseconds_per_row"] = dt * 1e6 / n_host
        want = np.asarray(host.matrix, dtype=np.float32)
        entry["host_compared_values_that_differ"] = int(((got != want) & ~(np.isnan(got) & np.isnan(want))).sum())
        entry["rows_with_a_match_in_the_compared_slice"] = int((~np.isnan(want[:, 0])).sum())
        res["cases"][name] = entry
        print(name, json.dumps(entry), file=sys.stderr, flush=True)
        del X, matrix
        torch.cuda.empty_cache()
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    sys.path.insert(0, ".")
    main()
