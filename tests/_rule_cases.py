"""AssociationModel documents whose rule-ranking situations are placed by construction, an
independent row-at-a-time reference over Python sets, a direct ``rules_launch`` harness with guard
elements, and named one-word mutants of the packed tables (``ops/rules.py``).

Every case has categorical "slot" fields ``s0 .. s{n-1}``: string fields that declare every item
value plus ``"zz"`` (a value that names no item), so the fp32 code ``k`` of a slot is item ``k`` and
code ``n_items`` is ``"zz"``; a missing slot is NaN. Some cases add a numeric field ``num`` whose
items are ``"3"``, ``"0.5"`` and ``"0.1"``: fp32 3.0 and 0.5 name their items, fp32 0.1 prints as
``0.10000000149011612`` and names none. Measures come from a grid of quarters, so equal measures are
everywhere and the tie rule (document order) decides; ``lift`` / ``leverage`` / ``affinity`` are absent
from a third of the rules.
"""

import math

import numpy as np

NAN = float("nan")
MEASURES = ("support", "confidence", "lift", "leverage", "affinity")
ALGORITHMS = ("recommendation", "exclusiveRecommendation", "ruleAssociation")
STRINGS = ("antecedent", "consequent", "rule", "ruleId")
NUMERIC_ITEMS = ("3", "0.5", "0.1")
GUARD = 64  # sentinel floats before and after the matrix
SENTINEL = np.float32(7.0)


def bits(a):
    """fp32 bit patterns, every NaN as one pattern (NaN equals NaN)."""
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float32))
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


# --------------------------------------------------------------------------- document builders


def out(name, rule_feature="consequent", algorithm="exclusiveRecommendation", rank=1, basis="confidence",
        order="descending", feature="ruleValue"):
    return dict(name=name, feature=feature, rule_feature=rule_feature, algorithm=algorithm, rank=rank, basis=basis,
                order=order)


def hot_pool(n_items, want=12):
    """Item indices on the word, register and LDS edges, then the lowest ones."""
    edges = [0, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1023, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17]
    pool = []
    for k in edges:
        if k < n_items and k not in pool:
            pool.append(k)
    return pool[:max(1, min(want, n_items))]


def make_case(name, n_items, n_rules, slots, outputs, seed, numeric=False, set_sizes=(0, 1, 1, 2, 2), n_rows=40,
              ids=True, mining=None, pool=12, fill=0.7):
    """A random document over a hot pool of items plus hand-placed rows: all missing, every slot
    filled, one item through two slots, ``"zz"``, a slot past the vocabulary (``returnInvalid``)."""
    rng = np.random.default_rng(seed)
    items = [f"i{k}" for k in range(n_items)]
    hot = hot_pool(n_items, pool)
    if numeric:
        for k, t in zip(hot[:3], NUMERIC_ITEMS):  # the numeric items sit in the hot pool
            items[k] = t
    itemsets, index = [], {}

    def itemset(members):
        key = tuple(sorted(members))
        if key not in index:
            index[key] = len(itemsets)
            itemsets.append(list(key))
        return index[key]

    quarters = (0.25, 0.5, 0.75, 1.0)
    rules = []
    for k in range(n_rules):
        na = min(int(rng.choice(set_sizes)), len(hot))
        nc = min(max(1, int(rng.choice(set_sizes))), n_items)
        ante = [int(v) for v in rng.choice(hot, size=na, replace=False)]
        # consequents mix hot items (inside many baskets) with cold ones (never inside)
        src = hot if rng.random() < 0.7 or n_items == len(hot) else list(range(n_items))
        cons = [int(v) for v in rng.choice(src, size=min(nc, len(src)), replace=False)]
        r = dict(antecedent=itemset(ante), consequent=itemset(cons), support=float(rng.choice(quarters)),
                 confidence=float(rng.choice(quarters)), id=f"r{k}" if ids else None)
        for m in ("lift", "leverage", "affinity"):
            r[m] = float(rng.choice(quarters)) if rng.random() < 0.67 else None
        rules.append(r)
    zz = float(n_items)
    F = slots + (1 if numeric else 0)
    X = np.full((n_rows, F), NAN, dtype=np.float32)
    for i in range(n_rows):
        for j in range(slots):
            u = rng.random()
            if u < fill:
                X[i, j] = float(rng.choice(hot))
            elif u < fill + 0.05:
                X[i, j] = zz
        if numeric:
            X[i, slots] = rng.choice(np.array([3.0, 0.5, 0.1, 2.0, NAN], dtype=np.float32))
    X[0, :] = NAN  # all missing
    X[1, :slots] = [float(hot[j % len(hot)]) for j in range(slots)]  # every slot filled
    if numeric:
        X[1, slots] = 3.0
    if slots >= 2:
        X[2, :] = NAN
        X[2, 0] = X[2, 1] = float(hot[0])  # one item through two fields
        X[3, 0] = zz  # a value naming no item
        X[4, 0] = zz + 5.0  # past the vocabulary: invalid, returnInvalid rejects the row
    return dict(name=name, items=items, itemsets=itemsets, rules=rules, slots=slots, numeric=numeric,
                outputs=outputs, X=X, mining=mining or {}, hot=hot)


def document(case, outputs=None):
    items, slots = case["items"], case["slots"]
    values = "".join(f'<Value value="{t}"/>' for t in items + ["zz"])
    dd = [f'<DataField name="s{j}" optype="categorical" dataType="string">{values}</DataField>' for j in range(slots)]
    ms = [f'<MiningField name="s{j}" {case["mining"].get(j, "")}/>' for j in range(slots)]
    if case["numeric"]:
        dd.append('<DataField name="num" optype="continuous" dataType="double"/>')
        ms.append('<MiningField name="num"/>')
    of = []
    for o in (outputs if outputs is not None else case["outputs"]):
        rf = f' ruleFeature="{o["rule_feature"]}"' if o["feature"] == "ruleValue" else ""
        dt = ' dataType="double"' if o["rule_feature"] in MEASURES and o["feature"] == "ruleValue" else ""
        of.append(f'<OutputField name="{o["name"]}" feature="{o["feature"]}"{rf} algorithm="{o["algorithm"]}" '
                  f'rank="{o["rank"]}" rankBasis="{o["basis"]}" rankOrder="{o["order"]}"{dt}/>')
    its = "".join(f'<Item id="{k}" value="{t}"/>' for k, t in enumerate(items))
    sets = "".join(f'<Itemset id="{k}" numberOfItems="{len(s)}">' + "".join(f'<ItemRef itemRef="{i}"/>' for i in s)
                   + "</Itemset>" for k, s in enumerate(case["itemsets"]))
    rl = []
    for r in case["rules"]:
        extra = "".join(f' {m}="{r[m]!r}"' for m in ("lift", "leverage", "affinity") if r[m] is not None)
        rid = f' id="{r["id"]}"' if r["id"] is not None else ""
        rl.append(f'<AssociationRule{rid} support="{r["support"]!r}" confidence="{r["confidence"]!r}"{extra} '
                  f'antecedent="{r["antecedent"]}" consequent="{r["consequent"]}"/>')
    return ('<?xml version="1.0"?><PMML version="4.3" xmlns="http://www.dmg.org/PMML-4_3"><Header/>'
            f'<DataDictionary numberOfFields="{len(dd)}">{"".join(dd)}</DataDictionary>'
            f'<AssociationModel modelName="{case["name"]}" functionName="associationRules" numberOfTransactions="100" '
            f'minimumSupport="0.1" minimumConfidence="0.1" numberOfItems="{len(items)}" '
            f'numberOfItemsets="{len(case["itemsets"])}" numberOfRules="{len(rl)}">'
            f'<MiningSchema>{"".join(ms)}</MiningSchema><Output>{"".join(of)}</Output>'
            f'{its}{sets}{"".join(rl)}</AssociationModel></PMML>')


# ten (basis, order) pairs and three algorithms, dealt round the cases four groups at a time
_GROUPS = [(b, o) for b in MEASURES for o in ("descending", "ascending")]


def _outputs(start, ranks, n_groups=4):
    """``n_groups`` scan groups from position ``start`` of the deal, the ranks spread over them,
    string and measure features alternating."""
    feats = ("consequent", "confidence", "ruleId", "lift", "rule", "affinity", "antecedent", "leverage", "support")
    outs = []
    for g in range(n_groups):
        basis, order = _GROUPS[(start + g) % len(_GROUPS)]
        alg = ALGORITHMS[(start + g) % 3]
        for r in ranks[g::n_groups] or ranks[:1]:
            f = feats[(len(outs) + start) % len(feats)]
            outs.append(out(f"o{len(outs)}_{alg[:3]}_{basis[:3]}_{order[:3]}_{r}", f, alg, r, basis, order))
    outs.append(out(f"o{len(outs)}_id", algorithm=ALGORITHMS[start % 3], basis=_GROUPS[start % 10][0],
                    order=_GROUPS[start % 10][1], feature="entityId"))
    return outs


def _cases():
    r8 = list(range(1, 9))
    c = []
    # one item, one rule, one field: the empty antecedent matches every row, rank 2 never exists
    one = make_case("one", 1, 1, 1, [out("c1", algorithm="recommendation"), out("c2", "ruleId", "recommendation", 2),
                                     out("x1", "confidence"), out("a1", "rule", "ruleAssociation")], 1,
                    set_sizes=(0,), n_rows=8)
    c.append(one)
    c.append(make_case("i31", 31, 63, 2, _outputs(0, [1, 2, 3]), 31, numeric=True))  # F = 3
    c.append(make_case("i32", 32, 64, 3, _outputs(4, [1, 2, 4]), 32, ids=False))
    c.append(make_case("i33", 33, 65, 8, _outputs(8, [1, 3, 5]), 33))
    c.append(make_case("i64", 64, 257, 8, _outputs(2, r8), 64, fill=0.9))
    c.append(make_case("i65", 65, 63, 7, _outputs(6, [1, 2, 3, 4]), 65, numeric=True,
                       mining={1: 'missingValueReplacement="i33"'}))  # F = 8
    c.append(make_case("i128", 128, 64, 8, _outputs(1, [1]), 128))  # rank 1 alone: the R = 1 instantiation
    c.append(make_case("i129", 129, 65, 8, _outputs(5, [1, 2, 6]), 129))
    c.append(make_case("i1024", 1024, 4096, 8, _outputs(3, r8, n_groups=2), 1024, n_rows=24, fill=0.9))
    # 128 fields (64 rows per workgroup) and 16-item itemsets over a pool the full rows cover
    c.append(make_case("f128", 33, 257, 128, _outputs(7, [1, 2, 7, 8]), 7, set_sizes=(1, 2, 16, 16), pool=20,
                       n_rows=24, fill=0.5))
    # 64 fields and 129 items: 128 rows per workgroup with the basket in LDS
    c.append(make_case("f64", 129, 64, 64, _outputs(9, [1, 2]), 9, n_rows=24, fill=0.3))
    return c


CASES = _cases()
CASE = {c["name"]: c for c in CASES}


def five_groups():
    """``i33`` asking for a fifth scan group."""
    c = CASE["i33"]
    extra = out("fifth", "ruleId", "recommendation", 1, "support", "ascending")
    assert (extra["algorithm"], extra["basis"], extra["order"]) not in {(o["algorithm"], o["basis"], o["order"])
                                                                       for o in c["outputs"]}
    return document(c, c["outputs"] + [extra]), "fifth"


def compiled_of(text):
    from flink_jpmml_amd.api.pmml_model import PmmlModel

    return PmmlModel.from_string(text)


_MODELS = {}


def model(name):
    """The parsed case, once per process."""
    if name not in _MODELS:
        _MODELS[name] = compiled_of(document(CASE[name]))
    return _MODELS[name]


# --------------------------------------------------------------------------- reference


def _text(v):
    """A numeric field's value as an item would be written: ``3`` for 3.0, else the shortest repr."""
    return str(int(v)) if v == math.floor(v) and abs(v) < 1e15 else repr(v)


def _set_text(vals):
    vals = sorted(vals)
    return vals[0] if len(vals) == 1 else "{" + ",".join(vals) + "}"


def reference(case, compiled):
    """Row at a time over Python sets, from the case's own lists and the prepared rows. Returns
    ``(columns, facts)``: per Output field the list of Python values (str, float or None; None on a
    rejected row), and the tallies of what the rows exercised."""
    items, slots = case["items"], case["slots"]
    vocab = items + ["zz"]
    P, ok = compiled.prepare(np.asarray(case["X"], dtype=np.float64))
    sets = [frozenset(items[i] for i in s) for s in case["itemsets"]]
    rules = case["rules"]
    facts = set()
    cols = {o["name"]: [] for o in case["outputs"]}
    raw = np.asarray(case["X"])
    for i in range(len(P)):
        if not ok[i]:
            facts.add("returnInvalid row")
            for o in case["outputs"]:
                cols[o["name"]].append(None)
            continue
        basket, seen = set(), []
        for j in range(slots):
            v = P[i, j]
            if math.isnan(v):
                continue
            t = vocab[int(v)]
            if t == "zz":
                facts.add("value naming no item")
                continue
            if t in seen:
                facts.add("item through two fields")
            seen.append(t)
            basket.add(t)
            if math.isnan(raw[i, j]):
                facts.add("missingValueReplacement item")
        if case["numeric"] and not math.isnan(P[i, slots]):
            t = _text(float(P[i, slots]))
            if t in items:
                basket.add(t)
                facts.add(f"numeric item {t}")
            else:
                facts.add("numeric value naming no item")
        if np.isnan(raw[i]).all() and not basket:
            facts.add("all-missing row")
        if slots and not np.isnan(raw[i, :slots]).any() and len(seen) == slots:
            facts.add("every slot filled")
        match = {}
        for alg in ALGORITHMS:
            ks = []
            for k, r in enumerate(rules):
                a, c = sets[r["antecedent"]], sets[r["consequent"]]
                if not all(x in basket for x in a):
                    continue
                whole = all(x in basket for x in c)
                if alg == "exclusiveRecommendation" and whole:
                    continue
                if alg == "ruleAssociation" and not whole:
                    continue
                if alg == "exclusiveRecommendation" and any(x in basket for x in c):
                    facts.add("consequent partly inside, still recommended")
                ks.append(k)
            match[alg] = ks
        for alg in ALGORITHMS:
            if all(match[alg] != match[b] for b in ALGORITHMS if b != alg):
                facts.add(f"{alg} differs from the other two")
        for o in case["outputs"]:
            ks = match[o["algorithm"]]
            basis = o["basis"]
            have = [k for k in ks if rules[k][basis] is not None]
            lack = [k for k in ks if rules[k][basis] is None]
            if o["order"] == "ascending":  # a rule without the measure ranks before every value
                ranked = lack + sorted(have, key=lambda k: (rules[k][basis], k))
            else:  # and after every value when descending
                ranked = sorted(have, key=lambda k: (-rules[k][basis], k)) + lack
            if lack and have and basis in ("lift", "leverage", "affinity"):
                facts.add(f"rules lacking {basis}, {o['order']}")
            r = o["rank"]
            n = len(ranked)
            facts.add(f"rank {r}")
            facts.add(f"basis {basis} {o['order']}")
            facts.add("0 matches" if n == 0 else "rank - 1 matches" if n == r - 1 else "rank matches" if n == r
                      else "more matches" if n > r else "fewer matches")
            if n >= r:
                k = ranked[r - 1]
                tied = [q for q in ks if rules[q][basis] == rules[k][basis]]
                if len(tied) > 1 and ranked != sorted(ranked):
                    facts.add("tie to document order, unlike sorted order")
                rule = rules[k]
                f = "ruleId" if o["feature"] == "entityId" else o["rule_feature"]
                if f in MEASURES:
                    val = NAN if rule[f] is None else float(rule[f])
                elif f == "antecedent":
                    val = _set_text(sets[rule["antecedent"]])
                elif f == "consequent":
                    val = _set_text(sets[rule["consequent"]])
                elif f == "rule":
                    val = "{" + ",".join(sorted(sets[rule["antecedent"]])) + "}->{" + \
                          ",".join(sorted(sets[rule["consequent"]])) + "}"
                else:
                    val = rule["id"] if rule["id"] is not None else str(k + 1)
                cols[o["name"]].append(val)
            else:
                cols[o["name"]].append(NAN if o["rule_feature"] in MEASURES and o["feature"] == "ruleValue" else None)
    # what the document itself places
    facts.add(f"items {len(items)}")
    facts.add(f"rules {len(rules)}")
    facts.add(f"F {slots + (1 if case['numeric'] else 0)}")
    used = {r["antecedent"] for r in rules} | {r["consequent"] for r in rules}
    for s in used:
        facts.add(f"itemset size {len(case['itemsets'][s])}")
        if len({i >> 5 for i in case["itemsets"][s]}) > 1:
            facts.add("itemset straddles a word edge")
    facts.add(f"groups {len({(o['algorithm'], o['basis'], o['order']) for o in case['outputs']})}")
    return cols, facts


_REFERENCE = {}


def expected(name):
    """``(columns, facts)`` of a case, computed once and never changed."""
    if name not in _REFERENCE:
        _REFERENCE[name] = reference(CASE[name], model(name).compiled)
    return _REFERENCE[name]


REQUIRED = (
    [f"items {n}" for n in (1, 31, 32, 33, 64, 65, 128, 129, 1024)]
    + [f"rules {n}" for n in (1, 63, 64, 65, 257, 4096)]
    + [f"itemset size {n}" for n in (0, 1, 2, 16)] + ["itemset straddles a word edge"]
    + [f"F {n}" for n in (1, 3, 8, 128)]
    + [f"{a} differs from the other two" for a in ALGORITHMS]
    + [f"rank {r}" for r in range(1, 9)]
    + ["0 matches", "rank - 1 matches", "rank matches", "more matches"]
    + [f"basis {b} {o}" for b in MEASURES for o in ("descending", "ascending")]
    + ["tie to document order, unlike sorted order"]
    + [f"rules lacking {b}, {o}" for b in ("lift", "leverage", "affinity") for o in ("descending", "ascending")]
    + ["consequent partly inside, still recommended", "item through two fields", "value naming no item",
       "all-missing row", "every slot filled", "missingValueReplacement item", "returnInvalid row",
       "numeric item 3", "numeric item 0.5", "numeric value naming no item", "groups 4"])


def is_numeric(o):
    return o["feature"] == "ruleValue" and o["rule_feature"] in MEASURES


def compare(case, cols, matrix, decode, rows=None):
    """``matrix`` (``[n, fields]``, any float type) and ``decode(name)`` against the reference columns
    of the case (row ``i`` of the matrix is reference row ``rows[i]``): numeric fields as fp32 bits,
    string fields as decoded strings. Returns the list of mismatches."""
    n = matrix.shape[0]
    rows = np.arange(n) if rows is None else np.asarray(rows)
    bad = []
    for j, o in enumerate(case["outputs"]):
        want = [cols[o["name"]][r] for r in rows]
        if is_numeric(o):
            w = np.array([NAN if v is None else v for v in want], dtype=np.float32)
            if not np.array_equal(bits(matrix[:, j]), bits(w)):
                bad.append((o["name"], "bits"))
        else:
            got = decode(o["name"])
            if got != want:
                bad.append((o["name"], next((i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w)))
    return bad


# --------------------------------------------------------------------------- plan, twin, direct launch


def dry_plan(name):
    """``(model, output plan)`` of a case lowered on the host with ``association_rules=True``."""
    from flink_jpmml_amd.runtime.plans import lowering_dry_run

    m = model(name)
    with lowering_dry_run():
        return m, m.compiled.output_plan("cpu", association_rules=True)


def twin(plan, X, tables=None, **kw):
    """The numpy twin over the raw rows ``X`` into a matrix of sentinels."""
    from flink_jpmml_amd.ops.rules import rules_numpy

    T = tables if tables is not None else plan.rules
    X = np.ascontiguousarray(X, dtype=np.float32)
    full = np.full((len(X), T.width), SENTINEL, dtype=np.float32)
    prep = plan.prep.numpy() if plan.prep is not None else None
    return rules_numpy(X, full, T, prep=prep, **kw)


def launch_direct(T, X, prep, device, layout="contiguous", stream=None):
    """``rules_launch`` on device copies of ``X`` laid out as ``layout`` says, into a matrix that
    sits between ``GUARD`` sentinels (and, for ``wide``, has sentinel columns to its right).
    Returns ``(matrix, everything else of the buffer)`` as numpy."""
    import torch

    from flink_jpmml_amd.ops.rules import rules_launch

    n, F = X.shape
    Xh = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32))
    if layout == "wide":  # rows 5 floats apart from each other's end: no 16-byte alignment of the rows
        buf = torch.full((n, F + 5), float("nan"), dtype=torch.float32, device=device)
        buf[:, :F] = Xh.to(device)
        Xd = buf[:, :F]
        ldo = T.width + 3
    elif layout == "misaligned":  # the matrix starts one float past an aligned address
        flat = torch.full((n * F + 1,), float("nan"), dtype=torch.float32, device=device)
        flat[1:] = Xh.to(device).reshape(-1)
        Xd = flat[1:].view(n, F)
        ldo = T.width
    else:
        Xd = Xh.to(device)
        ldo = T.width
    whole = torch.full((2 * GUARD + n * ldo,), float(SENTINEL), dtype=torch.float32, device=device)
    out = whole[GUARD:GUARD + n * ldo].view(n, ldo)[:, :T.width]
    pd = torch.from_numpy(np.ascontiguousarray(prep)).to(device) if prep is not None else None
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream(device))
    rules_launch(Xd, out, T, prep=pd, stream=stream)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize(device)
    host = whole.cpu().numpy()
    body = host[GUARD:GUARD + n * ldo].reshape(n, ldo)
    rest = np.concatenate([host[:GUARD], body[:, T.width:].reshape(-1), host[GUARD + n * ldo:]])
    return body[:, :T.width].copy(), rest


def retabled(T, **over):
    from flink_jpmml_amd.ops.rules import RuleTables

    kw = {k: getattr(T, k).copy() for k in RuleTables._ARRAYS}
    kw.update(n_items=T.n_items, width=T.width)
    kw.update(over)
    return RuleTables(**kw)


# --------------------------------------------------------------------------- mutants


def _top_pair(T):
    """The first pair of the best-ranked rule of group 0 whose antecedent is not empty."""
    for k in T.order[0]:
        p0, cnt = T.sets[T.rules[k][0]]
        if cnt:
            return int(p0)
    raise AssertionError("no rule with an antecedent")


def _cleared_bit(case, plan):
    T = plan.rules
    pairs = T.pairs.copy()
    p = _top_pair(T)
    pairs[p, 1] &= pairs[p, 1] - np.uint32(1)  # the lowest set bit
    return twin(plan, case["X"], retabled(T, pairs=pairs))


def _moved_pair(case, plan):
    T = plan.rules
    pairs = T.pairs.copy()
    p = _top_pair(T)
    W = (T.n_items + 31) // 32
    pairs[p, 0] = (pairs[p, 0] + 1) % W
    return twin(plan, case["X"], retabled(T, pairs=pairs))


def _swapped_order(case, plan):
    """The first and second match of group 0 on the first row that has both trade places."""
    T = plan.rules
    index = np.append(np.arange(T.n_rules, dtype=np.float32), np.float32(NAN))  # a column table of rule indices
    probe = twin(plan, case["X"], retabled(T, cols=[(0, 0, 0, 0), (0, 1, 0, 1)], tables=index))
    a, b = next((int(r[0]), int(r[1])) for r in probe if r[0] == r[0] and r[1] == r[1])
    order = T.order.copy()
    ia, ib = list(order[0]).index(a), list(order[0]).index(b)
    order[0, [ia, ib]] = order[0, [ib, ia]]
    return twin(plan, case["X"], retabled(T, order=order))


def _any_overlap(basket, T, first, count):
    """The wrong exclusive test: some item of the consequent is inside."""
    r = np.zeros(len(basket), dtype=bool)
    for w, mask in T.pairs[first:first + count]:
        r |= (basket[:, w] & mask) != 0
    return r


def _exclusive_per_item(case, plan):
    from flink_jpmml_amd.ops import rules as R

    old = R._excluded
    R._excluded = _any_overlap
    try:
        return twin(plan, case["X"])
    finally:
        R._excluded = old


def _r_one_short(case, plan):
    return twin(plan, case["X"], r=plan.rules.k - 1)


def _neighbour_group(case, plan):
    T = plan.rules
    cols = T.cols.copy()
    cols[0, 0] = (cols[0, 0] + 1) % len(T.groups)
    return twin(plan, case["X"], retabled(T, cols=cols))


def _ulp_off(case, plan):
    T = plan.rules
    nvals = T.nvals.copy()
    nvals[0] = np.nextafter(nvals[0], np.float32(np.inf))
    return twin(plan, case["X"], retabled(T, nvals=nvals))


# name -> (the case it belongs to, what runs it)
MUTANTS = {
    "a cleared mask bit": ("i65", _cleared_bit),
    "a pair moved to the neighbouring word": ("i65", _moved_pair),
    "two rules swapped in one group's order": ("i64", _swapped_order),
    "the exclusive test per item, not on the whole consequent": ("i33", _exclusive_per_item),
    "R one short": ("i64", _r_one_short),
    "a column reading the neighbouring group's match": ("i33", _neighbour_group),
    "a numeric item list one ulp off": ("i65", _ulp_off),
}
