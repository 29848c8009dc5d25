"""Class outputs of k-NN classifiers on the MI355X: the class-output instantiation of ``knn.hip``
through ``KnnPlan.launch(probs=)``, ``OutputPlan(knn_classes=True)`` and the public routes. Exact
documents (``_knn_vote_cases``) match the float64 oracle in every bit; inexact unweighted documents
match ``float32(count / k)`` wherever the oracle decides the neighbours; inexact weighted documents
match the float64 share of the device's own neighbours within ``SHARE_ULPS * 2^-24``."""

import numpy as np
import pytest

import _entity_cases as EC
import _knn_vote_cases as VC
from _exact import strided
from flink_jpmml_amd.api.pmml_model import PmmlModel
from flink_jpmml_amd.runtime.outputs import oracle_outputs, oracle_top_k

pytestmark = pytest.mark.gpu

GUARD = 7.0
ROW_COUNTS = (1, 33, 255, 256, 257)
TOP = 3
SQ, CITY = VC.EXACT_METRICS
# |device share - float64 share of the device's own neighbours| <= SHARE_ULPS * 2^-24: four times the
# largest ratio measured on the MI355X over the weighted inexact documents (1.98: knn64k5, MFMA), rounded up
SHARE_ULPS = 8.0

# (N, k, C, method, metric, knn_variant): k in {2, 8, 9, 32} on both KMAX instantiations, N = 33 below
# and N = 65 above the MFMA threshold of 64 instances, C in {2, 3, 40, 256}
SHAPES = [
    (33, 2, 2, "weighted", SQ, "valu"), (33, 8, 3, "weighted", CITY, "valu"), (33, 9, 40, "weighted", SQ, "valu"),
    (33, 32, 256, "weighted", CITY, "valu"), (65, 9, 3, "majority", CITY, "auto"), (65, 32, 2, "majority", SQ, "valu"),
    (33, 8, 40, "majority", "euclidean", "valu"), (33, 9, 3, "majority", "chebychev", "valu"),
    (33, 9, 256, "majority", 'minkowski p-parameter="3"', "valu"), (65, 8, 3, "majority", "euclidean", "auto"),
    (33, 2, 3, "weighted", SQ, "mfma"), (33, 8, 256, "weighted", SQ, "mfma"), (33, 9, 2, "weighted", SQ, "mfma"),
    (33, 32, 40, "majority", SQ, "mfma"), (65, 2, 40, "weighted", SQ, "auto"), (65, 8, 2, "weighted", SQ, "auto"),
    (65, 9, 256, "weighted", SQ, "auto"), (65, 32, 3, "weighted", SQ, "auto"),
]
HAND = [(n, v) for n, c in sorted(VC.EXACT.items()) if n.startswith("hand")
        for v in (("valu", "mfma") if c["metric"] in (SQ, "euclidean") else ("valu",))]


def _expect_variant(c, variant):
    if variant != "auto":
        return variant
    return "mfma" if c["metric"] in (SQ, "euclidean") and len(c["inst"]) >= 64 else "valu"


def _check_exact(gpu, c, variant, what):
    """Raw index / validity / shares of the index-mode plan, the columns and top-k of the output plan
    and its score against the scoring plan, for every row count."""
    import torch

    compiled = PmmlModel.from_string(VC.document(c, VC.class_outputs(c))).compiled
    plan = compiled.output_plan(gpu, knn_classes=True, top_k=TOP, knn_variant=variant)
    inner = plan.inner
    assert type(inner).__name__ == "KnnPlan" and inner.class_table is None
    assert inner.variant == _expect_variant(c, variant), what
    scoring = compiled.plan(gpu, knn_variant=variant)
    assert scoring.class_table is not None
    C = len(c["categories"])
    Xall = VC.rows(c, max(ROW_COUNTS))
    s, v, cols, res, ok = oracle_outputs(compiled, Xall, top_k=TOP)
    lab, valid, shares = VC.reference(c, Xall)
    assert np.array_equal(valid, np.asarray(res.valid, dtype=bool) & ok)
    ti, tp = oracle_top_k(res.probs, valid, TOP)
    for n in ROW_COUNTS:
        X = torch.from_numpy(Xall[:n]).to(gpu)
        raw_s, raw_v = inner.alloc_outputs(n)
        probs = torch.full((n, C), GUARD, dtype=torch.float32, device=gpu)
        inner.launch(X, raw_s, raw_v, probs=probs)
        sc, va, mat = plan.score_outputs(Xall[:n])
        s0, v0 = scoring.score(Xall[:n])
        torch.cuda.synchronize()
        assert np.array_equal(raw_v.cpu().numpy() != 0, valid[:n]), (what, n)
        assert np.array_equal(VC.bits(raw_s.cpu().numpy()), VC.bits(lab[:n])), (what, n)
        assert np.array_equal(VC.bits(probs.cpu().numpy()), VC.bits(shares[:n])), (what, n)
        mat = mat.cpu().numpy()
        for i, name in enumerate(plan.names):
            assert np.array_equal(VC.bits(mat[:, i]), VC.bits(cols[name][:n])), (what, n, name)
        w = len(plan.names)
        assert np.array_equal(np.nan_to_num(mat[:, w: w + TOP], nan=-1).astype(np.int64), ti[:n]), (what, n)
        assert np.array_equal(VC.bits(mat[:, w + TOP:]), VC.bits(tp[:n])), (what, n)
        assert np.array_equal(VC.bits(sc.cpu().numpy()), VC.bits(s0.cpu().numpy())), (what, n)
        assert np.array_equal(va.cpu().numpy() != 0, v0.cpu().numpy() != 0), (what, n)
        assert np.array_equal(VC.bits(sc.cpu().numpy()), VC.bits(s[:n])), (what, n)


@pytest.mark.parametrize("N,k,C,method,metric,variant", SHAPES)
def test_exact_shapes(gpu, N, k, C, method, metric, variant):
    _check_exact(gpu, VC.generated(N, k, C, method, metric), variant, (N, k, C, method, metric, variant))


@pytest.mark.parametrize("name,variant", HAND)
def test_exact_hand_made_votes(gpu, name, variant):
    _check_exact(gpu, VC.EXACT[name], variant, (name, variant))


@pytest.mark.parametrize("N,k,C,method,variant", [(33, 9, 3, "weighted", "valu"), (65, 8, 40, "weighted", "auto"),
                                                  (33, 32, 3, "majority", "mfma")])
def test_layouts_guards_and_a_side_stream(gpu, N, k, C, method, variant):
    """A contiguous input and a column view of a wider matrix; ``outputs`` a view with guard columns
    and guard elements around it; ``probs`` between guard rows (C = 3: its base is not 16-byte
    aligned); the launches on a side stream."""
    import torch

    c = VC.generated(N, k, C, method)
    compiled = PmmlModel.from_string(VC.document(c, VC.class_outputs(c))).compiled
    plan = compiled.output_plan(gpu, knn_classes=True, top_k=TOP, knn_variant=variant)
    n, W, pad = 261, plan.width, 3
    Xn = VC.rows(c, n)
    _, _, cols, res, ok = oracle_outputs(compiled, Xn, top_k=TOP)
    lab, valid, shares = VC.reference(c, Xn)
    side = torch.cuda.Stream(device=gpu)
    for layout in ("contiguous", "view"):
        Xt = torch.from_numpy(Xn).to(gpu) if layout == "contiguous" else \
            torch.from_numpy(strided(Xn)).to(gpu)[:, : Xn.shape[1]]
        buf = torch.full((2 + n * (W + pad) + 2,), GUARD, dtype=torch.float32, device=gpu)
        out = buf[2: 2 + n * (W + pad)].view(n, W + pad)[:, :W]
        score, vout = plan.alloc_outputs(n)
        pbuf = torch.full((n + 2, C), GUARD, dtype=torch.float32, device=gpu)
        raw_s, raw_v = plan.inner.alloc_outputs(n)
        torch.cuda.synchronize()
        plan.launch(Xt, score, vout, stream=side, outputs=out)
        plan.inner.launch(Xt, raw_s, raw_v, stream=side, probs=pbuf[1: n + 1])
        side.synchronize()
        host = buf.cpu().numpy()
        body = host[2: 2 + n * (W + pad)].reshape(n, W + pad)
        assert (host[:2] == GUARD).all() and (host[-2:] == GUARD).all() and (body[:, W:] == GUARD).all(), layout
        for i, name in enumerate(plan.names):
            assert np.array_equal(VC.bits(body[:, i]), VC.bits(cols[name])), (layout, name)
        p = pbuf.cpu().numpy()
        assert (p[0] == GUARD).all() and (p[-1] == GUARD).all(), layout
        assert np.array_equal(VC.bits(p[1:-1]), VC.bits(shares)), layout
        assert np.array_equal(VC.bits(raw_s.cpu().numpy()), VC.bits(lab)), layout


def test_launcher_rejects_what_it_cannot_take(gpu):
    import torch

    from flink_jpmml_amd.bench import synth

    reg = PmmlModel.from_string(synth.knn_pmml(40, 4, k=3, classification=False)).compiled.plan(gpu)
    X = torch.zeros((5, 4), device=gpu)
    s, v = reg.alloc_outputs(5)
    with pytest.raises(ValueError, match="no class vote shares"):
        reg.launch(X, s, v, probs=torch.zeros((5, 3), device=gpu))
    cls = PmmlModel.from_string(synth.knn_pmml(40, 4, k=3)).compiled.plan(gpu)
    with pytest.raises(ValueError, match="contiguous"):
        cls.launch(X, s, v, probs=torch.zeros((5, 6), device=gpu)[:, ::2])
    reg.labels, reg.inst_class = ["0", "1", "2"], cls.inst_class  # past the plan's own check: the launcher's
    with pytest.raises(Exception, match="-4"):
        reg.launch(X, s, v, probs=torch.zeros((5, 3), device=gpu))


@pytest.mark.parametrize("name,variant", [("hand5_weighted_sq", "valu"), ("c40k3_weighted", "auto")])
def test_public_routes(gpu, name, variant):
    """``predict_batch_outputs(knn_classes=True)`` and ``ScoringConfig(knn_classes=True,
    fallback="error")`` through ``predict_records(outputs=True)``: the oracle's columns, the host's
    label strings."""
    from flink_jpmml_amd.api.batch import RecordBatch
    from flink_jpmml_amd.config import ScoringConfig

    c = VC.EXACT[name]
    text = VC.document(c, VC.class_outputs(c))
    X = VC.rows(c, 70)
    model = PmmlModel.from_string(text)
    hs, hv, host = model.predict_batch_outputs(X, top_k=TOP)
    s, v, outs = model.predict_batch_outputs(X, device=gpu, knn_classes=True, top_k=TOP, knn_variant=variant)
    assert np.array_equal(v.cpu().numpy() != 0, hv)
    outs = outs.numpy()
    for n in outs.names:
        assert np.array_equal(VC.bits(outs[n]), VC.bits(host[n])), n
    assert outs.decode("lab") == host.decode("lab") and None in outs.decode("lab")
    assert np.array_equal(np.asarray(outs.top_index), host.top_index)
    assert np.array_equal(VC.bits(outs.top_probability), VC.bits(host.top_probability))
    bound = PmmlModel.from_string(text).bind(gpu, ScoringConfig(device=gpu, knn_classes=True, fallback="error"))
    assert bound.on_device
    pb = bound.predict_records(RecordBatch(X), outputs=True)
    assert np.array_equal(np.asarray(pb.valid, dtype=bool), hv)
    assert pb.outputs.decode("lab") == host.decode("lab")
    served = pb.outputs.numpy()
    for n in ("pwin", "p_nobody", outs.names[3]):
        assert np.array_equal(VC.bits(served[n]), VC.bits(host[n])), n
    strict = PmmlModel.from_string(text).bind(gpu, ScoringConfig(device=gpu, fallback="error"))
    with pytest.raises(Exception, match="has no index mode"):  # off: refused by name, no fall-back
        strict.predict_records(RecordBatch(X), outputs=True)


# --------------------------------------------------------------------------- inexact documents

INEXACT = VC.inexact()


def _share_fields(classes):
    return ['<OutputField name="lab" feature="predictedValue" optype="categorical" dataType="string"/>'] + \
        [f'<OutputField name="p_{x}" feature="probability" value="{x}" optype="continuous" dataType="double"/>'
         for x in range(classes)]


@pytest.mark.parametrize("name", [n for n, s in INEXACT.items() if not s["weighted"]])
@pytest.mark.parametrize("variant", ["valu", "mfma"])
def test_inexact_unweighted(gpu, name, variant):
    """Shares are ``float32(count / k)`` of the oracle in every bit wherever the oracle's k-th and
    (k+1)-th distances are an exact tie or at least twice ``2e-5 (1 + d)`` apart; labels (38 % of the
    rows are vote ties, so the rank order matters) wherever every rank <= k is decided."""
    spec = INEXACT[name]
    k, C = spec["k"], spec["classes"]
    compiled = PmmlModel.from_string(VC.with_outputs(spec["text"], _share_fields(C))).compiled
    X = VC.inexact_rows(1000)
    _, _, cols, res, ok = oracle_outputs(compiled, X)
    und = EC.undecided(compiled, X, list(range(1, k + 1)))
    plan = compiled.output_plan(gpu, knn_classes=True, knn_variant=variant)
    assert plan.inner.variant == variant
    mat = plan.score_outputs(X)[2].cpu().numpy()
    got = {n: mat[:, i] for i, n in enumerate(plan.names)}
    keep = ~und[k - 1]
    print(name, variant, "shares compared on", keep.mean(), "labels on", (~und.any(axis=0)).mean())
    assert keep.mean() >= 0.995
    for x in range(C):
        want = (np.round(np.asarray(res.probs)[:, x] * k) / k).astype(np.float32)
        assert np.array_equal(VC.bits(got[f"p_{x}"][keep]), VC.bits(want[keep])), (name, variant, x)
    keep = ~und.any(axis=0)
    assert keep.mean() >= 0.95
    assert np.array_equal(VC.bits(got["lab"][keep]), VC.bits(cols["lab"][keep])), (name, variant)


@pytest.mark.parametrize("name", [n for n, s in INEXACT.items() if s["weighted"]])
@pytest.mark.parametrize("variant", ["valu", "mfma"])
def test_inexact_weighted(gpu, name, variant):
    """The same document also asks the neighbours' ids and distances (``entity_ranks=True``): the
    reference is the float64 share of the device's own neighbour classes and fp32 distances, the
    bound ``SHARE_ULPS * 2^-24`` per share; the label is compared where the reference's two largest
    totals differ by more than that bound."""
    spec = INEXACT[name]
    k, C = spec["k"], spec["classes"]
    ranked = EC.with_ranked_outputs(spec["text"], range(1, k + 1))
    text = ranked.replace("<Output>", "<Output>" + "".join(_share_fields(C)), 1)
    compiled = PmmlModel.from_string(text).compiled
    X = VC.inexact_rows(1000)
    plan = compiled.output_plan(gpu, knn_classes=True, entity_ranks=True, knn_variant=variant)
    assert plan.inner.variant == variant and plan.entities is not None
    _, va, mat = plan.score_outputs(X)
    mat = mat.cpu().numpy()
    got = {n: mat[:, i] for i, n in enumerate(plan.names)}
    ok = ~np.isnan(got["id1"])
    assert ok.all()
    ev = compiled.evaluator
    cls = np.asarray(ev.inst_class)[np.stack([got[f"id{r}"] for r in range(1, k + 1)], axis=1).astype(np.int64) - 1]
    d = np.stack([got[f"aff{r}"] for r in range(1, k + 1)], axis=1).astype(np.float64)
    w = 1.0 / (np.abs(d) + float(np.float32(ev.knn.threshold)))
    assert np.isfinite(w).all()
    votes = np.zeros((len(X), C))
    for j in range(k):
        votes[np.arange(len(X)), cls[:, j]] += w[:, j]
    want = votes / votes.sum(axis=1, keepdims=True)
    have = np.stack([got[f"p_{x}"] for x in range(C)], axis=1).astype(np.float64)
    ratio = np.abs(have - want).max() / 2.0 ** -24
    print(name, variant, "largest |device - reference| / 2^-24 =", ratio)
    assert ratio <= SHARE_ULPS
    top = np.sort(want, axis=1)
    clear = (top[:, -1] - top[:, -2]) > SHARE_ULPS * 2.0 ** -24
    assert clear.mean() >= 0.995
    lookup = compiled.schema.lookup
    codes = np.array([lookup("lab", x) for x in ev.categories], dtype=np.float32)
    assert np.array_equal(got["lab"][clear], codes[want.argmax(axis=1)][clear]), (name, variant)
