"""The grouping grid of ``tests/_group_cases.py`` is populated, its order-free checker accepts the
sequential reference on every case and rejects every named mutant (CPU half of
``tests/test_gpu_grouping.py``). A mutant no case detects would mean the cases are too weak, not
that the kernels are right."""

import functools

import numpy as np
import pytest

from tests import _group_cases as GC


@pytest.mark.parametrize("name", GC.NAMES)
def test_checker_accepts_the_reference(name):
    cs = GC.case(name)
    assert GC.failures(cs, None) == []
    # the reference's own permutation is the stable one: slots ascend with the arrival row in a group
    s = cs.spec
    starts, Xg, inv = GC.ref_group_rows(cs.X, s.ldx, s.F, cs.codes, s.K)
    for k in range(min(s.K, 16)):
        at = inv[cs.codes.astype(np.int64) == k]
        assert np.array_equal(at, np.arange(starts[k], starts[k + 1]))


@functools.lru_cache(maxsize=None)
def _caught(mutant):
    return tuple(n for n in GC.NAMES if GC.failures(GC.case(n), mutant))


@pytest.mark.parametrize("mutant", list(GC.MUTANTS))
def test_checker_rejects_the_mutant(mutant):
    by = _caught(mutant)
    some = ", ".join(by[:6]) + (" ..." if len(by) > 6 else "")
    print(f"{mutant:20s} caught by {len(by):2d} of {len(GC.NAMES)} cases: {some}")
    assert len(by) >= 2, (mutant, by)


def test_mutants_are_caught_where_they_apply():
    """Which entry point sees which mutant (the table docs/PARITY.md prints)."""
    seen = {m: set() for m in GC.MUTANTS}
    for m in GC.MUTANTS:
        for n in _caught(m)[:4]:
            seen[m] |= {f.split(":")[0].split("-")[0] for f in GC.failures(GC.case(n), m)}
    both = {"group_rows", "group_slice"}
    assert all(seen[m] == both for m in ("slot-off-by-one", "shared-slot", "inclusive-prefix", "codes-u16",
                                         "pad-copied"))
    assert all(seen[m] == {"group_slice"} for m in ("no-model-counted", "tiles-floor", "tiles-code-order",
                                                    "counts-not-cleared", "ticket-not-reset", "invalid-unanswered"))
    assert all(seen[m] == {"ungroup"} for m in ("ungroup-no-gather", "second-pair-skipped"))


def test_grid_contains_what_it_claims():
    cases = [GC.case(n) for n in GC.NAMES]
    specs = [c.spec for c in cases]
    assert {s.code_bytes for s in specs} == {1, 2, 4}
    assert {s.n for s in specs} >= {1, 255, 256, 257, 4095, 4096, 4097, 12289}
    for cb, ks in ((1, {1, 2, 200, 255, 256}), (2, {2, 256, 257, 1024}), (4, {1, 255, 257, 1024})):
        assert {s.K for s in specs if s.code_bytes == cb} >= ks
    # layouts: every F x pitch; both copy paths; VEC4 with a pitch; VEC4 lost to either base alone
    assert {(s.F, s.pad) for s in specs} >= {(F, p) for F in (1, 3, 4, 5, 16) for p in (0, 1, 4)}
    assert {s.vec4 for s in specs} == {True, False}
    assert any(s.vec4 and s.F == 4 and s.ldx == 8 for s in specs)
    assert any(s.F % 4 == 0 and s.ldx % 4 == 0 and (s.x_off, s.xg_off) == (1, 0) for s in specs)
    assert any(s.F % 4 == 0 and s.ldx % 4 == 0 and (s.x_off, s.xg_off) == (0, 1) for s in specs)
    assert {c.count_workgroups for c in cases} >= {1, 2, 4}
    # codes: invalid ones of every kind; uint8 with K = 256 has none
    for c in cases:
        v = c.codes.astype(np.int64)
        bad = (v < 0) | (v >= c.spec.K)
        if c.spec.code_bytes == 1 and c.spec.K == 256:
            assert not bad.any()
        if c.spec.name == "k200-u8":
            assert (v >= 200).any() and (v[bad] >= 200).all()
        if c.spec.dist == "invalid":
            assert bad.all()
    assert any((c.codes.astype(np.int64) < 0).any() for c in cases if c.spec.code_bytes == 2)
    assert sum((c.codes.astype(np.int64) == 1 << 20).any() for c in cases if c.spec.code_bytes == 4) >= 2
    assert any(len(set(c.codes.tolist())) == 1 and c.spec.dist == "one" for c in cases)
    # entries: empty first, last and middle ones; a group ending on a tile boundary, one a row past it
    # and a single row; no entries; as many entries as the kernel allows; about half the codes without a model
    first = last = middle = on_tile = past_tile = single = 0
    for c in cases:
        ec = c.entry_counts()
        assert c.n_entries < 2 or not np.array_equal(c.order, np.sort(c.order))  # never the identity
        if c.n_entries >= 3 and ec.any():
            first += ec[0] == 0
            last += ec[-1] == 0
            middle += (ec[1:-1] == 0).any()
        tr = c.tile_rows[c.order[:c.n_entries]]
        on_tile += ((ec > 0) & (ec % tr == 0)).any()
        past_tile += (ec == tr + 1).any()
        single += (ec == 1).any()
    assert min(first, last, middle, on_tile, past_tile, single) >= 2, (first, last, middle, on_tile, past_tile, single)
    assert sum(c.n_entries == 0 and len(GC.tables(c.spec.K, "none")[1]) == 0 for c in cases) >= 2
    assert any(c.n_entries == c.spec.K == GC.GROUP_MAXK for c in cases)
    assert any(c.n_entries == 257 for c in cases)
    half = [c for c in cases if c.spec.models == "half"]
    assert len(half) >= 2 and all(abs(2 * int((c.tile_rows == 0).sum()) - c.spec.K) <= 1 for c in half)
    assert all((c.codes.astype(np.int64)[:, None] == np.flatnonzero(c.tile_rows == 0)[None, :16]).any() for c in half)
    assert {int(t) for c in cases for t in c.tile_rows} == {0, 64, 128, 256}
    # the back-to-back sequence shares one set of tables and changes n and the codes
    seq = [GC.case(n) for n in GC.SEQUENCE]
    assert len({(c.spec.K, c.spec.models, c.spec.code_bytes, c.spec.F) for c in seq}) == 1
    assert len({c.spec.n for c in seq}) == len(seq) and seq[0].count_workgroups == 4
    assert seq[2].spec.dist == "invalid" and seq[1].count_workgroups == 2


def test_rows_are_named_and_bit_equality_means_something():
    for name in ("n4097", "f5-p1", "k1024-i16"):
        cs = GC.case(name)
        s = cs.spec
        assert np.array_equal(cs.X[:, 0].view(np.float32), np.arange(s.n, dtype=np.float32))
        body = cs.X[:, 1:s.F]
        if body.size:
            f = body.view(np.float32)
            assert np.isnan(f).any() and np.isinf(f).any() and (body == 0x80000000).any()  # NaN, inf, -0.0
            assert (body == 0x00000001).any() and (body == 0x7FC00001).any()  # a subnormal, a NaN payload
        assert (cs.X[:, s.F:] >> 16 == 0xBAD0).all()
    # a misplaced row is named: swap two slots of the reference and read the message
    cs = GC.case("f5-p1")
    out = {k: v.copy() for k, v in GC.emulate_group_rows(cs).items()}
    Xg = GC.body(out["Xg"], cs.spec.n * cs.spec.F, cs.spec.xg_off).reshape(cs.spec.n, cs.spec.F)
    Xg[[0, 1]] = Xg[[1, 0]]
    with pytest.raises(AssertionError, match=r"slot 0 should hold row \d+ .* names row \d+"):
        GC.check_group_rows(cs, out)


def test_fleet_of_the_grouped_tree_launch():
    """CPU: the documents ``tests/test_gpu_grouping.py`` scores lower to the wide perfect kernel in
    two launch groups (depths 4 and 6, different tree counts, one model with field preparation),
    their oracle scores are exact in fp32, and the slices hold the crafted counts."""
    import torch

    from flink_jpmml_amd.runtime import plans as PL
    from flink_jpmml_amd.runtime.compiled import CompiledPmml
    from tests import _boundary as B

    X, codes = GC.fleet_inputs(), GC.fleet_codes()
    keys, trees = {}, {}
    for k, txt in enumerate(GC.fleet_documents()):
        if txt is None:
            continue
        c = CompiledPmml.from_string(txt)
        with PL.lowering_dry_run():
            plan = PL.TreePlan(c, torch.device("cpu"), layout="perfect", variant="wide")
        got = plan.grouped_args(GC.FLEET_F)
        assert got is not None and got[3] == 256 and plan.n_features == GC.FLEET_F
        keys[k], trees[k] = got[2], plan.n_trees
        assert (plan.prep is not None) == GC.FLEET[k][3]
        ref, vref = c.score_matrix_oracle(X[codes == k])
        B.assert_fp32_exact(ref, vref)
        assert vref.all() != GC.FLEET[k][3] and vref.mean() > 0.5
    for depth, group in zip((4, 6), GC.FLEET_GROUPS):
        assert len({keys[k] for k in group}) == 1 and keys[group[0]][0] == depth
        assert len({trees[k] for k in group}) == len(group)
    per = [np.bincount(codes[s:s + GC.FLEET_SLICE], minlength=len(GC.FLEET))
           for s in range(0, len(codes), GC.FLEET_SLICE)]
    assert len(per) == 5 and len(codes) == GC.FLEET_ROWS <= 13000
    assert (per[0][[0, 7]] == 0).all() and (per[1][[3, 5]] == 0).all() and (per[3][[1, 6]] == 0).all()
    assert per[0][[1, 2, 3]].tolist() == [256, 257, 1] and per[1][[6, 7, 0]].tolist() == [256, 257, 1]
    assert all((p > 0).all() for p in (per[2], per[4]))
