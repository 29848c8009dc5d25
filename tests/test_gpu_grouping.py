"""The row-grouping kernels (``ops/csrc/grouped.hip``) and the grouped tree launch
(``tree_common.h::tree_grouped_wide_kernel``, ``pmml_tree_launch_many``), bit for bit.

GPU half of ``tests/test_group_cases.py``: the grid of ``tests/_group_cases.py`` goes through
``pmml_group_rows``, ``pmml_ungroup`` and ``pmml_group_slice`` directly, over torch buffers that
carry guard words, and the order-free checkers of that module hold every result exactly — the
device tables (``row_start``, ``tile_start``, ``cursor``, ``counts``, ``ticket``) included. Every
launch stays inside the documented argument contract: buffers are exactly as long as the contract
says, plus guards. Then a fleet of integer-leaf GBDTs is scored through ``GroupedScorer.submit`` on
both routes and compared bit for bit with each model's own launch and with the float64 oracle."""

import functools

import numpy as np
import pytest
import torch

from tests import _boundary as B
from tests import _group_cases as GC

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _lib():
    from flink_jpmml_amd.ops import _lib

    return _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(buf: np.ndarray, gpu):
    """A guarded host buffer as a device tensor (uint32 words travel as int32)."""
    return torch.from_numpy(np.ascontiguousarray(buf.view(np.int32) if buf.dtype == np.uint32 else buf)).to(gpu)


def _ptr(t, off: int = 0) -> int:
    """Address of the buffer's body: behind the guard and ``off`` more elements."""
    assert t.data_ptr() % 16 == 0
    return t.data_ptr() + (GC.GUARD + off) * t.element_size()


def _host(t, dtype) -> np.ndarray:
    return t.cpu().numpy().view(dtype)


def _filled(values: np.ndarray, dtype, gpu, off: int = 0):
    buf = GC.guarded(len(values), dtype, off)
    GC.body(buf, len(values), off)[:] = values
    return _dev(buf, gpu)


def _inputs(cs, gpu):
    """``(X tensor, X pointer, Xg tensor, Xg pointer, codes tensor)``; asserts from the pointers which
    copy path the kernels will take."""
    s = cs.spec
    X = _filled(cs.X.reshape(-1), np.uint32, gpu, s.x_off)
    Xg = _dev(GC.guarded(s.n * s.F, np.uint32, s.xg_off), gpu)
    xp, gp = _ptr(X, s.x_off), _ptr(Xg, s.xg_off)
    assert xp % 16 == 4 * s.x_off and gp % 16 == 4 * s.xg_off
    vec4 = s.F % 4 == 0 and s.ldx % 4 == 0 and (xp | gp) % 16 == 0
    assert vec4 == s.vec4, s.name
    return X, xp, Xg, gp, torch.from_numpy(np.array(cs.codes)).to(gpu)


def _tables(K: int, n_entries: int, gpu) -> dict:
    """counts / ticket zeroed once (the kernel leaves them zero); the other tables hold the guard."""
    i32 = np.int32
    return dict(counts=_filled(np.zeros(K, i32), i32, gpu), ticket=_filled(np.zeros(1, i32), i32, gpu),
                cursor=_dev(GC.guarded(K, i32), gpu), row_start=_dev(GC.guarded(K + 1, i32), gpu),
                tile_start=_dev(GC.guarded(n_entries + 1, i32), gpu))


def _slice(cs, gpu, tab: dict, models=None) -> dict:
    """One ``pmml_group_slice`` over ``cs`` on the tables ``tab``; the buffers as numpy, for the checker."""
    s = cs.spec
    X, xp, Xg, gp, codes = _inputs(cs, gpu)
    tile_rows, order = models if models is not None else (
        torch.from_numpy(np.array(cs.tile_rows)).to(gpu),
        torch.from_numpy(np.array(cs.order) if cs.n_entries else np.zeros(1, np.int32)).to(gpu))
    perm = _dev(GC.guarded(s.n, np.int32), gpu)
    out_s = _dev(GC.guarded(s.n, np.uint32), gpu)
    out_v = _dev(GC.guarded(s.n, np.uint8), gpu)
    rc = _lib().pmml_group_slice(_stream(), xp, s.ldx, s.F, s.n, codes.data_ptr(), s.code_bytes, s.K,
                                 tile_rows.data_ptr(), order.data_ptr(), cs.n_entries, _ptr(tab["counts"]),
                                 _ptr(tab["ticket"]), _ptr(tab["cursor"]), _ptr(tab["row_start"]),
                                 _ptr(tab["tile_start"]), gp, _ptr(perm), _ptr(out_s), _ptr(out_v))
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert np.array_equal(_host(X, np.uint32), _dev_image(cs)), "the input rows were written"
    out = {k: _host(t, np.int32) for k, t in tab.items()}
    out.update(Xg=_host(Xg, np.uint32), perm=_host(perm, np.int32), out_s=_host(out_s, np.uint32),
               out_v=_host(out_v, np.uint8))
    return out


def _dev_image(cs) -> np.ndarray:
    s = cs.spec
    buf = GC.guarded(s.n * s.ldx, np.uint32, s.x_off)
    GC.body(buf, s.n * s.ldx, s.x_off)[:] = cs.X.reshape(-1)
    return buf


@pytest.mark.parametrize("name", GC.NAMES)
def test_group_rows_and_ungroup(gpu, name):
    """``pmml_group_rows`` on the host-counted cursor, then ``pmml_ungroup`` through the inverse
    permutation the device produced, with and without the second output pair."""
    cs = GC.case(name)
    s = cs.spec
    lib = _lib()
    X, xp, Xg, gp, codes = _inputs(cs, gpu)
    c = cs.codes.astype(np.int64)
    starts = np.concatenate([[0], np.cumsum(np.bincount(c[(c >= 0) & (c < s.K)], minlength=s.K))])
    cursor = _filled(starts[:s.K].astype(np.int32), np.int32, gpu)
    inv = _dev(GC.guarded(s.n, np.int32), gpu)
    rc = lib.pmml_group_rows(_stream(), xp, s.ldx, s.F, s.n, codes.data_ptr(), s.code_bytes, s.K, _ptr(cursor), gp,
                             _ptr(inv))
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert np.array_equal(_host(X, np.uint32), _dev_image(cs)), "the input rows were written"
    GC.check_group_rows(cs, dict(Xg=_host(Xg, np.uint32), inv=_host(inv, np.int32), cursor=_host(cursor, np.int32)))
    inv_h = GC.body(_host(inv, np.int32), s.n)
    sg, vg = _filled(cs.sg, np.uint32, gpu), _filled(cs.vg, np.uint8, gpu)
    for second in (True, False):
        o = [_dev(GC.guarded(s.n, dt), gpu) for dt in (np.uint32, np.uint8, np.uint32, np.uint8)]
        rc = lib.pmml_ungroup(_stream(), _ptr(sg), _ptr(vg), _ptr(inv), s.n, _ptr(o[0]), _ptr(o[1]),
                              _ptr(o[2]) if second else None, _ptr(o[3]) if second else None)
        assert rc == 0, rc
        torch.cuda.synchronize()
        out = dict(out_s=_host(o[0], np.uint32), out_v=_host(o[1], np.uint8))
        if second:
            out.update(out_s2=_host(o[2], np.uint32), out_v2=_host(o[3], np.uint8))
        else:  # a null second pair: nothing but the first pair is written
            assert (_host(o[2], np.uint32) == GC.GUARD32).all() and (_host(o[3], np.uint8) == GC.GUARD8).all()
        GC.check_ungroup(cs, inv_h, out)
    assert np.array_equal(GC.body(_host(sg, np.uint32), s.n), cs.sg)  # ungroup only reads its inputs
    assert np.array_equal(GC.body(_host(inv, np.int32), s.n), inv_h)


@pytest.mark.parametrize("name", GC.NAMES)
def test_group_slice(gpu, name):
    """``pmml_group_slice`` (count + place) on fresh tables: rows, permutation, answers of rows
    without a model, and every device table exactly."""
    cs = GC.case(name)
    GC.check_group_slice(cs, _slice(cs, gpu, _tables(cs.spec.K, cs.n_entries, gpu)))


def test_slices_back_to_back_reuse_counts_and_ticket(gpu):
    """Slice after slice on the SAME counts / ticket / cursor / row_start / tile_start tensors, with
    other codes and another row count each time (four, two, two and one counting workgroups; the
    third slice has no valid row at all): each result is right on its own, so nothing stale of the
    slice before is read."""
    seq = [GC.case(n) for n in GC.SEQUENCE]
    K, ne = seq[0].spec.K, seq[0].n_entries
    tab = _tables(K, ne, gpu)
    models = (torch.from_numpy(np.array(seq[0].tile_rows)).to(gpu), torch.from_numpy(np.array(seq[0].order)).to(gpu))
    for cs in seq + seq[::-1]:
        assert np.array_equal(cs.tile_rows, seq[0].tile_rows) and np.array_equal(cs.order, seq[0].order)
        GC.check_group_slice(cs, _slice(cs, gpu, tab, models))


def test_refusals_return_before_any_launch(gpu):
    """Arguments outside the kernels' limits are refused with the documented code, and neither a
    refusal nor ``n = 0`` writes a word (every pointer is a real buffer of the valid case's size)."""
    cs = GC.case("f4-p4")
    s = cs.spec
    lib = _lib()
    X, xp, Xg, gp, codes = _inputs(cs, gpu)
    tab = _tables(s.K, cs.n_entries, gpu)
    tile_rows = torch.from_numpy(np.array(cs.tile_rows)).to(gpu)
    order = torch.from_numpy(np.array(cs.order)).to(gpu)
    bufs = [_dev(GC.guarded(s.n, dt), gpu) for dt in (np.int32, np.uint32, np.uint8)]
    perm, out_s, out_v = bufs
    cursor = _dev(GC.guarded(s.K, np.int32), gpu)

    def rows(n=s.n, K=s.K, F=s.F, ldx=s.ldx, cb=s.code_bytes):
        return lib.pmml_group_rows(_stream(), xp, ldx, F, n, codes.data_ptr(), cb, K, _ptr(cursor), gp, _ptr(perm))

    def sliced(n=s.n, K=s.K, F=s.F, ldx=s.ldx, cb=s.code_bytes, ne=cs.n_entries):
        return lib.pmml_group_slice(_stream(), xp, ldx, F, n, codes.data_ptr(), cb, K, tile_rows.data_ptr(),
                                    order.data_ptr(), ne, _ptr(tab["counts"]), _ptr(tab["ticket"]),
                                    _ptr(tab["cursor"]), _ptr(tab["row_start"]), _ptr(tab["tile_start"]), gp,
                                    _ptr(perm), _ptr(out_s), _ptr(out_v))

    for fn in (rows, sliced):
        assert fn(K=0) == -2 and fn(K=GC.GROUP_MAXK + 1) == -2 and fn(F=0) == -2 and fn(ldx=s.F - 1) == -2
        assert fn(cb=3) == -3
        assert fn(n=0) == 0
    assert sliced(ne=s.K + 1) == -2 and sliced(ne=-1) == -2
    assert lib.pmml_ungroup(_stream(), _ptr(out_s), _ptr(out_v), _ptr(perm), 0, _ptr(out_s), _ptr(out_v), None,
                            None) == 0
    torch.cuda.synchronize()
    for t in [Xg, cursor, tab["cursor"], tab["row_start"], tab["tile_start"]] + bufs:
        h = t.cpu().numpy()
        assert (h == (GC.GUARD8 if h.dtype == np.uint8 else GC.G32I)).all()
    assert (GC.body(_host(tab["counts"], np.int32), s.K) == 0).all()
    assert GC.body(_host(tab["ticket"], np.int32), 1)[0] == 0
    # and the same buffers still serve a valid call
    GC.check_group_slice(cs, _slice(cs, gpu, tab))


# --------------------------------------------------------------------------- the grouped tree launch


@functools.lru_cache(maxsize=None)
def _fleet_reference():
    """Per tree model: (compiled, rows of the batch, oracle scores, oracle validity) — computed once."""
    from flink_jpmml_amd.runtime.compiled import CompiledPmml

    X, codes = GC.fleet_inputs(), GC.fleet_codes()
    ref = {}
    for k, txt in enumerate(GC.fleet_documents()):
        if txt is None:
            continue
        c = CompiledPmml.from_string(txt)
        rows = np.flatnonzero(codes == k)
        s, v = c.score_matrix_oracle(X[rows])
        B.assert_fp32_exact(s, v)
        assert v.any()
        ref[k] = (c, rows, s, v)
    assert not ref[1][3].all()  # the model with field preparation rejects some rows
    return ref


def test_grouped_tree_launch_bit_for_bit(gpu):
    """Five slices of a 5000-row batch through ``GroupedScorer.submit``, device-counted (count +
    place + ONE grouped wide launch per depth) and host-counted (group_rows + ``pmml_tree_launch_many``
    + ungroup), fed from pinned host memory and from a device tensor with a row stride above F:
    every row equals its own model's launch and the float64 oracle as fp32 bits, validity identical;
    rows of the two codes without a model are invalid with a NaN score."""
    from flink_jpmml_amd.api.batch import RecordBatch
    from flink_jpmml_amd.runtime import plans as PL
    from flink_jpmml_amd.runtime.engine import DevicePipeline, NullScorer, StreamingScorer
    from flink_jpmml_amd.runtime.grouped import GroupedScorer
    from flink_jpmml_amd.utils.metrics import METRICS

    F, n = GC.FLEET_F, GC.FLEET_ROWS
    X, codes, ref = GC.fleet_inputs(), GC.fleet_codes(), _fleet_reference()
    pipe = DevicePipeline(gpu, micro_batch=GC.FLEET_SLICE, h2d_streams=1)
    scorers, own = [], {}
    for k in range(len(GC.FLEET)):
        if k not in ref:
            scorers.append(NullScorer(F))
            continue
        plan = PL.TreePlan(ref[k][0], gpu, layout="perfect", variant="wide")
        assert plan.grouped_args(F) is not None and plan.rows_wide == 256, k
        assert (getattr(plan, "prep", None) is not None) == GC.FLEET[k][3]
        scorers.append(StreamingScorer(plan, pipeline=pipe))
        s, v = plan.score(np.array(X[ref[k][1]]))
        torch.cuda.synchronize()
        own[k] = (s.cpu().numpy(), v.cpu().numpy().astype(bool))
    for depth, group in zip((4, 6), GC.FLEET_GROUPS):
        assert {scorers[k].plan.depth for k in group} == {depth}
    # the slices hold what they are meant to hold
    per = [np.bincount(codes[s:s + GC.FLEET_SLICE], minlength=len(GC.FLEET)) for s in range(0, n, GC.FLEET_SLICE)]
    assert len(per) == 5 and (per[0][[0, 7]] == 0).all() and (per[1][[3, 5]] == 0).all() and (per[3][[1, 6]] == 0).all()
    assert per[0][[1, 2, 3]].tolist() == [256, 257, 1] and per[1][[6, 7, 0]].tolist() == [256, 257, 1]
    Xp = torch.from_numpy(np.array(X)).pin_memory()
    wide = torch.full((n, F + 3), float("nan"), dtype=torch.float32, device=gpu)
    wide[:, :F] = torch.from_numpy(np.array(X)).to(gpu)
    Xd = wide[:, :F]
    assert Xd.stride(0) == F + 3
    codes_d = torch.from_numpy(np.array(codes)).to(gpu)
    for device_grouping in (True, False):
        gs = GroupedScorer(pipe, rows_per_model=1, max_slice=GC.FLEET_SLICE)
        gs.device_grouping = device_grouping
        assert gs.slice_rows(len(scorers)) == GC.FLEET_SLICE
        for what, batch, cd in (("pinned", RecordBatch(Xp), np.array(codes)), ("device", RecordBatch(Xd), codes_d)):
            before = {k: METRICS.counters.get(k, 0) for k in ("grouped.slices", "grouped.device_counted_batches",
                                                              "grouped.tree_launches")}
            pb = gs.submit(batch, cd, scorers)
            pb.wait()
            torch.cuda.synchronize()
            after = {k: METRICS.counters.get(k, 0) - v for k, v in before.items()}
            assert after["grouped.slices"] == 5
            assert after["grouped.device_counted_batches"] == int(device_grouping)
            assert after["grouped.tree_launches"] == (10 if device_grouping else 0)  # two depths: two launches a slice
            sc, va = np.asarray(pb.scores, dtype=np.float32), np.asarray(pb.valid).astype(bool)
            tag = f"{'device' if device_grouping else 'host'}-counted, {what} rows"
            for k, (_, rows, s64, v64) in ref.items():
                assert np.array_equal(va[rows], v64), f"{tag}: model {k}: validity differs from the oracle"
                assert np.array_equal(va[rows], own[k][1]), f"{tag}: model {k}: validity differs from its own launch"
                got = sc[rows][v64].view(np.uint32)
                bad = np.flatnonzero(got != s64[v64].astype(np.float32).view(np.uint32))
                assert len(bad) == 0, (f"{tag}: model {k}: {len(bad)} rows differ from the oracle, first batch row "
                                       f"{rows[v64][bad[0]]}")
                assert np.array_equal(got, own[k][0][v64].view(np.uint32)), f"{tag}: model {k}: not its own launch"
            none = np.isin(codes, [k for k in range(len(GC.FLEET)) if k not in ref])
            assert none.sum() > 500 and not va[none].any() and np.isnan(sc[none]).all(), tag
        gs.drain()
