"""The driver's N-rank ``bench.py`` launch, rehearsed on the CPU.

``python -m torch.distributed.run --nproc-per-node N ... bench.py --rehearse-cpu --full`` runs the exact
DSL job, GatherSink (lockstep all-gather, host path over gloo) and collective code of the timed
region with the host oracle scorer; every rank then checks every rank's gathered rows against
that rank's oracle scores. The committed 8-rank run is ``profiles/r4_rehearsal/``.

Round 5: the check is per rank, over every gathered element, with the row
order taken from the source offsets — so it covers every bench mode: ``--models N`` (mixed-model
rows, each against its own model's oracle), ``--source binary`` (memory-mapped record files,
micro-batch elements) and ``--source text`` (CSV through the native parser), at world 8
(``profiles/r5_rehearsal/``)."""

import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rehearse(tmp_path, world, *extra):
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
           "--master-addr", "127.0.0.1", "--master-port", str(_port()), os.path.join(ROOT, "bench.py"), "--gpus",
           str(world), "--rehearse-cpu", "--rows", "512", "--passes", "2", "--steps", "1", "--warmup", "1",
           "--trees", "12", "--check-rows", "128", "--latency-iters", "2", "--ingest-threads", "1", "--full", *extra]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("mode", [("--models", "16"), ("--source", "binary", "--micro-batch", "200"),
                                  ("--source", "text", "--micro-batch", "200")])
def test_bench_eight_rank_rehearsal_every_mode(tmp_path, mode):
    out = _rehearse(tmp_path, 8, *mode)
    assert out["n_gpus"] == 8 and out["rehearsal_cpu"]
    assert out["job"]["rehearsal_gather_check"] == [True] * 8
    assert out["job"]["rehearsal_rows_checked_per_rank"] == [512 * 2 * 2] * 8  # rows x passes x steps
    assert out["job"]["rehearsal_rows_gathered_per_rank"] == 8 * 512 * 2 * 2


def test_rehearsal_check_catches_misplaced_rows():
    """The per-rank check fails when two ranks' chunks are swapped inside a gathered element."""
    from types import SimpleNamespace

    import numpy as np

    sys.path.insert(0, ROOT)
    import bench

    args = SimpleNamespace(rows=64, features=4, source="synthetic", models=1, warmup=0, steps=1, passes=1)
    from flink_jpmml_amd.bench import synth

    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_reh_model.pmml")
    with open(path, "w") as fh:
        fh.write(synth.gbdt_pmml(n_trees=5, depth=3, n_features=4, seed=3))
    try:
        parts = []
        for r in range(2):
            s, v = bench._rehearsal_reference(args, r, [path])
            parts.append((s.astype(np.float32), v, np.arange(64)))
        good = tuple(np.concatenate([p[i] for p in parts]) for i in range(3))
        swapped = tuple(np.concatenate([p[i] for p in parts[::-1]]) for i in range(3))
        for me in range(2):
            ctx = SimpleNamespace(world_size=2, rank=me)
            assert bench._rehearsal_check(args, SimpleNamespace(_parts=[good]), ctx, [path])[0]
            assert not bench._rehearsal_check(args, SimpleNamespace(_parts=[swapped]), ctx, [path])[0]
    finally:
        os.unlink(path)


def test_bench_spawns_its_own_ranks_without_a_launcher(tmp_path):
    """the driver's bare ``bench.py --gpus N`` (no torchrun, no WORLD_SIZE) must
    run N ranks — the parent spawns them and relays rank 0's JSON line."""
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR", "FJA_BENCH_CHILD"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--rehearse-cpu", "--rows", "512",
           "--passes", "2", "--steps", "1", "--warmup", "1", "--trees", "12", "--check-rows", "128",
           "--latency-iters", "2", "--full"]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.lstrip().startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]  # exactly one JSON line: rank 0's
    out = json.loads(lines[0])
    assert out["n_gpus"] == 4 and out["config"]["parallelism"] == "dp4"
    assert out["job"]["rehearsal_gather_check"] == [True] * 4


def test_bench_launcher_fails_when_a_rank_fails(tmp_path):
    """A rank that dies makes the launcher exit non-zero (the siblings are torn down)."""
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR", "FJA_BENCH_CHILD"):
        env.pop(k, None)
    # --models with a file source is refused inside every rank (SystemExit) after the group formed
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--rehearse-cpu", "--rows", "256",
           "--passes", "1", "--steps", "1", "--warmup", "1", "--trees", "4", "--check-rows", "0",
           "--models", "2", "--source", "binary"]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0
    assert not any(ln.lstrip().startswith("{") for ln in r.stdout.splitlines())


def test_bench_two_rank_cpu_rehearsal(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2",
           "--rehearse-cpu", "--rows", "1024", "--passes", "2", "--steps", "2", "--warmup", "1", "--trees", "20",
           "--check-rows", "256", "--latency-iters", "2", "--full"]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["n_gpus"] == 2 and out["rehearsal_cpu"] and out["metric"].startswith("[CPU REHEARSAL")
    assert out["job"]["rehearsal_gather_check"] == [True, True]
    assert out["job"]["rehearsal_rows_gathered_per_rank"] == 2 * 1024 * 2 * 3  # ranks x rows x passes x steps
    assert out["check"]["valid_match"]


def _plain_run(tmp_path, out_dir, *extra, gpus=1):
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR", "FJA_BENCH_CHILD"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--rehearse-cpu", "--rows", "700",
           "--passes", "3", "--steps", "2", "--warmup", "1", "--trees", "12", "--dump-outputs", str(out_dir), *extra]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_plain_run_is_lean_and_dumps_the_last_step(tmp_path):
    """A run without ``--full`` only times its steps (no oracle check, latency loop or kernel-only
    figures); ``--dump-outputs`` writes the last timed step's results, the same from run to run,
    and they are what the fp64 oracle scores for the rows at the recorded source offsets."""
    import numpy as np

    sys.path.insert(0, ROOT)
    import bench
    from flink_jpmml_amd.bench import synth
    from flink_jpmml_amd.runtime.compiled import CompiledPmml

    out = _plain_run(tmp_path, tmp_path / "a")
    assert out["steps"] == 2 and out["ms_per_step"] > 0 and not out["full"]
    assert out["value"] == pytest.approx(700 * 3 / (out["ms_per_step"] / 1e3))
    assert out["check"] == {} and out["p50_latency_ms"] is None and out["kernel_ms_per_1M_rows"] is None
    assert "rehearsal_gather_check" not in out["job"]
    _plain_run(tmp_path, tmp_path / "b")
    a = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in ("scores", "valid", "row_offsets")}
    assert sorted(os.listdir(tmp_path / "a")) == ["row_offsets.npy", "scores.npy", "valid.npy"]
    for n, dt in (("scores", np.float32), ("valid", np.float32), ("row_offsets", np.float64)):
        assert a[n].dtype == dt and a[n].shape == (700 * 3,)
        assert np.array_equal(a[n], np.load(tmp_path / "b" / f"{n}.npy"), equal_nan=True)
    # the last of the 1 + 2 steps: source offsets [2 * 2100, 3 * 2100), every row of it once
    assert a["row_offsets"].tolist() == list(range(2 * 2100, 3 * 2100))
    args = bench.parse_args(["--rows", "700", "--trees", "12"])
    ref, valid = CompiledPmml.from_string(bench.model_text(args)).score_matrix_oracle(
        synth.stream_matrix(700, args.features, seed=1000))
    rows = a["row_offsets"].astype(np.int64) % 700
    assert np.array_equal(a["valid"] != 0, valid[rows])
    assert np.array_equal(a["scores"], ref[rows].astype(np.float32))


def test_two_rank_run_dumps_every_ranks_rows(tmp_path):
    """``--dump-outputs`` at N = 2 (gloo): every rank samples, so both sinks run the same collectives,
    and rank 0 writes both ranks' rows of the last step, rank-major inside every gathered element."""
    import numpy as np

    sys.path.insert(0, ROOT)
    import bench
    from flink_jpmml_amd.bench import synth
    from flink_jpmml_amd.runtime.compiled import CompiledPmml

    out = _plain_run(tmp_path, tmp_path / "d", gpus=2)
    assert out["n_gpus"] == 2 and out["config"]["allgather_sink"] and not out["full"]
    a = {n: np.load(tmp_path / "d" / f"{n}.npy") for n in ("scores", "valid", "row_offsets")}
    assert all(x.shape == (2 * 3 * 700,) for x in a.values())
    args = bench.parse_args(["--rows", "700", "--trees", "12"])
    model = CompiledPmml.from_string(bench.model_text(args))
    ref = [model.score_matrix_oracle(synth.stream_matrix(700, args.features, seed=1000 + r)) for r in range(2)]
    for e in range(3):  # one gathered element per pass of the last step
        for r in range(2):
            part = slice((2 * e + r) * 700, (2 * e + r + 1) * 700)
            assert a["row_offsets"][part].tolist() == list(range((6 + e) * 700, (7 + e) * 700))
            assert np.array_equal(a["valid"][part] != 0, ref[r][1])
            assert np.array_equal(a["scores"][part], ref[r][0].astype(np.float32))


def test_output_sampler_is_seeded_and_bounded(monkeypatch):
    """Above the row budget the dump is a fixed, seeded, duplicate-free sample of the last step."""
    import numpy as np

    sys.path.insert(0, ROOT)
    import bench

    monkeypatch.setattr(bench, "DUMP_ROWS", 64)
    args = bench.parse_args(["--rows", "500", "--passes", "3", "--steps", "2", "--warmup", "1"])
    for world in (1, 2):
        got = []
        for _ in range(2):
            sm = bench._OutputSampler(args, world)
            for elem in range(3 * 3):  # (warmup + steps) x passes elements, `world` ranks' rows in each
                o = np.concatenate([elem * 500 + np.arange(500)] * world)
                s = np.concatenate([o[:500] + 0.25 * r for r in range(world)])
                sm.take(s, np.ones(len(s), dtype=bool), o)
            got.append([np.concatenate([p[i] for p in sm.parts]) for i in range(3)])
        s, v, o = got[0]
        assert all(np.array_equal(x, y) for x, y in zip(got[0], got[1]))
        assert len(s) == 64 and s.dtype == np.float32 and o.dtype == np.float64
        assert o.min() >= 2 * 1500 and o.max() < 3 * 1500  # last step only
        assert len({(x, y) for x, y in zip(o.tolist(), (s - o).tolist())}) == 64  # distinct (row, rank) pairs
        assert set((s - o).tolist()) == {0.25 * r for r in range(world)}
    # the engine path keeps only the last pass: same source offsets, restricted to that pass
    last = bench._OutputSampler(args, 1, last_pass_only=True)
    assert last.first == 2 * 1500 and len(last.pos) and last.pos.min() >= 1000 and last.pos.max() < 1500
    assert set(last.pos.tolist()) <= set(bench._OutputSampler(args, 1).pos.tolist())
    with pytest.raises(AssertionError):  # unequal rows per rank in a gathered element
        bench._OutputSampler(args, 2).take(np.zeros(501), np.ones(501, dtype=bool), 3000 + np.arange(501))
