"""bench.py's own contract: `--dump-outputs DIR` writes the last timed step's result arrays in float64 without losing a bit, the same
files for the same arguments; `--steps` is the number of timed steps and the line carries `ms_per_step`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_exact_float64_keeps_every_bit_of_64_bit_words():
    rng = np.random.default_rng(3)
    masks = rng.integers(0, 2 ** 63, (7, 5), dtype=np.uint64) | np.uint64(1 << 63)
    f = bench.exact_float64(masks)
    assert f.dtype == np.float64 and f.shape == (7, 5, 2)
    assert (f.astype(np.uint32).reshape(7, 10).view(np.uint64) == masks).all()
    small = np.array([-1, 0, 7, 2 ** 31 - 1], dtype=np.int32)
    assert (bench.exact_float64(small) == small).all()


def test_unscheduled_pods_are_given_per_pod_and_nothing_empty_is_written(tmp_path):
    """The unscheduled list becomes a per-pod array (place in the list, -1 when scheduled): its shape is the pod count whatever the result."""
    P, N = 6, 2
    arrays = {"n_existing": 0, "n_new": N, "pod_node": np.array([0, -1, 1, 0, -1, 1], np.int32), "pod_stage": np.zeros(P, np.int32), "pod_reason": np.zeros(P, np.uint32),
              "unscheduled": np.array([4, 1], np.int32), "node_pods_off": np.array([0, 2, 4], np.uint32), "node_pods": np.array([0, 3, 2, 5], np.int32),
              "node_tmpl": np.zeros(N, np.int32), "node_types": np.ones((N, 2), np.uint64), "node_requests": np.ones((N, 3), np.int64),
              "node_requests_present": np.ones(N, np.uint32), "node_present": np.ones(N, np.uint32), "node_complement": np.zeros(N, np.uint32),
              "node_mask": np.ones((N, 4), np.uint64)}
    outs = bench.result_outputs(arrays)
    assert "unscheduled" not in outs and outs["pod_unscheduled_order"].tolist() == [-1, 1, -1, -1, 0, -1] and outs["counts"].tolist() == [0, N, 2]
    none = bench.result_outputs(dict(arrays, unscheduled=np.zeros(0, np.int32), n_new=0, node_tmpl=np.zeros(0, np.int32), node_types=np.zeros((0, 2), np.uint64)))
    assert none["pod_unscheduled_order"].tolist() == [-1] * P
    bench.dump_outputs(str(tmp_path), none)
    assert "node_types.npy" not in os.listdir(tmp_path) and all(np.load(tmp_path / f).size for f in os.listdir(tmp_path))


def test_dump_is_bounded_and_its_sample_fixed(tmp_path, monkeypatch):
    outs = {"pod_node": np.arange(5000, dtype=np.float64), "node_types": np.ones((800, 64, 2))}
    bench.dump_outputs(str(tmp_path / "all"), outs)
    assert (np.load(tmp_path / "all" / "pod_node.npy") == outs["pod_node"]).all()
    assert not (tmp_path / "all" / "pod_node.rows.npy").exists()
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 100_000)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), outs)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(os.listdir(tmp_path / "b"))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 100_000 + 256 * len(files)      # (+ the .npy headers)
    for f in files:
        assert (np.load(tmp_path / "a" / f) == np.load(tmp_path / "b" / f)).all()
    rows = np.load(tmp_path / "a" / "pod_node.rows.npy")
    assert (np.load(tmp_path / "a" / "pod_node.npy") == outs["pod_node"][rows.astype(np.int64)]).all()


@pytest.mark.gpu
def test_plain_run_dumps_what_the_timed_path_computed(tmp_path):
    """A plain run at a small size: three timed steps, and the dumped arrays are the result of solve_from_pods on the same seeded problem."""
    from karpenter_core_amd import scheduler as S, workloads as W
    d = tmp_path / "out"
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None); env.pop("RANK", None); env.pop("LOCAL_RANK", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--pods", "3000", "--sizes", "5",
                        "--dump-outputs", str(d)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0
    assert "cpu_baseline" not in line and "whatif_batch" not in line          # (--full only)
    fp, _ = S.solve_from_pods(S.ParsedProblem(W.config3(pods=3000, sizes=5, seed=44)), 0)
    want = bench.result_outputs(fp.result_arrays())
    fp.close()
    want = {name: a for name, a in want.items() if a.size}
    assert sorted(f[:-4] for f in os.listdir(d)) == sorted(want)
    for name, a in want.items():
        got = np.load(d / f"{name}.npy")
        assert got.dtype == np.float64 and got.shape == a.shape and (got == a).all(), name
    assert line["config"]["new_nodes"] == int(want["counts"][1]) and line["config"]["unschedulable"] == int(want["counts"][2])
