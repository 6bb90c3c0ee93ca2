"""bench.py's plain run, --full and --dump-outputs.

CPU (-m "not gpu"): a plain command line switches off everything beside the headline
figure (config 5, the CPU baseline, the alternate partitions) and --full brings it
back; the cells --dump-outputs samples depend on the table size alone.
GPU (-m gpu): a plain run on a small odd-sized table prints the headline fields only,
runs exactly --steps timed steps and dumps the oracle's table cell for cell, the same
on a second run; --full adds config 5 and the CPU baseline to the same line.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, ROOT

sys.path.insert(0, ROOT)
sys.path.insert(0, PKG)
import bench  # noqa: E402
import nwhip  # noqa: E402
import oracle  # noqa: E402

N = 1537  # odd, no multiple of a 256-column strip, several strips and workgroups


def _parse(monkeypatch, argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return bench.parse()


def test_plain_run_measures_the_headline_only(monkeypatch):
    a = _parse(monkeypatch, ["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert a.no_config5 and a.no_cpu_baseline and a.alt_partition == "none"
    a = _parse(monkeypatch, ["--gpus", "2", "--alt-partition", "cols"])
    assert a.alt_partition == "cols" and a.no_cpu_baseline


def test_full_brings_the_rest_back(monkeypatch):
    a = _parse(monkeypatch, ["--gpus", "1", "--full"])
    assert a.full and not a.no_config5 and not a.no_cpu_baseline and a.alt_partition is None
    a = _parse(monkeypatch, ["--full", "--no-cpu-baseline", "--alt-partition", "none"])
    assert a.no_cpu_baseline and not a.no_config5 and a.alt_partition == "none"


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"]])
def test_step_counts_are_checked(monkeypatch, argv):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, argv)


@pytest.mark.parametrize("n1,n2", [(3, 2), (N, N), (262144, 262144)])
def test_dump_indices_fixed_and_in_range(n1, n2):
    rows, cell_rows, cell_cols = bench.dump_indices(n1, n2)
    again = bench.dump_indices(n1, n2)
    assert all(np.array_equal(x, y) for x, y in zip((rows, cell_rows, cell_cols), again))
    assert len(set(rows.tolist())) == rows.size == min(bench.DUMP_ROWS, n2 + 1)
    assert rows.min() >= 0 and rows.max() <= n2 and cell_rows.min() >= 0 and cell_rows.max() <= n2
    assert cell_cols.shape[0] == cell_rows.size and cell_cols.min() >= 0 and cell_cols.max() <= n1
    assert cell_cols.size <= bench.DUMP_CELLS
    # float64, everything --dump-outputs writes for this size: within the 64 MB bound
    assert 8 * (1 + (n1 + 1) + (n2 + 1) + rows.size * (n1 + 1) + cell_cols.size) <= 64 << 20


def _run_bench(args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["PYTHONPATH"] = PKG
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True,
                         text=True, timeout=300, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def torch_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def want_table():
    t = oracle.fill(nwhip.synth(1, N), nwhip.synth(2, N), (1, 0, -1))
    t.setflags(write=False)
    return t


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.mark.gpu
def test_plain_run_dumps_the_table(torch_gpu, want_table, tmp_path):
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    args = ["--gpus", "1", "--n", str(N), "--steps", "3", "--warmup", "1"]
    res = _run_bench(args + ["--dump-outputs", d1])
    assert res["steps"] == 3 and res["warmup"] == 1 and res["n_gpus"] == 1
    assert res["unit"] == "GCUPS" and res["higher_is_better"] is True and res["dtype"] == "int32"
    assert res["metric"].startswith("GCUPS") and res["value"] > 0 and res["ms_per_step"] > 0
    # value and ms_per_step say the same thing about the same 3 steps (value is rounded
    # to 0.01, ms_per_step to 0.001)
    rel = 0.005 / res["value"] + 0.0005 / res["ms_per_step"] + 1e-6
    assert res["value"] == pytest.approx(N * N / (res["ms_per_step"] * 1e6), rel=rel)
    assert "config5" not in res and "cpu_baseline" not in res
    assert res["score"] == int(want_table[N, N])
    got = _load(d1)
    assert sorted(got) == ["last_col", "last_row", "sample_cells", "sample_rows", "score"]
    assert all(a.dtype == np.float64 for a in got.values())
    rows, cell_rows, cell_cols = bench.dump_indices(N, N)
    np.testing.assert_array_equal(got["score"], [want_table[N, N]])
    np.testing.assert_array_equal(got["last_row"], want_table[N, :])
    np.testing.assert_array_equal(got["last_col"], want_table[:, N])
    np.testing.assert_array_equal(got["sample_rows"], want_table[rows, :])
    np.testing.assert_array_equal(got["sample_cells"], want_table[cell_rows[:, None], cell_cols])
    # the same arguments again: the same inputs, the same files
    _run_bench(args + ["--dump-outputs", d2])
    again = _load(d2)
    assert sorted(again) == sorted(got) and all(np.array_equal(got[k], again[k]) for k in got)


@pytest.mark.gpu
def test_sw_run_dumps_the_alignment(torch_gpu, tmp_path):
    """--workload sw: the table sample, and the alignment and edit script of the line."""
    d = str(tmp_path / "sw")
    res = _run_bench(["--workload", "sw", "--n", str(N), "--steps", "2", "--warmup", "1", "--dump-outputs", d])
    got = _load(d)
    assert sorted(got) == ["alignment", "last_col", "last_row", "ops", "sample_cells", "sample_rows", "score"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["alignment"].tolist() == [res["score"], *res["end"], *res["begin"], res["n_ops"]]
    s1, s2, scheme = nwhip.synth(1, N), nwhip.synth(2, N), (1, -1, -1)
    want = oracle.sw_fill(s1, s2, scheme)
    score, ei, ej = oracle.sw_best(s1, s2, scheme)
    ops, bi, bj = oracle.sw_traceback(s1, s2, want, (ei, ej), scheme)
    assert got["alignment"].tolist() == [score, ei, ej, bi, bj, ops.size]
    np.testing.assert_array_equal(got["ops"], ops)
    rows, cell_rows, cell_cols = bench.dump_indices(N, N)
    np.testing.assert_array_equal(got["score"], [want[N, N]])
    np.testing.assert_array_equal(got["last_row"], want[N, :])
    np.testing.assert_array_equal(got["last_col"], want[:, N])
    np.testing.assert_array_equal(got["sample_rows"], want[rows, :])
    np.testing.assert_array_equal(got["sample_cells"], want[cell_rows[:, None], cell_cols])


@pytest.mark.gpu
def test_full_run_adds_config5_and_cpu_baseline(torch_gpu, want_table):
    res = _run_bench(["--gpus", "1", "--n", str(N), "--steps", "1", "--warmup", "1", "--full",
                      "--cpu-n", "512"])
    assert res["steps"] == 1 and res["score"] == int(want_table[N, N])
    c5 = res["config5"]
    assert c5["workload"] == "sw_fill_traceback_65536x65536" and c5["result_ok"] is True
    assert c5["ms_per_step"] > 0
    cpu = res["cpu_baseline"]
    assert cpu["value"] > 0 and set(cpu["legs"]) == {"serial", "idxarray_mt_all", "idxarray_mt_8"}
    want = oracle.score(nwhip.synth(1, 512), nwhip.synth(2, 512))
    assert all(leg.get("score") == want for leg in cpu["legs"].values()), cpu["legs"]
