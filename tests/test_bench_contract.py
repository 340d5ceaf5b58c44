"""The bench line contract, checked on the committed round profile (profiles/r*_bench_collab.json is the
stdout of `python bench.py --full` on an MI355X): every key its readers use, with sane values."""
import glob
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_committed_bench_line_has_the_contract_keys():
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_bench_collab.json")))
    assert files, "no committed bench line"
    d = json.loads(open(files[-1]).read().strip().splitlines()[-1])
    base = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["metric"].startswith(base["metric"].split(",")[0]) and d["unit"] == "edges/s"
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None
    assert d["n_gpus"] == 1 and d["data"] == "synthetic" and d["dtype"] == "f32"
    assert "workload" in d["config"] and "model" not in d["config"]
    assert abs(d["value"] - d["config"]["global_batch"] / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-6
    r = d["roofline"]
    assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s")
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9 and r["frac"] > 0 and "traffic" in r
    assert r["frac"] <= 1.0                                     # hbm: bytes against 8 TB/s; mfma: the 16-bit MFMA FLOPs the launch issues against the dense 16-bit peak
    if r["bound"] == "mfma":
        assert r["peak"] == 2500.0 and r["mfma_per_f32_product"] == 3 and 0 < r["f32_equivalent_frac_of_f32_mfma_peak"] < 1.0
    assert r["avg_launch_ms"] > 0 and r["launches_per_step"] >= 1
    for rr in d.get("rooflines", {}).values():                  # every per-kernel object: an achieved rate never above its peak
        assert 0 < rr["frac"] <= 1.0 and (rr.get("traffic_frac") is None or rr["traffic_frac"] <= 1.0)
    c = d["cpu_baseline"]
    assert c["kind"] in ("port", "reference") and c["unit"] == "edges/s" and c["cores"] >= 1 and c["value"] > 0 and c["sample"]
    if "full" in c["sample"]:                                   # the CPU leg ran the step's whole candidate batch
        assert d["value"] / c["value"] > 10                     # north_star: >= 10x the CPU path at one MI355X
    assert d["parity_on_cpu_sample_max_abs_err"] < 1e-5


def test_profiles_hold_the_rocprof_summaries():
    names = {os.path.basename(f) for f in glob.glob(os.path.join(ROOT, "profiles", "*"))}
    assert any(n.endswith("_bench_kernel_stats.csv") for n in names) and any(n.endswith("_pmc.json") for n in names)
    stats = open(sorted(glob.glob(os.path.join(ROOT, "profiles", "*_bench_kernel_stats.csv")))[-1]).read()
    for kernel in ("heads_fused_kernel", "cn_gather_kernel", "cn_flags_kernel"):
        assert kernel in stats


def test_dump_outputs_writes_float32_scores_and_a_fixed_sample_above_the_cap(tmp_path, monkeypatch):
    """--dump-outputs: the scores as float32; above the byte cap, a seeded sample of rows (the same one every run) with
    their row ids beside them, both files together within the cap."""
    import sys
    import numpy as np
    import torch
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    s = torch.randn(1000, 1, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    bench.dump_outputs(str(tmp_path / "whole"), s)
    got = np.load(tmp_path / "whole" / "scores.npy")
    assert got.dtype == np.float32 and np.array_equal(got, s.float().numpy())
    assert not (tmp_path / "whole" / "scores_rows.npy").exists()
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 1200)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), s)
    rows, got = np.load(tmp_path / "a" / "scores_rows.npy"), np.load(tmp_path / "a" / "scores.npy")
    assert rows.dtype == np.float64 and got.dtype == np.float32 and rows.nbytes + got.nbytes <= 1200 and len(rows) == 100
    assert np.all(np.diff(rows) > 0) and np.array_equal(got, s.float().numpy()[rows.astype(np.int64)])
    assert np.array_equal(rows, np.load(tmp_path / "b" / "scores_rows.npy"))


def test_full_and_dump_outputs_are_options():
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs DIR" in r.stdout
