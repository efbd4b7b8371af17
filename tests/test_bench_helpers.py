"""Host-side helpers of bench.py: the sysfs shader-clock reader and the
per-step PMC traffic lookup keyed by the kernel sources."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_clock_sampler_reads_current_level(tmp_path):
    import bench
    f = tmp_path / "pp_dpm_sclk"
    f.write_text("0: 500Mhz\n1: 1600Mhz\n2: 2400Mhz *\n")
    cs = bench.ClockSampler.__new__(bench.ClockSampler)
    cs.path, cs.mhz, cs._stop = str(f), [], None
    assert cs._read() == 2400
    cs.mhz = [2390, 2400, 2380]
    s = cs.summary()
    assert (s["sclk_mhz_min"], s["sclk_mhz_median"], s["sclk_mhz_max"], s["samples"]) == (2380, 2390, 2400, 3)
    cs.mhz = []
    assert cs.summary()["sclk_mhz_median"] is None


def test_plain_run_is_lean_and_full_adds_the_cpu_checks(monkeypatch):
    """The CPU baseline and the parity check run only behind --full."""
    import bench
    for argv, want in (([], False), (["--full"], True), (["--full", "--no-cpu-baseline"], False),
                       (["--no-cpu-baseline"], False)):
        monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"] + argv)
        a = bench.parse()
        assert (a.steps, a.warmup, a.cpu_checks, a.dump_outputs) == (3, 1, want, None)


def test_dump_outputs_formats_and_fixed_sample(tmp_path, monkeypatch):
    """--dump-outputs: float32 / float64 files; an array above its share is a
    seeded row sample (the same rows every run) plus its full column sums."""
    import numpy as np
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 2 * 4096)
    rng = np.random.default_rng(1)
    img = rng.random((50, 64), dtype=np.float32)             # 12 800 B > the 4 096 B share
    counts = np.array([7, 2 ** 40 + 1], np.int64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"result": img, "rejected": counts})
    a = {f: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    b = {f: np.load(tmp_path / "b" / f) for f in sorted(os.listdir(tmp_path / "b"))}
    assert sorted(a) == ["rejected.npy", "result.npy", "result_colsum.npy", "result_rows.npy"]
    assert all(np.array_equal(a[f], b[f]) for f in a)
    assert a["rejected.npy"].dtype == np.float64 and a["rejected.npy"].tolist() == [7.0, float(2 ** 40 + 1)]
    rows = a["result_rows.npy"].astype(int)
    assert a["result.npy"].dtype == np.float32 and 1 <= len(rows) < 50 and np.all(np.diff(rows) > 0)
    assert np.array_equal(a["result.npy"], img[rows])
    assert np.array_equal(a["result_colsum.npy"], img.sum(axis=0, dtype=np.float64))
    assert sum(v.nbytes for v in a.values()) <= 2 * 4096
    # below its share an array is written whole
    bench.dump_outputs(str(tmp_path / "c"), {"result": img[:8]})
    assert os.listdir(tmp_path / "c") == ["result.npy"]
    assert np.array_equal(np.load(tmp_path / "c" / "result.npy"), img[:8])


def test_traffic_records_match_sources():
    """Every committed per-step traffic record names its profile file, and a
    record is only used while the kernel sources hash the same."""
    import bench
    recs = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic_aux.json")))
    for cfg, r in recs.items():
        assert r["bytes_per_step_scope"] > 0
        assert os.path.exists(os.path.join(ROOT, r["source"].split(" ")[0])), r["source"]
        t, _ = bench.aux_traffic(cfg)
        assert t == (r["bytes_per_step_scope"] if r["source_hash"] == bench.aux_source_hash(cfg) else None)
