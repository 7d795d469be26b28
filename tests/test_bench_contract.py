"""bench.py: the pieces that can be checked without a GPU (the PMC-summary staleness guard) and, with -m gpu, the JSON line
the driver parses (one small run as a subprocess)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_pmc_summary_is_used_only_for_the_sources_it_was_measured_on(tmp_path, monkeypatch):
    b = _bench()
    digest = b.kernel_source_digest()
    assert len(digest) == 16 and digest == b.kernel_source_digest()
    prof = tmp_path / "profiles"
    prof.mkdir()
    monkeypatch.setattr(b, "ROOT", str(tmp_path))
    (tmp_path / "echoglad_amd").mkdir()
    os.symlink(os.path.join(ROOT, "echoglad_amd", "csrc"), tmp_path / "echoglad_amd" / "csrc")
    assert b.pmc_traffic("k_gcn_layer")[0] is None                     # no summary at all
    (prof / "r09_pmc.json").write_text(json.dumps({"kernel_source_digest": "0" * 16, "k_gcn_layer": {"hbm_bytes_per_launch": 1.0}}))
    traffic, why = b.pmc_traffic("k_gcn_layer")
    assert traffic is None and "stale" in why
    (prof / "r09_pmc.json").write_text(json.dumps({"kernel_source_digest": digest, "k_gcn_layer": {"hbm_bytes_per_launch": 7.5e8}}))
    assert b.pmc_traffic("k_gcn_layer") == (750000000, "profiles/r09_pmc.json")
    # other *_pmc.json files next to the real one (the training step's summary sorts AFTER r09_pmc.json; round 2's HEAD
    # picked it and reported traffic = null) are never candidates for the inference kernel's traffic
    (prof / "r09_train_pmc.json").write_text(json.dumps({"k_bn_act_fwd": {"hbm_bytes_per_launch": 3.5e9}}))
    (prof / "zz_pmc.json").write_text("{}")
    assert b.pmc_traffic("k_gcn_layer") == (750000000, "profiles/r09_pmc.json")
    # ... and the training summary has its own digest (over the training kernels' sources) and its own reader
    assert b.train_pmc_traffic()[0] is None and "stale" in b.train_pmc_traffic()[1]
    (prof / "r09_train_pmc.json").write_text(json.dumps({"kernel_source_digest": b.kernel_source_digest(b.TRAIN_KERNEL_SOURCES),
                                                         "hbm_bytes_per_step": 5.0e10}))
    assert b.train_pmc_traffic() == (50000000000, "profiles/r09_train_pmc.json")
    assert b.pmc_traffic("k_gcn_layer") == (750000000, "profiles/r09_pmc.json")


def test_committed_pmc_summary_matches_the_committed_kernel_sources():
    """profiles/r*_pmc.json of this round must have been measured on the dominant kernel's current sources."""
    b = _bench()
    traffic, src = b.pmc_traffic("k_gcn_layer")
    assert traffic is not None, src
    assert 5.9e8 <= traffic <= 1.2e9            # >= the algorithmic 590 MB per launch, and not absurdly above it


@pytest.mark.gpu
def test_bench_line_contract():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "5", "--warmup", "2", "--no-cpu-baseline",
                        "--no-other-configs", "--repeats", "2", "--spinup", "0.05"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "repeats", "distributed"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 5 and d["warmup"] == 2 and d["dtype"] == "f32" and d["scaling"] == "weak"
    assert d["vs_baseline"] is None and d["higher_is_better"] is True and "workload" in d["config"]
    assert abs(d["value"] - 8 / (d["ms_per_step"] * 1e-3)) < 1e-2 * d["value"]
    rf = d["roofline"]
    assert rf["bound"] in ("hbm", "mfma") and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3 and 0 < rf["frac"] < 1
    assert d["repeats"]["n"] == 2 and d["repeats"]["min"] <= d["repeats"]["max"]
    assert d["eager_ms_per_step"] > 0 and "replay" in d["config"]["launch"]
    assert len(lines[0]) <= 1600 and os.path.exists(os.path.join(ROOT, d["details"]))
    full = json.load(open(os.path.join(ROOT, d["details"])))
    assert full["value"] == d["value"] and "avg_launch_timing" in full["roofline"]


@pytest.mark.gpu
def test_plain_bench_line_times_k_steps_and_dumps_the_last_steps_logits(tmp_path):
    """Without --full the run is lean: the headline keys only (no side measurement), `steps` timed steps, and --dump-outputs
    writes the logits of the last timed step; the same arguments give the same inputs, so a second run writes the same bits."""
    import numpy as np
    got = []
    for k in range(2):
        out = tmp_path / f"run{k}"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                            "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1
        d = json.loads(lines[0])
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "config"):
            assert key in d, key
        for key in ("roofline", "repeats", "eager_ms_per_step", "cpu_baseline", "parity", "other_configs", "after_path"):
            assert key not in d, key
        assert d["steps"] == 7 and d["warmup"] == 2 and d["unit"] == "frames/s" and d["dtype"] == "f32"
        assert abs(d["value"] - 8 / (d["ms_per_step"] * 1e-3)) < 1e-2 * d["value"]
        assert sorted(os.listdir(out)) == ["logits.npy"]
        lg = np.load(out / "logits.npy")
        assert lg.dtype == np.float32 and lg.shape == (8 * d["config"]["nodes_per_frame"], 4) and np.isfinite(lg).all()
        got.append(lg)
    assert np.array_equal(got[0], got[1])


def _counting_clock(monkeypatch, b):
    """bench's clock reads the number of steps taken so far: every step lasts exactly one second."""
    import time
    import types
    import torch
    calls = [0]
    monkeypatch.setattr(b, "time", types.SimpleNamespace(perf_counter=lambda: float(calls[0]), time=time.time, sleep=time.sleep))
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    lines = []
    monkeypatch.setattr(b, "emit", lines.append)
    return calls, lines


@pytest.mark.parametrize("mode", ["infer", "train"])
def test_plain_run_times_exactly_the_given_steps_and_dumps_the_last_one(tmp_path, monkeypatch, mode):
    """The timed region spans exactly --steps steps (one second each here: ms_per_step is exactly 1000) and --dump-outputs writes
    what the LAST timed step returned (each step returns its own number)."""
    import types
    import numpy as np
    import torch
    b = _bench()
    calls, lines = _counting_clock(monkeypatch, b)
    B, N, K, W = 2, 5, 7, 3
    topo = types.SimpleNamespace(num_nodes=N, num_undirected_edges=3)

    def step():
        calls[0] += 1
        return torch.full((B * N, 4), float(calls[0])) if mode == "infer" else torch.tensor(float(calls[0]))

    if mode == "infer":
        graph = types.SimpleNamespace(kidsum_rows=1)
        model = types.SimpleNamespace(_resolver=types.SimpleNamespace(resolve=lambda ei, n: (graph, None)), chain_layers=True,
                                      fuse_classifier=True)
        monkeypatch.setattr(b, "infer_workload", lambda *a, **k: (model, {}, topo, torch.zeros(B * N, 128), None, step))
        untimed = min(max(K + W, 32), 512) + W              # the launch burst in front of the warm-up steps, then the warm-up
    else:
        step.reducer, step.model = None, torch.nn.Linear(2, 2)
        monkeypatch.setattr(b, "train_workload", lambda *a, **k: (step, topo))
        untimed = W
    monkeypatch.setattr(sys, "argv", ["bench.py", "--mode", mode, "--batch", str(B), "--steps", str(K), "--warmup", str(W),
                                      "--spinup", "0", "--dump-outputs", str(tmp_path)])
    args = b.parse()
    (b.main_infer if mode == "infer" else b.main_train)(args, 1, 0, "cpu", {"world_size": 1, "backend": None})
    (d,) = lines
    assert calls[0] == untimed + K                           # nothing runs after the timed steps without --full
    assert d["steps"] == K and d["ms_per_step"] == 1000.0 and d["value"] == B
    for key in ("roofline", "repeats", "eager_ms_per_step", "hip_graph_replay", "cpu_baseline", "other_configs"):
        assert key not in d, key
    if mode == "infer":
        lg = np.load(tmp_path / "logits.npy")
        assert lg.dtype == np.float32 and lg.shape == (B * N, 4) and (lg == untimed + K).all()
    else:
        assert np.load(tmp_path / "loss.npy").tolist() == [untimed + K]
        assert sorted(os.listdir(tmp_path)) == ["loss.npy", "param.bias.npy", "param.weight.npy"]


def test_dump_outputs_keeps_to_its_budget_with_a_fixed_sample(tmp_path, monkeypatch):
    import numpy as np
    b = _bench()
    small = np.arange(12, dtype=np.float16).reshape(3, 4)
    b.dump_outputs(str(tmp_path / "a"), {"x": small, "y": np.ones(2)})
    assert sorted(os.listdir(tmp_path / "a")) == ["x.npy", "y.npy"]
    x = np.load(tmp_path / "a" / "x.npy")
    assert x.dtype == np.float32 and np.array_equal(x, small.astype(np.float32))
    assert np.load(tmp_path / "a" / "y.npy").dtype == np.float64
    monkeypatch.setattr(b, "DUMP_BYTES", 4096)
    big = np.random.default_rng(1).standard_normal((1000, 4)).astype(np.float32)
    for run in ("b", "c"):
        b.dump_outputs(str(tmp_path / run), {"logits": big})
    files = sorted(os.listdir(tmp_path / "b"))
    assert files == ["logits.npy", "logits_rows.npy"]
    assert sum(os.path.getsize(tmp_path / "b" / f) for f in files) <= 4096 + 2 * 128          # (+ the .npy headers)
    rows = np.load(tmp_path / "b" / "logits_rows.npy")
    assert rows.dtype == np.float64 and (np.diff(rows) > 0).all()
    assert np.array_equal(np.load(tmp_path / "b" / "logits.npy"), big[rows.astype(np.int64)])
    for f in files:
        assert np.array_equal(np.load(tmp_path / "b" / f), np.load(tmp_path / "c" / f))


def test_headline_of_a_full_result_fits_the_drivers_tail_window():
    """The driver keeps the last 2000 characters of the run's output: the stdout line must fit there as a WHOLE JSON object
    with the numbers a reader needs (round 5's line was 7 KB and arrived truncated)."""
    b = _bench()
    full = json.load(open(os.path.join(ROOT, "profiles", "r05_bench_default.json")))
    full["eager_ms_per_step"] = 0.8312
    full["cpu_baseline"]["sample_batch"] = 2
    h = b.headline_of(full, "gpurun_out/bench_details.json")
    line = json.dumps(h)
    assert len(line) <= 1536, len(line)          # 1.5 KB
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "eager_ms_per_step", "higher_is_better",
                "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline", "parity", "cfg4_train"):
        assert key in h, key
    assert h["roofline"]["frac"] == full["roofline"]["frac"] and h["roofline"]["traffic"] == full["roofline"]["traffic"]
    assert h["cfg4_train"]["traffic_bytes_per_step"] == full["other_configs"]["cfg4_train"]["traffic_bytes_per_step"]
    assert h["cpu_baseline"]["sample_batch"] == 2 and h["other_ms_per_step"]["cfg2_b1"] > 0


def test_only_the_result_line_reaches_stdout():
    """bench.py prints ONE JSON line.  Native libraries write to stdout as well (RCCL's version banner, block-buffered: behind a
    pipe it lands after the result): guard_stdout() points descriptor 1 at stderr, emit() writes the line to the real stdout."""
    import subprocess
    import sys
    import textwrap
    code = textwrap.dedent(f'''
        import ctypes, importlib.util, sys
        spec = importlib.util.spec_from_file_location("bench_module", {os.path.join(ROOT, "bench.py")!r})
        b = importlib.util.module_from_spec(spec); spec.loader.exec_module(b)
        b.guard_stdout()
        ctypes.CDLL(None).printf(b"native banner line\\n")
        print("a python print")
        b.emit({{"ok": 1}})
    ''')
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-1000:]
    assert r.stdout == '{"ok": 1}\n'
    assert "native banner line" in r.stderr and "a python print" in r.stderr
