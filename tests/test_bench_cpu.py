"""bench.py's host-side logic (no GPU): counter records are never reported stale, counter arithmetic follows the MI355X
guide, the rank environment is the same for both launch forms, a wedged phase ends the process, and `--gpus N` from a
bare shell starts its own ranks."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_help_and_defaults():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--frames" in out.stdout and "--channels-per-gpu" in out.stdout
    a = bench.build_parser().parse_args([])
    assert (a.gpus, a.window, a.channels_per_gpu, a.frames) == (1, 1024, None, None)       # rank_main: 1024 x 512 at one GPU
    assert not a.full                                                                       # a plain run is the headline alone


def _rank_main_recording(monkeypatch, argv):
    """rank_main on CPU (the oracle standing in for the analyser, under the product engine's name) with the side measurements
    replaced by recorders: which of them ran, and the line."""
    from test_sharded_cpu import _OracleEngine

    class Engine(_OracleEngine):
        name = "gpu"

    ran = []

    def counters(window, channels, frames, input_file, **kw):
        ran.append("counters")
        assert np.load(input_file).shape == (channels, frames, window)                 # the same bytes as the timed region
        return {"FETCH_SIZE": 1.0, "WRITE_SIZE": 1.0}, "recorded"

    def extras(*a, **kw):
        ran.append("extras")
        return {"recorded": True}

    def cpu_baseline(*a, **kw):
        ran.append("cpu_baseline")
        return {"value": 1.0}

    monkeypatch.setattr(bench, "measure_counters", counters)
    monkeypatch.setattr(bench, "extras", extras)
    monkeypatch.setattr(bench, "cpu_baseline", cpu_baseline)
    args = bench.build_parser().parse_args(["--channels-per-gpu", "2", "--frames", "3", "--steps", "2", "--warmup", "1"] + argv)
    return bench.rank_main(args, Engine(), 0, 1), ran


def test_a_plain_run_does_only_the_headline(monkeypatch, capsys):
    """Without --full a run sets up, warms up, times its steps and prints: no counter passes, no extras, no CPU baseline."""
    d, ran = _rank_main_recording(monkeypatch, [])
    assert ran == []
    assert d["cpu_baseline"] is None and "not requested" in d["roofline"]["counters_source"] and d["roofline"]["traffic"] is None
    assert d["steps"] == 2 and d["roofline"]["launches_timed"] == 2 and d["value"] > 0 and d["ms_per_step"] > 0
    assert "bench.py extras" not in capsys.readouterr().err


def test_full_adds_counters_extras_and_the_cpu_baseline(monkeypatch, capsys):
    d, ran = _rank_main_recording(monkeypatch, ["--full"])
    assert sorted(ran) == ["counters", "cpu_baseline", "extras"]
    assert d["cpu_baseline"] == {"value": 1.0} and d["roofline"]["counters_source"] == "recorded" and d["roofline"]["traffic"] == 3 * 1024.0
    assert 'bench.py extras: {"recorded": true}' in capsys.readouterr().err
    d, ran = _rank_main_recording(monkeypatch, ["--full", "--no-pmc", "--no-extra", "--no-cpu-baseline"])
    assert ran == [] and d["cpu_baseline"] is None


def test_options_of_full_runs_are_refused_without_it():
    for flag in (["--only-extra", "osc_sink"], ["--write-counters"]):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + flag, capture_output=True, text=True)
        assert p.returncode == 2 and "--full" in p.stderr, flag


def test_committed_counters_are_never_reported_stale(tmp_path):
    """A committed counter record is a fallback for runs that cannot read counters themselves, and only if it was taken
    from exactly the kernel sources that are running: after any change under csrc/ it reads as absent, not as a number."""
    sha = bench.kernel_sources_sha()
    assert len(sha) == 16 and sha == bench.kernel_sources_sha()
    path = str(tmp_path / "counters.json")
    pmc = {"FETCH_SIZE": 1058689.4, "WRITE_SIZE": 115145.3, "SQ_INSTS_VALU": 2734.6 * 524288}
    json.dump({"1024:1024:512": {"pmc": pmc, "kernel_sources_sha": sha}}, open(path, "w"))
    rec, why = bench.committed_counters(1024, 1024, 512, path=path)
    assert rec and rec["pmc"]["FETCH_SIZE"] == pmc["FETCH_SIZE"] and "same kernel sources" in why
    rec, why = bench.committed_counters(1024, 1024, 512, path=path, sources_sha="0" * 16)
    assert rec is None and "stale" in why
    rec, why = bench.committed_counters(2048, 1024, 512, path=path)
    assert rec is None                                                               # other shapes: unknown, not guessed
    rec, why = bench.committed_counters(1024, 1024, 512, path=str(tmp_path / "missing.json"))
    assert rec is None
    # whatever is committed in profiles/ obeys the same rule
    rec, why = bench.committed_counters(1024, 1024, 512)
    assert rec is None or rec["kernel_sources_sha"] == sha


def test_counter_arithmetic_follows_the_guide():
    """HBM bytes = 2 x FETCH_SIZE + WRITE_SIZE (KB; gfx950 tallies 128-B read requests at 64 B), per launch; instruction
    counts per frame; per-wave activity as a share of wave cycles."""
    n = 1024 * 512
    f = bench.counters_to_fields({"FETCH_SIZE": 1058689.4, "WRITE_SIZE": 115145.3, "SQ_INSTS_VALU": 2734.6 * n, "SQ_INSTS_LDS": 400.0 * n,
                                  "SQ_WAVE_CYCLES": 1000.0, "SQ_ACTIVE_INST_VALU": 230.0, "SQ_WAIT_INST_LDS": 128.0}, n)
    algorithmic = (4 * 1024 + 48) * n
    assert algorithmic <= f["traffic"] <= 1.1 * algorithmic
    assert abs(f["valu_insts_per_frame"] - 2734.6) < 1e-6 and abs(f["lds_insts_per_frame"] - 400.0) < 1e-9
    assert abs(f["valu_active_per_wave"] - 0.23) < 1e-12 and abs(f["lds_issue_stall_per_wave"] - 0.128) < 1e-12
    assert bench.counters_to_fields({}, n) == {}
    assert abs(bench.flops_per_frame(1024) - 235520.0) < 1e-6 and 5.0e5 < bench.flops_per_frame(2048) < 5.2e5


def test_usable_cores_is_sane():
    n = bench.usable_cores()
    assert 1 <= n <= (os.cpu_count() or 1)


def test_rank_environment_is_the_same_for_both_launch_forms(monkeypatch):
    """What self_launch hands its children and what a rank started by the driver's own torch.distributed.run command sets
    for itself is one function: HSA_ENABLE_IPC_MODE_LEGACY=0 (dmabuf IPC, which RCCL's peer buffers need here)."""
    env = bench.rank_environment({})
    assert env["HSA_ENABLE_IPC_MODE_LEGACY"] == "0" and "OMP_NUM_THREADS" in env
    assert bench.rank_environment({"HSA_ENABLE_IPC_MODE_LEGACY": "1"})["HSA_ENABLE_IPC_MODE_LEGACY"] == "1"   # an explicit choice wins
    monkeypatch.delenv("HSA_ENABLE_IPC_MODE_LEGACY", raising=False)
    bench.rank_environment()
    assert os.environ["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_watchdog_ends_a_wedged_phase():
    code = ("import sys, time; sys.path.insert(0, %r); import bench\n"
            "with bench.Watchdog(1, 'a phase that never ends'):\n"
            "    time.sleep(30)\n" % ROOT)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=25)
    assert p.returncode == 124 and "did not finish within 1 s" in p.stderr
    with bench.Watchdog(30, "a phase that ends"):
        pass                                                                       # cancelled: nothing fires later


def test_committed_bench_line_has_the_contract_fields():
    paths = sorted(p for p in os.listdir(os.path.join(ROOT, "profiles")) if p.endswith("_bench.json") and p.startswith("r03"))
    if not paths:
        pytest.skip("no round-3 bench line committed yet")
    d = json.loads(open(os.path.join(ROOT, "profiles", paths[-1])).read().strip().splitlines()[-1])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["vs_baseline"] is None and d["scaling"] == "weak" and d["dtype"] == "f32" and "workload" in d["config"]
    r = d["roofline"]
    assert r["unit"] == "GB/s" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12
    c = r["compute"]
    assert r["bound"] == "valu" and abs(c["frac"] - c["achieved_tflops"] / c["peak_no_fma"]) < 1e-12 and c["peak_tflops"] == 157.3


def test_gpus_n_without_a_launcher_starts_its_own_ranks(monkeypatch):
    """`python bench.py --gpus 4` from a bare shell must start 4 child ranks through torch.distributed.run (and never
    exec) without touching the GPU itself; with WORLD_SIZE set (the driver's torchrun form) it must not."""
    import subprocess as sp
    seen = {}

    class Done:
        returncode = 0

    def fake_run(cmd, env=None, **kw):
        seen["cmd"], seen["env"] = cmd, env
        return Done()

    monkeypatch.setattr(sp, "run", fake_run)
    monkeypatch.setattr(bench, "visible_gpus", lambda: 4)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "7"])
    try:
        bench.main()
    except SystemExit as e:
        assert e.code == 0
    cmd = seen["cmd"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node" in cmd and cmd[cmd.index("--nproc-per-node") + 1] == "4"
    assert "127.0.0.1" in cmd and cmd[-4:] == ["--gpus", "4", "--steps", "7"] and cmd[-5].endswith("bench.py")
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
    # too few GPUs for RCCL: refuse loudly instead of hanging in the communicator
    monkeypatch.setattr(bench, "visible_gpus", lambda: 1)
    try:
        bench.main()
        raise AssertionError("expected SystemExit")
    except SystemExit as e:
        assert "only 1 GPU" in str(e.code)


def test_no_nested_profiler_children():
    """A bench.py that runs under rocprofv3 must not start rocprofv3 children of its own (they would inherit the tool library,
    initialise the GPU in the launcher and then exec)."""
    import bench
    assert not bench.under_profiler({})
    assert bench.under_profiler({"LD_PRELOAD": "/opt/rocm/lib/librocprofiler-sdk-tool.so"})
    assert bench.under_profiler({"ROCPROF_OUTPUT_PATH": "/tmp/x"})
    assert bench.under_profiler({"ROCP_TOOL_LIBRARIES": "/opt/rocm/lib/rocprofiler-sdk/librocprofiler-sdk-tool.so"})


def test_dump_outputs_writes_the_last_timed_step_and_steps_sets_the_timed_calls(tmp_path):
    """--dump-outputs DIR: raw / smoothed of the LAST timed step as DIR/<name>.npy (float32), on inputs that are the same from run to
    run; --steps is the number of timed calls.  rank_main on CPU with the oracle standing in for the GPU analyser."""
    from test_sharded_cpu import _OracleEngine
    from oracle import fx_oracle as fo
    from importlib import import_module
    fx = import_module("feature-extractor_amd")
    C, T, N, steps, warmup = 3, 4, 1024, 3, 1
    args = bench.build_parser().parse_args(["--channels-per-gpu", str(C), "--frames", str(T), "--steps", str(steps), "--warmup", str(warmup),
                                            "--no-cpu-baseline", "--no-extra", "--no-pmc", "--dump-outputs", str(tmp_path / "out")])
    d = bench.rank_main(args, _OracleEngine(), 0, 1)
    assert d["steps"] == steps and d["roofline"]["launches_timed"] == steps and d["ms_per_step"] > 0
    assert d["dumped_outputs"]["files"] == ["raw", "smoothed"] and not d["dumped_outputs"]["sampled"]
    assert len(json.dumps(d)) < 4096                                  # a line a reader of the tail of stdout can parse whole
    frames = fx.synth.frames(C, T, N)
    want = [fo.Channel(N) for _ in range(C)]
    for _ in range(warmup + steps):
        got = [ch.process_frames(frames[c]) for c, ch in enumerate(want)]
    for k, name in enumerate(("raw", "smoothed")):
        a = np.load(str(tmp_path / "out" / (name + ".npy")))
        assert a.dtype == np.float32 and a.shape == (C, T, 12)
        assert np.array_equal(a, np.stack([g[k] for g in got]), equal_nan=True), name


def test_dump_outputs_samples_channels_above_the_limit(tmp_path, monkeypatch):
    """Above the size limit a fixed, seeded sample of channels is written (the same one every run), with its indices."""
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1 << 20)
    x = np.arange(1000 * 50 * 12, dtype=np.float32).reshape(1000, 50, 12)
    recs = [bench.dump_outputs(str(tmp_path / k), {"raw": x, "smoothed": -x}) for k in ("a", "b")]
    assert recs[0]["sampled"] and 0 < recs[0]["channels"] < 1000 and recs[0]["files"] == ["channels", "raw", "smoothed"]
    total = sum(os.path.getsize(str(tmp_path / "a" / f)) for f in os.listdir(str(tmp_path / "a")))
    assert total <= 1 << 20
    keep = np.load(str(tmp_path / "a" / "channels.npy"))
    assert keep.dtype == np.float64 and np.array_equal(keep, np.load(str(tmp_path / "b" / "channels.npy")))
    raw = np.load(str(tmp_path / "a" / "raw.npy"))
    assert raw.dtype == np.float32 and np.array_equal(raw, x[keep.astype(np.int64)])


def test_steps_below_one_is_refused():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True)
    assert p.returncode == 2 and "--steps" in p.stderr
