"""bench.py --gpus 2 under torch.distributed.run, on the CPU: the N > 1 branch of the
script the driver launches on the multi-GPU node (rank/world handling, sharded runner,
barriers, max-over-ranks timing, the one JSON line of rank 0), run with the emulated
engine over gloo -- with torch's all_to_all and with the engine's own exchange (fake
RCCL).  Numbers are meaningless here; the contract of the line is what is checked."""
import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _final_and_rows(stdout, rows_file):
    """The contract of the output (the driver keeps a tail of stdout, round 5's single 28-KB line did not
    fit it): the LAST JSON line is the compact one (< 4 KB); every line before it is a detail row {"row": kind, ...};
    the rows file holds both."""
    lines = [ln for ln in stdout.splitlines() if ln.startswith("{")]
    assert lines and stdout.rstrip().splitlines()[-1] == lines[-1]
    assert len(lines[-1]) < 4096, len(lines[-1])
    final = json.loads(lines[-1])
    assert "row" not in final and "metric" in final and "value" in final
    rows = [json.loads(ln) for ln in lines[:-1]]
    assert all("row" in x and "metric" not in x for x in rows)
    with open(rows_file) as f:
        saved = json.load(f)
    assert saved["rows"] == rows and saved["final_line"] == final
    return final, rows


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("collective", ["torch", "rccl"])
def test_bench_two_ranks_gloo(collective, tmp_path):
    from emu.build_emu import build, build_fake_rccl
    build()
    env = dict(os.environ, MAXSUM_COLLECTIVE=collective,
               MAXSUM_RCCL_LIB=build_fake_rccl(), FAKE_RCCL_DIR=str(tmp_path), OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "tests", "emu", "run_emulated.py"), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "6", "--warmup", "2",
           "--full", "--backend", "gloo", "--vars-per-gpu", "300", "--rows-file", str(tmp_path / "rows.json")]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    out, rows = _final_and_rows(r.stdout, tmp_path / "rows.json")
    assert [x["row"] for x in rows] == ["extra", "extra"]   # rank 0 only
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "extras"):
        assert key in out, key
    assert out["n_gpus"] == 2 and out["steps"] == 6 and out["warmup"] == 2
    # N > 1 = STRONG scaling of ONE fixed instance, BASELINE configs[3] (here scaled down 1 : 333): value is the rate of
    # that instance -- no multiplication by N (VERDICT r4 / ADVICE r3: the weak-scaling aggregate is a labelled extra)
    assert out["scaling"] == "strong" and out["unit"].startswith("iterations/s of ONE 3000-variable instance") and out["dtype"] == "f64"
    cfg = out["config"]
    its = cfg["iterations_per_s_of_this_instance"]
    assert out["value"] == its == out["iterations_per_s_of_the_instance"]
    assert its > 0 and abs(its - 1e3 / out["ms_per_step"]) < 1e-6 * its
    ns = out["north_star_speedup"]   # north_star's ">= 6x at 8 GPUs" reading, at the top level
    assert ns["workload"].startswith("coloring_1m_deg6") and ns["scaling"] == "strong" and ns["speedup_vs_one_gpu"] > 0
    assert abs(ns["speedup_vs_one_gpu"] - out["value"] / out["one_gpu_iterations_per_s"]) < 1e-9
    assert cfg["workload"].startswith("coloring_1m_deg6 (BASELINE configs[3]): strong scaling")
    assert cfg["n_vars"] == 3000 and cfg["n_factors"] == 9000
    assert f"exchange: {collective}" in cfg["parallelism"]
    assert cfg["one_gpu_iterations_per_s"] > 0 and cfg["speedup_vs_one_gpu_on_this_instance"] > 0
    assert "cpu_baseline" not in out  # rank 0 at N = 1 only
    assert cfg["check"] == {"cycles": 8, "identical_to_single_engine": True, "differences": 0}
    # labelled extras: the weak-scaling aggregate of the metric's family (ONE 2 x 300-variable instance) and the metric's
    # own instance split two ways
    assert [e["workload"] for e in out["extras"]] == ["coloring_100k x2", "coloring_100k"]   # the final line: a summary
    assert all(e["identical_to_single_engine"] for e in out["extras"])
    weak, small = rows
    assert weak["scaling"] == "weak" and weak["n_vars"] == 600 and weak["workload"] == "coloring_100k x2"
    assert abs(weak["aggregate_iterations_per_s_per_100k_variables"] - 2 * weak["iterations_per_s_of_this_instance"]) < 1e-9 * weak["iterations_per_s_of_this_instance"]
    assert small["scaling"] == "strong" and small["n_vars"] == 300 and small["workload"] == "coloring_100k"
    for e in (weak, small):
        assert e["check"]["identical_to_single_engine"] and e["iterations_per_s_of_this_instance"] > 0
        assert e["speedup_vs_one_gpu"] > 0


def test_bench_single_gpu_line_carries_every_config(tmp_path):
    """N = 1 on the emulated engine, sizes scaled down by a patched workload table: the one JSON
    line has the top-level metric, the cpu_baseline object and one record per extra configuration
    with roofline + traffic source + the parity test id."""
    from emu.build_emu import build
    code = (
        f"import sys, runpy; sys.argv = ['bench.py', '--full', '--steps', '4', '--warmup', '1', '--vars-per-gpu', '400', '--reference-budget', '4', '--rows-file', {str(tmp_path / 'rows.json')!r}]\n"
        f"from pydcop_amd import engine; engine.register_test_engine({build()!r}, make_default=True)\n"
        "import pydcop_amd.generators as G\n"
        "_ising, _meet, _col = G.ising_grid, G.meeting_like, G.random_coloring\n"
        "G.ising_grid = lambda r, c, **k: _ising(12, 12, **k)\n"
        "G.meeting_like = lambda n, **k: _meet(40, **{**k, 'dom': 6})\n"
        "G.random_coloring = lambda n, **k: _col(min(n, 600), **k)\n"
        "_het = G.meeting_hetero\n"
        "G.meeting_hetero = lambda n, **k: _het(40, **{**k, 'doms': (6, 5)})\n"
        "_sf, _secp = G.scalefree_coloring, G.secp_like\n"
        "G.scalefree_coloring = lambda n, **k: _sf(min(n, 500), **k)\n"
        "G.secp_like = lambda a, b, c, **k: _secp(60, 40, 50, **k)\n"
        "_peav = G.peav_like\n"
        "G.peav_like = lambda *a, **k: _peav(40, 25, slots=10, max_length=4, max_resources_event=4, **k)\n"
        f"runpy.run_path({os.path.join(ROOT, 'bench.py')!r}, run_name='__main__')\n")
    env = dict(os.environ, OMP_NUM_THREADS="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    out, rows = _final_and_rows(r.stdout, tmp_path / "rows.json")
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline", "timing", "rows", "rows_file"):
        assert key in out, key
    assert out["n_gpus"] == 1 and out["config"]["workload"] == "coloring_100k" and out["dtype"] == "f64"
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic", "bytes_basis", "algorithmic_bytes_per_launch",
                "stored_bytes_per_launch", "avg_launch_us", "resident", "kernel", "hbm_resident_reference"):
        assert key in out["roofline"], key
    configs = [x for x in rows if x["row"] == "config"]
    algos = [x for x in rows if x["row"] == "algorithm"]
    head = [x for x in rows if x["row"] == "headline_detail"]
    assert len(head) == 1 and head[0]["timing"]["warmup_by_time_steps"] > 0 and head[0]["factor_kernels"]
    # the timed region: exactly `steps` cycles, their time / steps is the line's ms_per_step; --full adds the
    # repetitions of exactly `steps` cycles (median, fastest, slowest)
    tm = out["timing"]
    assert tm["timed_steps"] == out["steps"] == 4 and out["ms_per_step"] == tm["timed_region_ms"] / 4 > 0
    assert tm["steps_per_repetition"] == out["steps"] == 4 and tm["repeats"] >= 9
    assert tm["wall_iterations_per_s"] > 0   # the host-clock rate over the whole region, beside the event-clock median
    assert 0 < tm["ms_per_step_min"] <= tm["ms_per_step_median"] <= tm["ms_per_step_max"]
    assert abs(out["value"] - 1e3 / out["ms_per_step"]) < 1e-9 * out["value"]
    from oracle.stage_reference import locate
    cb = out["cpu_baseline"]
    if locate():   # the reference's own thread-agent runtime, timed in this run, leads; the C port is an extra
        assert cb["kind"] == "reference" and cb["value"] > 0 and cb["cores"] >= 1
        # the reference's rate on the benchmarked instance is an extrapolation of a measured sample, labelled so
        assert cb["extrapolated"] is True and cb["sample_measured_here"] is True and cb["sample_n_vars"] == 1000
        assert cb["port"]["kind"] == "port" and cb["port"]["value"] > 0
        detail = [x for x in rows if x["row"] == "cpu_baseline_detail"]
        assert len(detail) == 1 and all(t["n_vars"] == 1000 for t in detail[0]["thread_agents"])
    else:
        assert cb["kind"] == "port" and cb["value"] > 0
    assert out["roofline"]["traffic_source"] is None or "static" in out["roofline"]["traffic_source"]
    # a cache-resident headline never travels alone: the HBM-resident figure of the same kernel beside it
    assert out["roofline"]["resident"] in ("infinity_cache", "hbm")
    assert out["roofline"]["hbm_resident_reference"]["workload"] == "coloring_1m_deg6"
    got = {(c["workload"], c["dtype"]) for c in configs}
    assert {f"{w}/{d}" for w, d in got} | {"amaxsum", "dsa", "mgm"} == set(out["rows"])   # the one-glance summary
    for c in configs:
        us, frac = out["rows"][f"{c['workload']}/{c['dtype']}"]
        assert abs(us - c["roofline"]["avg_launch_us"]) <= 0.01 and abs(frac - c["roofline"]["frac"]) <= 0.001
    assert got == {("coloring_100k", "f32"), ("coloring_10k", "f64"), ("coloring_10k", "f32"),
                   ("ising_1024", "f64"), ("ising_1024", "f32"), ("coloring_1m_deg6", "f64"),
                   ("coloring_1m_deg6", "f32"), ("meeting_50k", "f64"), ("meeting_50k", "f32"),
                   ("peav_50k", "f64"), ("peav_50k", "f32"), ("coloring_100k_d8", "f64"), ("coloring_100k_d8", "f32"),
                   ("meeting_50k_float", "f64"), ("meeting_50k_float", "f32"),
                   ("meeting_50k_hetero", "f64"), ("meeting_50k_hetero", "f32"),
                   ("coloring_100k_scalefree", "f64"), ("coloring_100k_scalefree", "f32"),
                   ("secp_100k", "f64"), ("secp_100k", "f32"), ("secp_100k_m4", "f64"), ("secp_100k_m4", "f32")}
    for c in configs:
        assert c["parity_checked"] is True and c["parity_test"].startswith("tests/test_gpu_parity.py::")
        rf = c["roofline"]
        for key in ("achieved", "frac", "algorithmic_bytes_per_launch", "avg_launch_us", "traffic", "traffic_source"):
            assert key in rf
        assert c["ms_per_step"] > 0 and c["iterations_per_s"] > 0
    # the widened rows: amaxsum, DSA, MGM on the metric's instance, each naming its parity test
    assert [a["algo"].split()[0] for a in algos] == ["amaxsum", "dsa", "mgm"]
    assert algos[0]["messages"] > 0 and algos[0]["messages_per_s"] > 0
    for a in algos[1:]:
        assert a["cycles_per_s"] > 0 and a["cost_now"] <= a["cost_at_start"]
    for a in algos:   # every widened row with bytes by a stated formula and a fraction of the peak
        assert a["roofline"]["achieved"] > 0 and 0 < a["roofline"]["frac"] and "formula" in a["roofline"]
    for c in configs:  # tables stored narrow enough: the row leads with the stored-byte fraction
        if c["roofline"]["bytes_basis"] == "stored":
            assert c["roofline"]["stored_bytes_per_launch"] < 0.8 * c["roofline"]["algorithmic_bytes_per_launch"]
            assert c["roofline"]["frac"] == c["roofline"]["frac_of_stored_bytes"] and "frac_algorithmic" in c["roofline"]
    for a in algos:
        assert a["parity_test"].startswith("tests/test_gpu_") and os.path.exists(
            os.path.join(ROOT, a["parity_test"].split("::")[0]))


def test_bench_launches_its_own_ranks(tmp_path):
    """`python3 bench.py --gpus 2 ...` from a plain shell (no launcher, no WORLD_SIZE) -- the way the driver runs
    --gpus 1 -- starts its own ranks under torch.distributed.run and prints the same lines (task 2)."""
    from emu.build_emu import build, build_fake_rccl
    build()
    env = dict(os.environ, MAXSUM_COLLECTIVE="rccl", MAXSUM_RCCL_LIB=build_fake_rccl(), FAKE_RCCL_DIR=str(tmp_path),
               MAXSUM_BENCH_ENTRY=os.path.join(ROOT, "tests", "emu", "run_emulated.py") + " " + os.path.join(ROOT, "bench.py"))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "5", "--warmup", "2", "--backend", "gloo",
           "--vars-per-gpu", "300", "--configs", "main", "--rows-file", str(tmp_path / "rows.json"),
           "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    out, rows = _final_and_rows(r.stdout, tmp_path / "rows.json")
    assert out["n_gpus"] == 2 and out["steps"] == 5 and out["scaling"] == "strong" and rows == []
    import numpy as np   # the sharded run's selection and beliefs after the timed steps, written by rank 0
    assert out["outputs"] == {"selection": 3000, "belief": 3000}
    assert np.load(tmp_path / "out" / "selection.npy").shape == (3000,)
    assert out["config"]["check"]["identical_to_single_engine"] and out["north_star_speedup"]["n_gpus"] == 2
    assert out["ranks_seen"] == 2


def test_bench_rejects_mismatched_world():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1"],
                       env=dict(os.environ, WORLD_SIZE="1"), cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "WORLD_SIZE" in (r.stdout + r.stderr)


def _plain_run(tmp_path, tag, steps, warmup, extra=()):
    from emu.build_emu import build
    argv = ["bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--vars-per-gpu", "400",
            "--rows-file", str(tmp_path / f"rows_{tag}.json"), "--dump-outputs", str(tmp_path / tag), *extra]
    code = (f"import sys, runpy; sys.argv = {argv!r}\n"
            f"from pydcop_amd import engine; engine.register_test_engine({build()!r}, make_default=True)\n"
            f"runpy.run_path({os.path.join(ROOT, 'bench.py')!r}, run_name='__main__')\n")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, OMP_NUM_THREADS="1"), cwd=ROOT,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return _final_and_rows(r.stdout, tmp_path / f"rows_{tag}.json")


def test_bench_plain_run_is_lean_and_dumps_its_outputs(tmp_path, oracle_built):
    """`bench.py --gpus 1 --steps N --warmup W` without --full: the headline only (no detail rows, no cpu_baseline,
    no other configurations), exactly N timed steps, and --dump-outputs writes the state after W + N cycles --
    the same in two runs, and what the oracle computes after W + N cycles."""
    import numpy as np
    from oracle.maxsum_oracle import OracleMaxSum
    from pydcop_amd import generators as G
    from pydcop_amd.graph import Params
    out, rows = _plain_run(tmp_path, "a", steps=7, warmup=2)
    out2, _ = _plain_run(tmp_path, "b", steps=7, warmup=2)
    assert rows == []
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "timing"):
        assert key in out, key
    assert out["unit"] == "iterations/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
    assert "cpu_baseline" not in out and "rows" not in out
    assert out["steps"] == out["timing"]["timed_steps"] == 7 and out["warmup"] == out["timing"]["warmup_steps"] == 2
    assert out["ms_per_step"] > 0 and abs(out["value"] - 1e3 / out["ms_per_step"]) < 1e-9 * out["value"]
    names = ("selection", "belief", "v2f", "f2v", "count_v2f", "count_f2v", "cost")
    assert set(out["outputs"]) == set(names) and out["outputs"] == out2["outputs"]
    got = {}
    for name in names:
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype in (np.float32, np.float64) and a.shape == (out["outputs"][name],)
        assert np.array_equal(a, b), name
        got[name] = a
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= 64_000_000
    g = G.random_coloring(400, avg_degree=4, n_colors=3, seed=0, names=False)
    ora = OracleMaxSum(g, Params(mode="min", dtype="f64"))
    ora.run(2 + 7)
    idx, belief = ora.assignment()
    v2f, f2v, cv, cf = ora.messages()
    cost, viol = ora.eval_cost()
    ora.close()
    assert np.array_equal(got["selection"], idx) and np.array_equal(got["belief"], belief)
    assert np.array_equal(got["v2f"], v2f) and np.array_equal(got["f2v"], f2v)
    assert np.array_equal(got["count_v2f"], cv) and np.array_equal(got["count_f2v"], cf)
    assert got["cost"][1] == viol and abs(got["cost"][0] - cost) <= 1e-9 * max(1.0, abs(cost))


def test_bench_dump_outputs_samples_what_exceeds_the_limit(tmp_path, monkeypatch):
    """Outputs larger than the limit are written as a fixed, seeded sample with its positions."""
    import numpy as np
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 40_000)
    big, small = np.arange(10_000, dtype=np.float64), np.arange(10, dtype=np.int32)
    for tag in ("a", "b"):
        n = bench.dump_outputs(str(tmp_path / tag), {"big": big, "small": small, "flags": np.ones(5, np.uint8)})
        assert n["small"] == 10 and n["flags"] == 5 and 0 < n["big"] < 10_000
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= 40_000
    pos = np.load(tmp_path / "a" / "big_positions.npy")
    vals = np.load(tmp_path / "a" / "big.npy")
    assert vals.dtype == np.float64 and np.array_equal(vals, big[pos.astype(np.int64)]) and (np.diff(pos) > 0).all()
    assert np.load(tmp_path / "a" / "flags.npy").dtype == np.float32
    assert np.load(tmp_path / "a" / "small.npy").dtype == np.float64
    for name in ("big", "big_positions", "small", "flags"):
        assert np.array_equal(np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy"))
