"""The line the driver parses: bench.py prints its sub-records first and ONE compact line last.
BENCH_r05.json was unparsed because the single line had grown to 20 KB; these tests pin the size and the keys."""
import io
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (stdlib imports only at module level)

FULL = os.path.join(ROOT, "profiles", "r5_fused_c2", "bench_default_with_extras.json")   # a complete default-run record (20 KB, round 5)

CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config", "roofline", "cpu_baseline")


def _full():
    with open(FULL) as fh:
        return json.load(fh)


def test_compact_line_is_last_small_and_complete(tmp_path):
    full = _full()
    buf = io.StringIO()
    text = bench.emit(full, str(tmp_path / "full.json"), buf)
    lines = buf.getvalue().splitlines()
    assert lines[-1] == text and buf.getvalue().endswith(text + "\n")
    assert len(text) < 4096
    line = json.loads(text)
    for k in CONTRACT:
        assert k in line, k
    assert line["value"] == pytest.approx(full["value"], rel=1e-5)
    assert line["ms_per_step"] == pytest.approx(full["ms_per_step"], rel=1e-5)
    assert line["config"]["workload"].startswith("C2: 2000 keypoints")
    assert set(("bound", "achieved", "peak", "unit", "frac", "traffic", "launch_ms")) <= set(line["roofline"])
    assert line["roofline"]["frac"] == pytest.approx(line["roofline"]["achieved"] / line["roofline"]["peak"], rel=1e-4)
    assert set(("value", "unit", "cores", "kind", "sample")) <= set(line["cpu_baseline"])
    assert line["label_match_vs_cpu_reference"] == 1.0 and line["tiles_identical"] is True
    for sub in ("c1", "c3", "c4", "n500", "c5", "c5_single_frame", "single_frame_latency_us", "single_frame_latency_us_n500"):
        assert sub in line, sub
    # the complete record is on disk and every sub-record is a line of its own before the compact one
    assert json.load(open(tmp_path / "full.json"))["c4"]["value"] == full["c4"]["value"]
    recs = [json.loads(l).get("record") for l in lines[:-1]]
    assert {"c1", "c3", "c4", "n500", "c5", "cpu_baseline", "end_to_end", "roofline_detail"} <= set(recs)


def test_compact_line_has_no_note_strings():
    line = bench.compact_line(_full())

    def strings(o):
        if isinstance(o, dict):
            for v in o.values():
                yield from strings(v)
        elif isinstance(o, list):
            for v in o:
                yield from strings(v)
        elif isinstance(o, str):
            yield o
    assert max(len(s) for s in strings(line)) <= 80


def test_compact_line_stays_small_with_long_numbers_and_multi_gpu():
    """Worst case: every float at full repr length, 8 ranks, every optional key present."""
    full = _full()

    def inflate(o):
        if isinstance(o, dict):
            return {k: inflate(v) for k, v in o.items()}
        if isinstance(o, list):
            return [inflate(v) for v in o]
        if isinstance(o, float):
            return o * 1.0000001234567 + 1e-9
        return o
    full = inflate(full)
    full["n_gpus"] = 8
    full["multi_gpu"] = {"ms_per_step_by_rank": [1.8234567891234] * 8, "ranks_in_collective": 8, "backend": "nccl",
                         "label_gather": {"serial_ms_per_step": 1.9, "overlapped_ms_per_step": 1.83, "exposed_ms_per_step": 0.07123456789,
                                          "bytes_per_rank": 4194304}}
    full["label_gather_ok"] = True
    full["device"] = "AMD Instinct MI355X pci 0000:f5:00 uuid 0123456789abc"
    full["end_to_end"]["host_to_host"] = dict(full["end_to_end"]["host_to_host"], best_frames_per_s=1.3312345678e6, best_frac_of_link=0.8412345678)
    full["c5"]["single_frame"]["frac_wall"] = 0.40123456789
    text = bench.emit(full, None, io.StringIO())
    assert len(text) < 4096
    assert json.loads(text)["multi_gpu"]["ranks_in_collective"] == 8


def test_plain_record_prints_the_compact_line_alone():
    """A plain run (no --full) records the timed steps and their configuration only: the compact line is all it prints, with no
    empty sections for what only --full measures."""
    full = _full()
    plain = {k: full[k] for k in CONTRACT[:-2] + ("build_ms_per_batch", "scaling_measured")}
    buf = io.StringIO()
    text = bench.emit(plain, None, buf)
    assert buf.getvalue() == text + "\n"
    line = json.loads(text)
    assert set(line) == set(plain)
    assert line["value"] == pytest.approx(full["value"], rel=1e-5)
    assert line["ms_per_step"] == pytest.approx(full["ms_per_step"], rel=1e-5)


def test_oversized_line_is_refused(monkeypatch):
    monkeypatch.setattr(bench, "COMPACT_LIMIT", 512)
    with pytest.raises(SystemExit):
        bench.emit(_full(), None, io.StringIO())


class _Batch:
    """Stand-in for a BatchCRF handle: the two host accessors --dump-outputs reads."""

    def __init__(self, Q, M):
        self.Q, self.M = Q, M

    def probability(self):
        return self.Q.copy()

    def map(self):
        return self.M.copy()


def test_dump_outputs_writes_a_fixed_sample_within_the_budget(tmp_path, monkeypatch):
    import numpy as np
    rng = np.random.default_rng(1)
    F, N, L = 2000, 100, 2
    Q = rng.random((F, N, L), dtype=np.float32)
    M = rng.integers(0, L, (F, N)).astype(np.int16)
    batches = [_Batch(Q[:1200], M[:1200]), _Batch(Q[1200:], M[1200:])]
    monkeypatch.setattr(bench, "DUMP_LIMIT", 10 ** 6)
    runs = []
    for d in ("a", "b"):
        S = bench.dump_outputs(str(tmp_path / d), batches)
        assert 0 < S < F
        assert sum(os.path.getsize(tmp_path / d / f) for f in os.listdir(tmp_path / d)) <= 10 ** 6
        runs.append({n: np.load(tmp_path / d / (n + ".npy")) for n in ("probability", "map", "frame_index")})
    for n in runs[0]:
        assert runs[0][n].dtype in (np.float32, np.float64), n
        assert np.array_equal(runs[0][n], runs[1][n]), n                 # the same sample every run
    sel = runs[0]["frame_index"].astype(np.int64)
    assert len(np.unique(sel)) == sel.size == runs[0]["probability"].shape[0] and np.all(np.diff(sel) > 0)
    assert np.array_equal(runs[0]["probability"], Q[sel]) and np.array_equal(runs[0]["map"], M[sel].astype(np.float32))
    # a batch within the budget is written whole
    assert bench.dump_outputs(str(tmp_path / "c"), [_Batch(Q[:50], M[:50])]) == 50
    assert np.array_equal(np.load(tmp_path / "c" / "probability.npy"), Q[:50])


@pytest.mark.gpu
def test_bench_dumps_what_its_last_timed_step_computed(tmp_path, po, wl):
    """bench.py --dump-outputs on a small C2 batch: --steps sets the timed steps, and the dumped Q and labels are the CPU checker's
    for the frames they name, bit for bit."""
    import subprocess
    import numpy as np
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--frames", "256",
                        "--no-extras", "--no-cpu-baseline", "--no-check", "--full-json", str(tmp_path / "full.json"),
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 2 and line["warmup"] == 1
    Q, M, sel = (np.load(out / (n + ".npy")) for n in ("probability", "map", "frame_index"))
    assert Q.dtype == M.dtype == np.float32 and Q.shape == (256, 2000, 2) and M.shape == (256, 2000)
    assert np.array_equal(sel, np.arange(256))
    for f in (0, 1, 63, 64, 255):
        pb = wl.slam_problem(2000, f % 64 + 1)                            # bench.make_batch: 64 distinct frames, seeds 1.., tiled
        o = po.OracleCRF(pb["N"], pb["L"])
        o.set_unary_from_label(pb["label"], pb["conf"])
        for feat, w in pb["kernels"]:
            o.add_pairwise(feat, w)
        o.inference_native(5, True)
        assert np.array_equal(M[f], o.map().astype(np.float32)), f
        assert np.array_equal(Q[f].view(np.int32), o.probability().view(np.int32)), f
        o.close()


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_full_adds_the_records(tmp_path):
    """bench.py without --full prints the headline line alone and writes no full record; with --full the same command adds the
    kernel timing and roofline, the parity gate and the end-to-end record, and writes the full record."""
    import subprocess
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--frames", "256",
           "--distinct", "4", "--full-json", str(tmp_path / "full.json")]
    lines = {}
    for mode, extra in (("plain", []), ("full", ["--full", "--no-extras", "--no-cpu-baseline"])):
        r = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        out = r.stdout.strip().splitlines()
        lines[mode] = json.loads(out[-1])
        records = [l for l in out[:-1] if l.startswith('{"record"')]
        if mode == "plain":
            assert not records and not (tmp_path / "full.json").exists()
        else:
            assert "roofline_detail" in [json.loads(l)["record"] for l in records]
            assert json.load(open(tmp_path / "full.json"))["value"] == pytest.approx(lines[mode]["value"], rel=1e-5)
    for line in lines.values():
        for k in CONTRACT[:-2]:
            assert k in line, k
        assert line["steps"] == 2 and line["warmup"] == 1 and line["config"]["frames_in_flight_per_gpu"] == 256
    assert not {"roofline", "label_match_vs_cpu_reference", "tiles_identical", "end_to_end", "cpu_baseline"} & set(lines["plain"])
    full = lines["full"]
    assert full["roofline"]["launch_ms"] > 0 and full["end_to_end"]["one_launch_ms_per_batch"] > 0
    assert full["label_match_vs_cpu_reference"] == 1.0 and full["tiles_identical"] is True and full["frames_checked"] == 4
