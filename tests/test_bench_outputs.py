"""bench.py's result line and --dump-outputs: the line is one compact JSON object whose `steps` are the timed steps and whose `ms_per_step` is one of
them; the dump is what the last timed step delivered (result rows, MPDU bytes) as float32 / float64 .npy files, at most 64 MB, the same from
run to run for the same arguments.  A plain run carries the headline only; --full adds the reference check, the roofline and the CPU baseline."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _table(n, frame_len=1500):
    import sora_amd
    rows = np.zeros(n, sora_amd.ROW_DTYPE)
    rows["capture_id"] = np.arange(n)
    rows["error_code"] = np.where(np.arange(n) % 5 == 4, sora_amd.E_PLCP_HEADER_FAIL, sora_amd.E_FRAME_OK)
    rows["error_code"][3] = sora_amd.E_CRC32_FAIL
    rows["length"] = frame_len
    rows["cfo_est"] = -7
    rows["crc32"] = 0xFFFFFFFF
    rows["mpdu_offset"] = np.arange(n) * frame_len
    return rows, np.random.default_rng(n).integers(0, 256, n * frame_len).astype(np.uint8)


def _load(d):
    return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_writes_rows_and_mpdus_exactly(tmp_path):
    import bench
    import sora_amd
    rows, mpdu = _table(64)
    bench.dump_outputs(str(tmp_path), sora_amd, rows, mpdu)
    got = _load(str(tmp_path))
    assert set(got) == {"row_index.npy", "mpdu.npy"} | {"row_%s.npy" % f for f in rows.dtype.names}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    for f in rows.dtype.names:
        assert np.array_equal(got["row_%s.npy" % f], rows[f].astype(np.float64)), f
    carried = [i for i in range(64) if rows["error_code"][i] in (sora_amd.E_FRAME_OK, sora_amd.E_CRC32_FAIL)]
    want = np.concatenate([mpdu[rows["mpdu_offset"][i]:rows["mpdu_offset"][i] + 1500] for i in carried])
    assert np.array_equal(got["mpdu.npy"], want.astype(np.float32))


def test_dump_outputs_of_a_large_table_is_a_fixed_sample_under_64_mb(tmp_path):
    import bench
    import sora_amd
    rows, mpdu = _table(16000, 4095)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), sora_amd, rows, mpdu)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert sum(os.path.getsize(str(tmp_path / "a" / f)) for f in a) <= 64 * 10 ** 6
    assert set(a) == set(b) and all(np.array_equal(a[f], b[f]) for f in a)
    idx = a["row_index.npy"].astype(np.int64)
    assert 0 < len(idx) < len(rows) and np.all(np.diff(idx) > 0)
    assert np.array_equal(a["row_capture_id.npy"], rows["capture_id"][idx].astype(np.float64))


@pytest.mark.gpu
def test_bench_line_and_dump_on_the_gpu(tmp_path):
    """Two small runs with different --steps: each line's `steps` / `timed_steps` are its --steps, the line stays compact, the dumps are equal."""
    lines = []
    for d, k in (("a", 3), ("b", 7)):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(k), "--warmup", "2", "--frames", "256", "--check", "16",
                            "--full", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / d)], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        out = [ln for ln in p.stdout.splitlines() if ln.strip()]
        assert len(out) == 1, p.stdout[-3000:]
        assert len(out[0]) < 16384, len(out[0])
        r = json.loads(out[0])
        assert r["steps"] == k and r["timed_steps"] == k and r["ms_per_step"] > 0 and r["parity"]["ok"], r
        lines.append(r)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert set(a) == set(b) and all(np.array_equal(a[f], b[f]) for f in a)
    assert len(a["row_index.npy"]) == lines[0]["delivery"]["rows_per_call"] and a["mpdu.npy"].size > 0


FULL_ONLY = ("parity", "roofline", "kernel_ms", "kernel_ms_one_call_in_flight", "ms_per_step_profiled", "cpu_baseline", "gathered")


@pytest.mark.gpu
def test_plain_bench_run_is_the_headline_alone(tmp_path):
    """A run without --full prints the headline fields and none of what --full measures, and its timed steps deliver exactly what a --full
    run's do: the two dumps are equal."""
    lines = {}
    for d, extra in (("plain", []), ("full", ["--full", "--check", "16", "--no-cpu-baseline"])):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--frames", "256",
                            "--dump-outputs", str(tmp_path / d)] + extra, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        out = [ln for ln in p.stdout.splitlines() if ln.strip()]
        assert len(out) == 1, p.stdout[-3000:]
        lines[d] = json.loads(out[0])
    r = lines["plain"]
    assert r["full"] is False and lines["full"]["full"] is True
    assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"} <= set(r), r
    assert r["metric"] == lines["full"]["metric"] and r["unit"] == "Msamples/s" and r["higher_is_better"] is True and r["dtype"] == lines["full"]["dtype"]
    assert r["steps"] == 3 and r["timed_steps"] == 3 and r["value"] > 0 and r["ms_per_step"] > 0
    assert r["delivery"]["calls_with_wrong_rows"] == 0 and r["delivery"]["calls_delivered_and_compared"] > 0, r["delivery"]
    assert not set(FULL_ONLY) & set(r), set(FULL_ONLY) & set(r)
    assert {"parity", "roofline", "kernel_ms_one_call_in_flight"} <= set(lines["full"]) and lines["full"]["parity"]["ok"]
    a, b = _load(str(tmp_path / "plain")), _load(str(tmp_path / "full"))
    assert set(a) == set(b) and all(np.array_equal(a[f], b[f]) for f in a)
