"""bench.py --dump-outputs: write_outputs keeps a dump under its byte budget with a sample that is the
same in every run, and scan_output_arrays names every result field of the scan's output record."""

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _dir_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_small_arrays_are_written_whole_as_floats(tmp_path):
    arrays = {"a": np.arange(12.0).reshape(3, 4), "b": np.arange(5, dtype=np.float32), "c": np.arange(7)}
    w = bench.write_outputs(str(tmp_path), arrays)
    assert w == {"a": [12, 12], "b": [5, 5], "c": [7, 7]}
    a, b, c = (np.load(tmp_path / f"{k}.npy") for k in "abc")
    assert a.dtype == np.float64 and np.array_equal(a, arrays["a"])
    assert b.dtype == np.float32 and np.array_equal(b, arrays["b"])
    assert c.dtype == np.float64 and np.array_equal(c, arrays["c"])  # integers leave as float64


def test_large_arrays_are_sampled_the_same_way_under_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 1 << 16)
    rng = np.random.default_rng(3)
    arrays = {"big": rng.normal(size=(26, 1000)), "big2": rng.normal(size=30000).astype(np.float32),
              "small": rng.normal(size=22)}
    w1 = bench.write_outputs(str(tmp_path / "x"), arrays)
    w2 = bench.write_outputs(str(tmp_path / "y"), {k: v.copy() for k, v in arrays.items()})
    assert w1 == w2 and w1["small"] == [22, 22]
    assert w1["big"][0] < w1["big"][1] == 26000 and w1["big2"][0] < w1["big2"][1] == 30000
    for d in ("x", "y"):
        assert _dir_bytes(str(tmp_path / d)) <= 1 << 16
    for k in arrays:
        x, y = np.load(tmp_path / "x" / f"{k}.npy"), np.load(tmp_path / "y" / f"{k}.npy")
        assert np.array_equal(x, y)
    # the sample is elements of the array at increasing flat indices
    big = np.load(tmp_path / "x" / "big.npy")
    flat = arrays["big"].reshape(-1)
    pos = np.searchsorted(np.sort(flat), big)
    assert np.array_equal(np.sort(flat)[pos], big)
    idx = np.argsort(flat)[pos]
    assert np.all(np.diff(idx) > 0)


def test_scan_output_arrays_cover_the_result_fields():
    sys.path.insert(0, os.path.join(ROOT, "gc-slam_amd"))
    from gcslam import _lib as L
    out = L.GcsScanOutputs()
    out.z_t[2] = 1.5
    out.belief.L[23] = 2.0
    out.stage_ms[0] = 9.0
    arrs = bench.scan_output_arrays(out)
    want = {"scan_" + n for n, _ in L.GcsScanOutputs._fields_ if n not in ("belief", "stage_ms")}
    want |= {"scan_belief_" + n for n in ("X_anchor", "stamp_sec", "z_lin", "L", "h")}
    assert set(arrs) == want
    assert arrs["scan_z_t"][2] == 1.5 and arrs["scan_belief_L"][1, 1] == 2.0
    assert all(a.dtype == np.float64 for a in arrs.values())
