"""The host IMU entries (gcs_preintegrate_imu, gcs_imu_odom_evidence) against the numpy oracle on every window of
tests/imu_window_util.py -- the windows the device sweep (tests/test_gpu_imu_window_shapes.py) runs --, the
generator's guards, and the proof that the cases between them reach every branch of k_preint and k_imu_odom that
depends on the window's shape.  Host numerics only: no GPU.  Bars: tests/test_imu_odom.py's (_compare) and
tests/test_gpu_preint.py's (1e-12 absolute on the delta pose and the twist, relative 1e-13 on ess)."""

import numpy as np
import pytest

import imu_window_util as U
from oracle import se3
from test_imu_odom import _compare, _hip


def _id(c):
    return f"{c[0]}-{c[1]}"


@pytest.mark.parametrize("case", U.IO_CASES, ids=_id)
def test_host_imu_odom_matches_oracle(lib, case):
    U.io_guard(*case)
    d = U.io_case(*case)
    L_h, h_h, cert = _hip(lib, d)
    _compare(L_h, h_h, cert, U.io_oracle(*case))
    if U.io_n_in(d) < 2:
        assert cert[10] == 0.0


@pytest.mark.parametrize("name", U.PRE_CASES)
def test_host_preintegration_matches_oracle(lib, name):
    from gcslam import _lib as L
    me = U.pre_guard(name)
    c = U.pre_case(name)
    xi, pre, w = U.pre_oracle(name)
    dp, ess = np.zeros(6), np.zeros(1)
    args = [np.ascontiguousarray(a, np.float64) for a in (c["stamps"], c["gyro"], c["accel"], w, U.PRE_ROTVEC, U.PRE_GB,
                                                            U.PRE_AB, U.PRE_G)]
    assert lib.gcs_preintegrate_imu(len(w), *[L.dptr(a) for a in args], L.dptr(dp), L.dptr(ess)) == 0
    np.testing.assert_allclose(dp, pre["delta_pose"], rtol=0, atol=1e-12)
    assert ess[0] == pytest.approx(pre["ess"], rel=1e-13)
    xi_h = np.array(se3.se3_log(dp), np.float64)
    if c["rotation_only"]:
        xi_h[:3] = 0.0
    np.testing.assert_allclose(xi_h, xi, rtol=0, atol=1e-12)
    if name in U.PRE_EXACT_ZERO:
        assert me == 1 and np.all(dp == 0.0)


def test_cases_reach_every_branch():
    """Every shape-dependent path of the two kernels is taken by some case ("IMU windows")."""
    io = {c: U.io_case(*c) for c in U.IO_CASES}
    n_in = {c: U.io_n_in(d) for c, d in io.items()}
    unordered = {c for c, d in io.items() if U.io_unordered(d)}
    # the medians: both parities of m, every network io_sort can run
    assert {m % 2 for m in U.IO_SIZES} == {0, 1}
    assert {U.io_pow2(m) for m in U.IO_SIZES} == {1 << k for k in range(1, 11)}
    assert min(U.IO_SIZES) == 2 and max(U.IO_SIZES) == 1024  # the refusals stand just outside
    # the dt_int sort runs (two in-window stamps out of order) at every size, and with them the network of n_in
    # keys from the smallest to the largest; the ordered windows skip it
    assert {m for m, v in unordered} == set(U.IO_SIZES) and unordered == {c for c in io if c[1] == "shuffled"}
    assert {U.io_pow2(n_in[c]) for c in unordered} >= {2, 4, 64, 128, 256, 512, 1024}
    # n_in: none, one (dt_int = 0 by the count), a few, and more than a compaction pass holds
    assert {0, 1} <= set(n_in.values()) and any(2 <= n <= 512 for n in n_in.values())
    assert all(n_in[(m, "shuffled")] > 512 and n_in[(m, "ordered")] > 512 for m in (1023, 1024))
    # the compaction's second pass with nothing before it, and the padding's stamps (<= 0) inside no window
    assert all(n_in[(m, "outside")] == 0 and n_in[(m, "one_inside")] == 1 for m in U.IO_SIZES)
    # window_carry in k_imu_odom: one chunk, a full chunk, a second chunk of 1 / 511 / 512 samples
    assert {512, 513, 1023, 1024} <= set(U.IO_SIZES)
    # k_preint: the trimmed lengths around the wave, the chunk, two chunks, a fourth chunk of one sample
    trimmed = {U.trimmed_len(U.pre_case(n)["stamps"]) for n in U.PRE_CASES}
    assert trimmed >= {1, 2, 3, 39, 63, 64, 65, 401, 511, 512, 513, 1023, 1024, 1025, 1537}
    assert any(U.pre_case(n)["rotation_only"] for n in U.PRE_CASES)
    tails = {len(U.pre_case(n)["stamps"]) - U.trimmed_len(U.pre_case(n)["stamps"]) for n in U.PRE_CASES}
    assert tails == {0, 1, 69, 88, 199}


def test_recut_imu_keeps_the_span():
    from gcslam import synthetic
    sc = synthetic.make_scan(16, 3)
    v = sc["imu_stamps"] > 0.0
    for n in (37, 200, 1100):
        r = U.recut_imu(sc, n)
        assert r["imu_stamps"].shape == (n,) and r["imu_gyro"].shape == (n, 3) and r["imu_accel"].shape == (n, 3)
        assert np.all(np.diff(r["imu_stamps"]) > 0.0)
        assert r["imu_stamps"][0] == sc["imu_stamps"][v][0] and r["imu_stamps"][-1] == sc["imu_stamps"][v][-1]
        assert np.allclose(r["imu_gyro"][[0, -1]], sc["imu_gyro"][v][[0, -1]], rtol=0, atol=1e-15)
