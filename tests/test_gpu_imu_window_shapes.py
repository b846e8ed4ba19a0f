"""k_preint (gcs_preint.hip) and k_imu_odom (gcs_imu_odom.hip) at every window shape of tests/imu_window_util.py:
the sizes on the wave, sort-network, workgroup and chunk seams, unordered and padded windows, windows with no or
one stamp inside, the trimmed trailing run, and one context across large and small windows.  Each case is one or two
one-workgroup launches against the numpy oracle at the bars of tests/test_gpu_preint.py and
tests/test_imu_odom.py (_compare); tests/test_imu_window_shapes.py runs the same windows through the host entries
and shows that the cases reach every shape-dependent branch.

The one bar of this file's own: dt_int, dt_imu and transport_sigma come from the same sorted keys on the device and
on the host (only dt_int's gap sum, at most 1,023 positive terms, is added in another order), so they agree to a
relative 1e-13."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import imu_window_util as U
from gcslam import synthetic
from test_gpu_imu_odom import _branch_mismatches, _ctx, _device, _scans_both_branches
from test_gpu_preint import _assert_prologues_agree, _device_preint, _scans_both_prologues
from test_imu_odom import _compare, _hip

pytestmark = pytest.mark.gpu

SORT_CERTS = [10, 11, 3]  # dt_int, dt_imu, transport_sigma


@pytest.fixture(scope="module")
def ctx():
    c = _ctx()
    yield c
    c.close()


def _preint(name):
    c = U.pre_case(name)
    return _device_preint(c["stamps"], c["gyro"], c["accel"], c["t0"], c["t1"], U.PRE_SIGMA, U.PRE_ROTVEC, U.PRE_GB,
                          U.PRE_AB, c["rotation_only"])


# ------------------------------------------------------------------------------------------------ k_preint
@pytest.mark.parametrize("name", U.PRE_CASES)
def test_k_preint_window_matches_oracle(name):
    U.pre_guard(name)
    out = _preint(name)
    xi, pre, _ = U.pre_oracle(name)
    np.testing.assert_allclose(out[:6], xi, rtol=0, atol=1e-12)
    assert out[6] == pytest.approx(pre["ess"], rel=1e-13)
    np.testing.assert_allclose(out[7:13], pre["delta_pose"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(out[13:16], pre["delta_v"], rtol=0, atol=1e-11)
    if name in U.PRE_EXACT_ZERO:  # one sample after the trim: dt = 0, an exact identity
        assert np.all(out[:6] == 0.0) and np.all(out[7:16] == 0.0)


def test_k_preint_large_small_large():
    a = _preint("scale6-1537")
    _preint("scale6-3")
    b = _preint("scale6-1537")
    assert a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------- k_imu_odom
@pytest.mark.parametrize("case", U.IO_CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_k_imu_odom_window_matches_oracle(ctx, lib, case):
    U.io_guard(*case)
    d = U.io_case(*case)
    L_d, h_d, cert = _device(ctx, d)
    _compare(L_d, h_d, cert, U.io_oracle(*case))
    cert_h = _hip(lib, d)[2]
    np.testing.assert_allclose(cert[SORT_CERTS], cert_h[SORT_CERTS], rtol=1e-13, atol=0)
    if U.io_n_in(d) < 2:
        assert cert[10] == 0.0 and cert_h[10] == 0.0


def _bytes(res):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in res)


def test_k_imu_odom_one_context_many_windows():
    """A large unordered window, a tiny one, a padded one, the first again: the staged window, the LDS pads and
    the stamped record hold nothing of the call before (each result bitwise that of a fresh context)."""
    seq = [(1024, "shuffled"), (3, "ordered"), (129, "padded"), (1024, "shuffled")]
    fresh = {}
    for case in set(seq):
        c = _ctx()
        try:
            fresh[case] = _bytes(_device(c, U.io_case(*case)))
        finally:
            c.close()
    c = _ctx()
    try:
        got = [_bytes(_device(c, U.io_case(*case))) for case in seq]
    finally:
        c.close()
    assert [g == fresh[case] for g, case in zip(got, seq)] == [True] * len(seq)


def test_k_imu_odom_refusals_leave_the_context_usable(ctx):
    case = (65, "ordered")
    d1 = U.io_case(2, "ordered")
    d1 = dict(d1, stamps=d1["stamps"][:1], gyro=d1["gyro"][:1], accel=d1["accel"][:1], w_int=d1["w_int"][:1])
    d2 = U.io_case(1024, "ordered")
    d2 = dict(d2, **{k: np.concatenate([d2[k], d2[k][-1:]]) for k in ("stamps", "gyro", "accel", "w_int")})
    assert d1["stamps"].shape == (1,) and d2["stamps"].shape == (1025,)
    for d, msg in ((d1, "missing input"), (d2, "2 .. 1024 samples")):
        with pytest.raises(AssertionError, match=msg):
            _device(ctx, d)
        _compare(*_device(ctx, U.io_case(*case)), U.io_oracle(*case))


# --------------------------------------------------------------------------------------------- whole scans
DENSE = dict(n_bins=48, n_points_cap=2048, max_raw_points=4096, mode="dense")


def test_scans_device_preint_at_other_window_lengths():
    """Three scans with k_preint's twist against the host prologue's, the IMU windows cut anew to 200, 1,100
    (the staged window grows past its first 7 x 512 words) and 37 samples, none padded."""
    scans = [U.recut_imu(synthetic.make_scan(4096, 51 + k), n) for k, n in enumerate((200, 1100, 37))]
    _assert_prologues_agree(_scans_both_prologues(scans, **DENSE))


def test_scans_device_imu_odom_at_other_window_lengths():
    """Two scans with the device IMU / odometry branch against the host branch: windows of 1,024 samples (two
    keys a lane, two chunks), then 111."""
    scans = [U.recut_imu(synthetic.make_scan(4096, 120 + s), n) for s, n in enumerate((1024, 111))]
    bad = _branch_mismatches(_scans_both_branches(scans, "dense", 48, 2048, 4096))
    assert not bad, bad
