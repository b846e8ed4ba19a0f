"""IMU windows for the shape sweeps of the two one-workgroup IMU kernels (k_preint, gcs_preint.hip; k_imu_odom,
gcs_imu_odom.hip) and of the host entries beside them: one generator, seeded per (family, size, variant), the
case tables, each case's oracle result (computed once per process and shared by the CPU and the GPU file) and the
guards that show a case reaches the branch it is for.  numpy only.

Sizes sit on the kernels' seams: 64 lanes a wave, 128 keys a wave in io_sort (so 129 is the first window whose
network goes through LDS), 512 lanes a workgroup / samples a window_carry chunk, 1,024 keys in io_sort and the
largest k_imu_odom window.  io_pow2 of the listed seams skips the 16- and 32-key networks, so 16, 17, 32 and 33
stand beside them."""

import functools

import numpy as np

from oracle import ops, se3
from test_imu_odom import _inputs, _oracle

G_ACC = np.array([0.0, 0.0, 9.81])

# ------------------------------------------------------------------------------------------- IMU / odometry
IO_SIZES = (2, 3, 4, 5, 16, 17, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024)
IO_VARIANTS = ("ordered", "shuffled", "padded", "outside", "one_inside")
IO_CASES = [(m, v) for m in IO_SIZES for v in IO_VARIANTS]
IO_T0, IO_T1 = 100.0, 100.2
IO_EPS = 1e-9  # compute_imu_integration_time's window slack


def io_pow2(n):
    """gcs_imu_odom.hip io_pow2: the size of the sorting network for n keys."""
    p = 2
    while p < n:
        p <<= 1
    return p


def in_window(stamps, t0, t1):
    """The stamps dt_int is taken over (oracle.imu_odom.compute_imu_integration_time; k_imu_odom's compaction)."""
    s = np.asarray(stamps)
    return (s > t0 - IO_EPS) & (s <= t1 + IO_EPS) & (s > 0.0)


def _draw_stamps(rng, n, t0, t1):
    return np.sort(rng.uniform(t0 - 0.05, t1 + 0.02, n))


def _rng(family, m, variant, attempt=0):
    return np.random.default_rng([family, m, variant, attempt])


def _io_window(m, variant):
    """stamps, gyro, accel of one IMU / odometry window, and the generator for the rest of the inputs."""
    vi = IO_VARIANTS.index(variant)
    t0, t1 = IO_T0, IO_T1
    n = m - m // 3 if variant == "padded" else m
    for attempt in range(256):  # (a small window is drawn again until it can hold its variant)
        rng = _rng(0, m, vi, attempt)
        st = _draw_stamps(rng, n, t0, t1)
        if variant != "shuffled" or in_window(st, t0, t1).sum() >= 2:
            break
    else:
        raise AssertionError((m, variant))
    if variant == "one_inside":
        # every in-window stamp but one moves behind the window; with none inside, the middle one moves in
        inside = np.flatnonzero(in_window(st, t0, t1))
        keep = inside[inside.shape[0] // 2] if inside.shape[0] else n // 2
        st[inside] = t1 + 1e-3 + rng.uniform(0.0, 0.019, inside.shape[0])
        st[keep] = rng.uniform(t0 + 0.01, t1 - 0.01)
        st = np.sort(st)
    gy = rng.normal(0.0, 0.3, (n, 3))
    ac = rng.normal(0.0, 0.5, (n, 3)) + G_ACC
    if variant == "shuffled":
        p = rng.permutation(n)
        s = st[p][in_window(st[p], t0, t1)]
        if not np.any(s[1:] < s[:-1]):  # (a tiny window's draw can leave the in-window stamps in order)
            p = np.arange(n)[::-1]
        st, gy, ac = st[p], gy[p], ac[p]  # the samples travel with their stamps
    elif variant == "padded":
        if n > 4:
            st[n // 2 + 1] = st[n // 2]  # a repeated stamp among the real ones
        st = np.concatenate([st, np.zeros(m - n)])  # as the node pads: zero stamps, zero rates
        gy = np.concatenate([gy, np.zeros((m - n, 3))])
        ac = np.concatenate([ac, np.zeros((m - n, 3))])
    elif variant == "outside":
        st = st + 5.0
    return st, gy, ac, rng


@functools.lru_cache(maxsize=None)
def io_case(m, variant):
    """The inputs (test_imu_odom._inputs' dict, arrays read-only) of one IMU / odometry window."""
    st, gy, ac, rng = _io_window(m, variant)
    pose0 = np.concatenate([rng.normal(0, 0.2, 3), rng.normal(0, 0.1, 3)])
    pose_pred = np.asarray(se3.se3_compose(pose0, np.array([0.1, 0.0, 0.0, 0.0, 0.0, 0.03])), np.float64)
    sd_pose = np.array([0.01, 0.01, 0.01, 3.5e-3, 3.5e-3, 3.5e-3])
    sd_twist = np.array([0.02, 0.02, 0.02, 8.7e-3, 8.7e-3, 8.7e-3])
    odom_pose = pose_pred + sd_pose * rng.standard_normal(6)
    odom_twist = np.array([0.5, 0.0, 0.0, 0.0, 0.0, 0.15]) + sd_twist * rng.standard_normal(6)
    d = _inputs(st, gy, ac, IO_T0, IO_T1, IO_T1 - IO_T0, pose0, pose_pred, rng.normal(0, 1e-2, 22),
                rng.normal(0, 1e-2, 22), odom_pose, np.diag(sd_pose ** 2), odom_twist, np.diag(sd_twist ** 2),
                sigma_warp=0.02)
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def io_oracle(m, variant):
    """test_imu_odom._oracle of the case: (L, h, named, info, dt_int, dt_imu, omega_avg)."""
    return _oracle(io_case(m, variant))


def io_n_in(d):
    return int(in_window(d["stamps"], d["t_last_scan"], d["t_scan"]).sum())


def io_unordered(d):
    """True where two in-window stamps are out of order: k_imu_odom then sorts them for dt_int."""
    s = d["stamps"][in_window(d["stamps"], d["t_last_scan"], d["t_scan"])]
    return bool(np.any(s[1:] < s[:-1]))


def io_guard(m, variant):
    """The case holds what its variant is for (assertions on the inputs alone)."""
    d = io_case(m, variant)
    st = d["stamps"]
    assert st.shape == (m,) and d["gyro"].shape == (m, 3) and d["accel"].shape == (m, 3)
    n_in = io_n_in(d)
    if variant == "ordered":
        assert np.all(np.diff(st) > 0.0) and not io_unordered(d)
    elif variant == "shuffled":
        assert n_in >= 2 and io_unordered(d)
        assert np.all(np.diff(np.sort(st)) > 0.0)
        if m >= 1023:
            assert n_in > 512  # the compaction's second pass finds room taken by the first
    elif variant == "padded":
        n = m - m // 3
        assert np.all(st[n:] == 0.0) and np.all(d["gyro"][n:] == 0.0) and np.all(d["accel"][n:] == 0.0)
        assert np.all(st[:n] > 0.0) and not io_unordered(d)
        assert (np.sum(np.diff(st[:n]) == 0.0) == 1) == (n > 4)
    elif variant == "outside":
        assert n_in == 0 and np.all(st > IO_T1 + 1.0)
    elif variant == "one_inside":
        assert n_in == 1 and np.all(np.diff(st) > 0.0)


# ------------------------------------------------------------------------------------------- preintegration
PRE_SIZES = (1, 2, 3, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 1537)
PRE_T0, PRE_T1 = 100.0, 100.1
PRE_SIGMA = 0.013
PRE_ROTVEC = np.array([0.05, -0.3, 1.1])
PRE_GB = np.array([0.001, -0.002, 0.0005])
PRE_AB = np.array([0.02, 0.01, -0.03])
PRE_G = np.array([0.0, 0.0, -9.81])
PRE_TURN_RATE = np.array([6.0, 0.0, 20.0])  # rad/s: about 2.1 rad over the 0.1 s window
PRE_TRAILING = ((40, 2), (600, 89), (601, 89), (600, 200))  # (m, r) -> trimmed to 39, 512, 513, 401 samples

PRE_CASES = ([f"scale0.5-{m}" for m in PRE_SIZES] + [f"scale6-{m}" for m in PRE_SIZES] +
             [f"turn-{m}" for m in (65, 513, 1025)] + [f"trailing_run-{m}-{r}" for m, r in PRE_TRAILING] +
             ["all_equal-70", "still-513", "rotation_only-513"])
PRE_EXACT_ZERO = ("scale0.5-1", "scale6-1", "all_equal-70")


def trimmed_len(stamps):
    """The samples k_preint is given: the trailing run of repeated stamps is cut to its first one
    (gcs_capi.cpp launch_device_preint, gcs_debug_preintegrate)."""
    r = len(stamps) - 1
    while r > 0 and stamps[r - 1] == stamps[r]:
        r -= 1
    return r + 1


@functools.lru_cache(maxsize=None)
def pre_case(name):
    """dict(stamps, gyro, accel, t0, t1, rotation_only) of one preintegration window (arrays read-only)."""
    kind, *num = name.split("-")
    m = int(num[0])
    kinds = ("scale0.5", "scale6", "turn", "trailing_run", "all_equal", "still", "rotation_only")
    rng = _rng(1, m, kinds.index(kind), int(num[1]) if len(num) > 1 else 0)
    t0, t1 = PRE_T0, PRE_T1
    st = _draw_stamps(rng, m, t0, t1)
    scale = 6.0 if kind == "scale6" else 0.5
    gy = rng.normal(0.0, scale, (m, 3))
    ac = rng.normal(0.0, 1.0, (m, 3)) + G_ACC
    if kind == "turn":
        gy = gy + PRE_TURN_RATE
    elif kind == "trailing_run":
        r = int(num[1])
        head = _draw_stamps(rng, m - r, t0, t1)
        w = ops.smooth_window_weights(head, t0, t1, PRE_SIGMA)
        # one stamp well inside [t0, t1] (weight about 0.93), repeated r times behind the ordered ones
        st = np.concatenate([head, np.full(r, head[np.argmin(np.abs(w - 0.93))])])
    elif kind == "all_equal":
        st[:] = t0 + 0.04
    elif kind == "still":
        gy[:] = PRE_GB  # zero rates: every so3_exp takes its small-angle branch
    for a in (st, gy, ac):
        a.setflags(write=False)
    return dict(stamps=st, gyro=gy, accel=ac, t0=t0, t1=t1, rotation_only=kind == "rotation_only")


@functools.lru_cache(maxsize=None)
def pre_oracle(name):
    """(twist, oracle.ops.preintegrate_imu's dict) of the case, as tests/test_gpu_preint.py's _oracle."""
    c = pre_case(name)
    w = ops.smooth_window_weights(c["stamps"], c["t0"], c["t1"], PRE_SIGMA)
    pre = ops.preintegrate_imu(c["stamps"], c["gyro"], c["accel"], w, PRE_ROTVEC, PRE_GB, PRE_AB, PRE_G)
    xi = np.array(se3.se3_log(pre["delta_pose"]), np.float64)
    if c["rotation_only"]:
        xi[:3] = 0.0
    return xi, pre, w


def pre_guard(name):
    """The case holds what its variant is for (assertions on the inputs and the oracle alone)."""
    c = pre_case(name)
    xi, pre, w = pre_oracle(name)
    kind, *num = name.split("-")
    st, m = c["stamps"], int(num[0])
    assert st.shape == (m,)
    me = trimmed_len(st)
    angle = float(np.linalg.norm(pre["delta_pose"][3:6]))
    if kind in ("scale0.5", "scale6", "turn", "still", "rotation_only"):
        assert me == m and np.all(np.diff(st) > 0.0)
    if kind == "turn":
        assert 1.8 < angle <= 2.1  # large, and clear of so3_log's loss of conditioning towards pi
    elif kind == "trailing_run":
        r = int(num[1])
        assert me == m - r + 1 and np.all(st[m - r:] == st[m - 1]) and c["t0"] < st[m - 1] < c["t1"]
        assert np.all(np.diff(st[:m - r]) > 0.0) and st[m - 1] in st[:m - r]
        assert 0.9 < w[m - 1] < 0.96
        # a dropped or miscounted tail must show: the tail's weight beyond the kept sample is above 0.5
        assert pre["ess"] - w[:me].sum() > 0.5
    elif kind == "all_equal":
        assert me == 1 and np.all(st == st[0])
        assert np.all(pre["delta_pose"][:3] == 0.0) and np.all(pre["delta_v"] == 0.0)
        assert angle < 1e-15 and w[0] > 0.5 and pre["ess"] > 0.5 * m  # the trimmed 69 samples carry the ess
    elif kind == "still":
        assert np.all(c["gyro"] == PRE_GB) and angle < 1e-15 and np.linalg.norm(pre["delta_v"]) > 0.1
    return me


# ------------------------------------------------------------------------------------------- whole scans
def recut_imu(sc, n):
    """The scan with its IMU window cut anew to n samples, no padding: the synthetic IMU interpolated linearly
    over its valid span."""
    st = sc["imu_stamps"]
    v = st > 0.0
    t = np.linspace(st[v][0], st[v][-1], n)
    cut = lambda a: np.stack([np.interp(t, st[v], a[v][:, k]) for k in range(3)], axis=1)  # noqa: E731
    return dict(sc, imu_stamps=t, imu_gyro=cut(sc["imu_gyro"]), imu_accel=cut(sc["imu_accel"]))
