"""gcs_camera_splats at the shapes and branches the workload uses, against the reference's own code:
tests/golden/camera_edges_*.npz (tests/golden/make_camera_splats_edges.py) hold a scene of 11,372
points from 2.5 to 48 m with patches of up to 1,304 candidates per feature, 300 features and what the
reference gave under four configs; tests/camera_pad.py pads the cloud to 16,500 / 65,536 / 66,000 points
(more than one wave of k_cs_offsets, max_points, two blocks per thread).

Bars: those of tests/test_gpu_camera_splats.py (integer decisions exact; Route A bitwise in its order
statistics with identity extrinsics, rtol 1e-9 otherwise; Route B and the batch arrays rtol 1e-7), with
the Route-B / batch atol taken per feature row, 1e-7 max|ref| of that row.  Features whose plane fit
the fixture flags as undetermined (an eigen-gap under 1e-3) are compared on everything that does not
pass through the eigenvector.  Every comparison prints its worst error / tolerance ratio."""

import ctypes as C
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from camera_pad import PADDED_SIZES, digest, filler, pad_cloud
from gcslam.camera import CameraSplatBuilder, DepthFusionConfig, PinholeIntrinsics

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CASES = ("r8_A", "r8_B", "r3_A", "fit_A", "depth_A")
BATCH_F64 = ("Lambdas", "thetas", "etas", "weights", "timestamps", "colors")
BATCH_INT = ("sources", "source_indices", "valid_mask")
FEATURE_KEYS = ("u", "v", "depth_Lambda_c", "depth_theta_c", "weight", "kappa_app", "mu_app", "has_mu", "color",
                "has_color")
N_FEAT, N_SURFEL, LDS_CAP = 512, 64, 1024


def _load(name):
    return dict(np.load(os.path.join(GOLD, f"camera_edges_{name}.npz")))


@pytest.fixture(scope="module")
def scene():
    return _load("scene")


@pytest.fixture(scope="module")
def ref():
    return {c: _load(c) for c in CASES + ("r8_E",)}


def _config(scene, cid):
    row = scene["cfg_values"][list(scene["config_ids"]).index(cid)]
    return DepthFusionConfig(**{str(k): (int(v) if is_int else float(v))
                                for k, v, is_int in zip(scene["cfg_names"], row, scene["cfg_is_int"])})


def _features(scene, idx):
    f = {k: scene[k][idx] for k in FEATURE_KEYS}
    f.update(xyz=scene["xyz_in"][idx], cov=scene["cov_in"][idx])
    return f


def _builder(scene, cid, **kw):
    kw.setdefault("n_feat", N_FEAT)
    kw.setdefault("max_points", 16384)
    return CameraSplatBuilder(_config(scene, cid), n_surfel=N_SURFEL, eps_lift=float(scene["eps_lift"]), **kw)


def _points(scene, ref, case):
    return (ref[case]["points_base"] if case.endswith("_B") else scene["points"]).astype(np.float64)


def _build(bld, scene, idx, points, R=np.eye(3), t=np.zeros(3)):
    """One call on the features idx; host copies of the batch and the diagnostics."""
    b = bld.build(_features(scene, idx), points, PinholeIntrinsics(*scene["intrinsics"]), R, t,
                  float(scene["timestamp"]), want_diag=True)
    out = {k: getattr(b, k).cpu().numpy() for k in BATCH_F64 + BATCH_INT}
    out.update({k: v.cpu().numpy() for k, v in b.camera_diag.items()})
    out["n_camera_valid"] = b.n_camera_valid
    return out


def _run_rows(ref, case):
    """Features of a case that fit the kernel's 1,024-candidate LDS table (the others fail the call)."""
    return np.flatnonzero(ref[case]["n_pt"] <= LDS_CAP)


@pytest.fixture(scope="module")
def runs(scene, ref):
    """One call per recorded case on every feature that fits the candidate table, shared below."""
    out = {}
    for case in CASES:
        bld = _builder(scene, case.split("_")[0])
        try:
            out[case] = _build(bld, scene, _run_rows(ref, case), _points(scene, ref, case),
                               ref[case]["R_base_camera"], ref[case]["t_base_camera"])
        finally:
            bld.close()
    return out


def _close(name, got, want, rtol, atol):
    """|got - want| <= atol + rtol |want| elementwise; atol a scalar or one value per leading row."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    atol = np.asarray(atol, np.float64)
    if atol.ndim == 1:
        atol = atol.reshape((-1,) + (1,) * (want.ndim - 1))
    err = np.abs(got - want)
    tol = atol + rtol * np.abs(want)
    ratio = np.where(err == 0.0, 0.0, err / np.maximum(tol, 1e-300))
    print(f"{name}: rows {got.shape[0]}, max abs err {err.max() if err.size else 0.0:.3e}, worst err / tol "
          f"{ratio.max() if ratio.size else 0.0:.3e}")
    bad = ~(err <= tol)
    assert not bad.any(), f"{name}: {bad.sum()} / {bad.size} outside tol; worst err / tol {ratio.max():.3e}"


def _close_rows(name, got, want):
    """The Route-B / batch bar: rtol 1e-7, atol 1e-7 max|ref| of each feature's row."""
    want = np.asarray(want, np.float64)
    row_max = np.abs(want.reshape(want.shape[0], -1)).max(axis=1) if want.size else np.zeros(want.shape[0])
    _close(name, got, want, 1e-7, 1e-7 * row_max)


def _same_bits(a, b, what):
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), f"{what}: {k} differs"


def _check(name, got, scene, r, idx, identity, n_feat=N_FEAT):
    """Every assertion of one call on the features idx against the recorded case r."""
    m = idx.size
    n = min(m, n_feat)
    det = r["plane_determined"][idx]
    assert np.array_equal(got["n_pt"], r["n_pt"][idx]), f"{name}: n_pt"
    assert np.array_equal(got["fused"].astype(bool)[det], r["fused"][idx][det]), f"{name}: fused"
    for k in ("z_med", "mad"):
        want = r[k][idx]
        ok = np.isfinite(want)
        assert np.array_equal(np.isfinite(got[k]), ok) and np.array_equal(np.isnan(got[k]), ~ok), f"{name}: {k} NaN pattern"
        if identity:
            assert np.array_equal(got[k][ok].view(np.int64), want[ok].view(np.int64)), f"{name}: {k} bits"
        else:
            _close(f"{name} {k}", got[k][ok], want[ok], 1e-9, 1e-12)
    for k in ("Lambda_A", "theta_A"):        # no eigenvector: every feature
        _close(f"{name} {k}", got[k], r[k][idx], 1e-9, 0.0 if identity else 1e-12)
    for k in ("Lambda_B", "theta_B", "z_f"):
        _close_rows(f"{name} {k}", got[k][det], r[k][idx][det])
    assert got["n_camera_valid"] == n
    dn = det[:n]
    want = dict(Lambdas=r["Lambdas"][idx][:n], thetas=r["thetas"][idx][:n], weights=r["weights"][idx][:n],
                colors=r["colors"][idx][:n], timestamps=np.full(n, float(scene["timestamp"])))
    etas = np.zeros((n, 3, 3))
    etas[:, 0] = r["eta0"][idx][:n]
    want["etas"] = etas
    for k in BATCH_F64:
        _close_rows(f"{name} {k}", got[k][:n][dn], want[k][dn])
        assert not got[k][n:].any(), f"{name}: {k} padding rows"       # and the untouched LiDAR slice
    for k in ("weights", "colors", "timestamps"):                       # independent of the plane fit: all rows
        _close_rows(f"{name} {k} (all rows)", got[k][:n], want[k])
    assert not got["etas"][:n, 1:].any()
    total = n_feat + N_SURFEL
    assert np.array_equal(got["valid_mask"], np.arange(total) < n)
    assert np.array_equal(got["source_indices"], np.where(np.arange(total) < n, np.arange(total), 0))
    assert not got["sources"].any()


@pytest.mark.parametrize("case", CASES)
def test_recorded_case(scene, ref, runs, case):
    idx = _run_rows(ref, case)
    assert idx.size >= 257
    _check(case, runs[case], scene, ref[case], idx, identity=case.endswith("_A"))


@pytest.mark.parametrize("m", [1, 256, 257])
def test_feature_subsets_are_the_same_rows(scene, ref, runs, m):
    """Features are independent; only the box (and with it the table) changes with the feature set."""
    idx = _run_rows(ref, "r8_A")
    r = ref["r8_A"]
    # m = 1: a degenerate box around a feature that runs both routes on more than 256 candidates
    first = int(np.flatnonzero((r["n_pt"][idx] > 256) & r["plane_determined"][idx])[0])
    sel = np.arange(first, first + 1) if m == 1 else np.arange(m)
    bld = _builder(scene, "r8")
    try:
        got = _build(bld, scene, idx[sel], _points(scene, ref, "r8_A"))
    finally:
        bld.close()
    _check(f"m={m}", got, scene, r, idx[sel], identity=True)
    full = runs["r8_A"]
    for k in ("n_pt", "z_med", "mad", "Lambda_A", "theta_A", "Lambda_B", "theta_B", "z_f", "fused"):
        assert got[k].tobytes() == full[k][sel].tobytes(), k
    for k in ("Lambdas", "thetas", "etas", "weights", "colors"):
        assert got[k][:sel.size].tobytes() == full[k][sel].tobytes(), k


def test_n_feat_smaller_than_the_feature_count(scene, ref, runs):
    """Rows past n_feat: diagnostics only."""
    idx = _run_rows(ref, "r8_A")
    bld = _builder(scene, "r8", n_feat=128)
    try:
        got = _build(bld, scene, idx, _points(scene, ref, "r8_A"))
    finally:
        bld.close()
    _check("n_feat=128", got, scene, ref["r8_A"], idx, identity=True, n_feat=128)
    full = runs["r8_A"]
    for k in ("n_pt", "z_med", "mad", "Lambda_A", "theta_A", "Lambda_B", "theta_B", "z_f", "fused"):
        assert got[k].shape[0] == idx.size and got[k].tobytes() == full[k].tobytes(), k
    for k in BATCH_F64:
        assert got[k][:128].tobytes() == full[k][:128].tobytes(), k


@pytest.mark.parametrize("n_total", PADDED_SIZES)
def test_padded_cloud(scene, ref, runs, n_total):
    """More than 64 blocks (the scan's cross-wave prefix), n_points == max_points = 65,536, and 258
    blocks (two per thread): the outputs are those of the stored cloud, bit for bit."""
    cloud = pad_cloud(scene["points"], n_total)
    assert digest(cloud) == str(scene["padded_sha256"][list(scene["padded_sizes"]).index(n_total)])
    max_points = n_total if n_total <= 65536 else 70000
    idx = _run_rows(ref, "r8_A")
    bld = _builder(scene, "r8", max_points=max_points)
    try:
        got = _build(bld, scene, idx, cloud.astype(np.float64))
    finally:
        bld.close()
    _same_bits(got, runs["r8_A"], f"padded to {n_total}")
    _check(f"padded {n_total}", got, scene, ref["r8_A"], idx, identity=True)


def test_one_point_more_than_max_points_raises(scene, ref, runs):
    cloud = pad_cloud(scene["points"], PADDED_SIZES[0]).astype(np.float64)
    bld = _builder(scene, "r8", max_points=PADDED_SIZES[0] - 1)
    try:
        with pytest.raises(ValueError, match="n_points exceeds max_points"):
            _build(bld, scene, _run_rows(ref, "r8_A"), cloud)
        assert not (cloud[-1] == scene["points"].astype(np.float64)).all(axis=1).any()      # a filler row
        got = _build(bld, scene, _run_rows(ref, "r8_A"), cloud[:-1])      # n_points == max_points runs
        _same_bits(got, runs["r8_A"], "n_points == max_points")
    finally:
        bld.close()


def test_candidate_capacity_exactly_reached(scene, ref, runs):
    idx = _run_rows(ref, "r8_A")
    n = ref["r8_A"]["n_pt"][idx]
    cap = int(n.max())
    assert 900 < cap <= LDS_CAP
    bld = _builder(scene, "r8", max_candidates=cap)
    try:
        _same_bits(_build(bld, scene, idx, _points(scene, ref, "r8_A")), runs["r8_A"], f"max_candidates={cap}")
    finally:
        bld.close()
    bld = _builder(scene, "r8", max_candidates=cap - 1)
    try:
        first = int(np.flatnonzero(n > cap - 1)[0])
        with pytest.raises(RuntimeError, match=rf"feature {first} has more than max_candidates={cap - 1} "):
            _build(bld, scene, idx, _points(scene, ref, "r8_A"))
    finally:
        bld.close()


def test_more_than_1024_candidates_raise_and_leave_no_valid_row(scene, ref):
    """All 300 features at the default capacity: the first feature past the LDS table is named, its
    candidate count is still the reference's, and (through the C-ABI, as the wrapper raises before it
    returns a batch) no row is left valid."""
    from gcslam import _lib as L
    from gcslam.surfels import create_empty_measurement_batch
    r = ref["r8_A"]
    over = np.flatnonzero(r["n_pt"] > LDS_CAP)
    assert over.size >= 3
    m = r["n_pt"].shape[0]
    bld = _builder(scene, "r8")
    try:
        with pytest.raises(RuntimeError, match=rf"feature {over[0]} has more than max_candidates=1024 "):
            _build(bld, scene, np.arange(m), _points(scene, ref, "r8_A"))
        fa = bld.device_features(_features(scene, np.arange(m)))
        p = torch.as_tensor(_points(scene, ref, "r8_A"), device=DEV).contiguous()
        batch = create_empty_measurement_batch(N_FEAT, N_SURFEL, DEV)
        batch.valid_mask[:] = True          # stale content the failing call must clear
        batch.weights[:] = 1.0
        n_pt = torch.full((m,), -1, dtype=torch.int32, device=DEV)
        i, o = L.GcsCamsplatInputs(), L.GcsCamsplatOutputs()
        i.points_base, i.n_points, i.n_features = p.data_ptr(), p.shape[0], m
        i.R_base_camera[:], i.t_base_camera[:] = np.eye(3).reshape(9).tolist(), [0.0, 0.0, 0.0]
        i.fx, i.fy, i.cx, i.cy = (float(x) for x in scene["intrinsics"])
        for k, v in fa.items():
            setattr(i, k, v.data_ptr())
        for k in L.CAMSPLAT_BATCH_FIELDS:
            x = getattr(batch, k)
            setattr(o, k, (x.view(torch.uint8) if k == "valid_mask" else x).data_ptr())
        o.n_pt = n_pt.data_ptr()
        torch.cuda.synchronize()
        rc = bld.lib.gcs_camera_splats(bld.h, C.byref(i), C.byref(o))
        assert rc == -4 and o.n_camera_valid == 0
        assert np.array_equal(n_pt.cpu().numpy(), r["n_pt"])            # counted past the table, exactly
        assert not batch.valid_mask[:N_FEAT].any() and not batch.weights[:N_FEAT].any()
        assert not batch.Lambdas[:N_FEAT].any() and not batch.thetas[:N_FEAT].any()
    finally:
        bld.close()


def test_no_point_and_all_points_behind_the_camera(scene, ref):
    """Every row: the incoming splat (re-projected at its camera depth where it has one) in the base frame."""
    idx = np.arange(scene["u"].shape[0])
    bld = _builder(scene, "r8")
    try:
        empty = _build(bld, scene, idx, np.zeros((0, 3)))
        behind = filler(512)[::2].astype(np.float64)
        assert (behind[:, 2] < 0).all()
        hidden = _build(bld, scene, idx, behind)
    finally:
        bld.close()
    _check("no points", empty, scene, ref["r8_E"], idx, identity=True)
    _same_bits(hidden, empty, "all points behind the camera")


def test_builder_reused_for_a_large_then_a_small_cloud(scene, ref, runs):
    """The large call leaves a table beyond the small call's cnt[kCntTab]; a fresh builder's bits."""
    idx = _run_rows(ref, "r8_A")
    bld = _builder(scene, "r8", max_points=70000)
    try:
        big = _build(bld, scene, idx, pad_cloud(scene["points"], PADDED_SIZES[2]).astype(np.float64))
        small = _build(bld, scene, idx, _points(scene, ref, "r8_A"))
        few = _build(bld, scene, idx, _points(scene, ref, "r8_A")[:700])
    finally:
        bld.close()
    _same_bits(big, runs["r8_A"], "66k cloud")
    _same_bits(small, runs["r8_A"], "small cloud after the 66k cloud")
    fresh = _builder(scene, "r8")
    try:
        _same_bits(few, _build(fresh, scene, idx, _points(scene, ref, "r8_A")[:700]), "700 points after the 66k cloud")
    finally:
        fresh.close()


@pytest.mark.parametrize("case", ["r8_A", "r8_B", "fit_A"])
def test_two_runs_are_bitwise_equal(scene, ref, runs, case):
    bld = _builder(scene, case.split("_")[0])
    try:
        again = _build(bld, scene, _run_rows(ref, case), _points(scene, ref, case), ref[case]["R_base_camera"],
                       ref[case]["t_base_camera"])
    finally:
        bld.close()
    _same_bits(again, runs[case], case)
