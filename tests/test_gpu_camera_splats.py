"""gcs_camera_splats against the reference's own code: tests/golden/camera_splats.npz holds the
inputs and what the reference's lidar_depth_evidence / splat_prep_fused, the node's base-frame
conversion and the camera slice of the MeasurementBatch gave on them (tests/golden/make_camera_splats.py).

Case A has identity extrinsics, so the kernel's base -> camera transform is exact and Route A's order
statistics must equal the reference's bit for bit; case B has a real R_base_camera / t_base_camera.
Bars: integer decisions exact; Route A (no eigenvector) rtol 1e-9; everything that passes through
Route B's plane-fit eigenvector, and the batch arrays, rtol 1e-7 with atol 1e-7 max|ref| per array
(the bars of tests/test_gpu_surfels.py)."""

import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from gcslam.camera import CameraSplatBuilder, DepthFusionConfig, PinholeIntrinsics, camera_batch_from_features

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH_F64 = ("Lambdas", "thetas", "etas", "weights", "timestamps", "colors")


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "camera_splats.npz")))


def _features(fx):
    return dict(u=fx["u"], v=fx["v"], depth_Lambda_c=fx["depth_Lambda_c"], depth_theta_c=fx["depth_theta_c"],
                xyz=fx["xyz_in"], cov=fx["cov_in"], weight=fx["weight"], kappa_app=fx["kappa_app"],
                mu_app=fx["mu_app"], has_mu=fx["has_mu"], color=fx["color"], has_color=fx["has_color"])


def _config(fx):
    return DepthFusionConfig(lidar_projection_radius_pix=float(fx["radius"]))


def _run(fx, case, n_feat=128, want_diag=True, builder=None):
    args = (_features(fx), fx[f"{case}_points_base"].astype(np.float64), PinholeIntrinsics(*fx["intrinsics"]),
            fx[f"{case}_R_base_camera"], fx[f"{case}_t_base_camera"], float(fx["timestamp"]))
    if builder is not None:
        return builder.build(*args, want_diag=want_diag)
    return camera_batch_from_features(*args, config=_config(fx), n_feat=n_feat, n_surfel=64,
                                      eps_lift=float(fx["eps_lift"]), want_diag=want_diag)


@pytest.fixture(scope="module")
def runs(fx):
    """One call per case, shared by the comparisons below (host copies)."""
    out = {}
    for case in "AB":
        b = _run(fx, case)
        out[case] = dict(batch={k: getattr(b, k).cpu().numpy() for k in BATCH_F64 + ("sources", "source_indices",
                                                                                     "valid_mask")},
                         diag={k: v.cpu().numpy() for k, v in b.camera_diag.items()}, n_camera_valid=b.n_camera_valid,
                         n_lidar_valid=b.n_lidar_valid, n_feat=b.n_feat, n_surfel=b.n_surfel)
    return out


def _expected_slice(fx, case, n_feat, n_total):
    """The reference's batch arrays for this n_feat (measurement_batch.py:198-259)."""
    n = min(fx["u"].shape[0], n_feat)
    e = dict(Lambdas=np.zeros((n_total, 3, 3)), thetas=np.zeros((n_total, 3)), etas=np.zeros((n_total, 3, 3)),
             weights=np.zeros(n_total), timestamps=np.zeros(n_total), colors=np.zeros((n_total, 3)),
             sources=np.zeros(n_total, np.int32), source_indices=np.zeros(n_total, np.int32),
             valid_mask=np.zeros(n_total, bool))
    e["Lambdas"][:n] = fx[f"{case}_Lambdas"][:n]
    e["thetas"][:n] = fx[f"{case}_thetas"][:n]
    e["etas"][:n, 0] = fx[f"{case}_eta0"][:n]
    e["weights"][:n] = fx[f"{case}_weights"][:n]
    e["timestamps"][:n] = float(fx["timestamp"])
    e["colors"][:n] = fx[f"{case}_colors"][:n]
    e["source_indices"][:n] = np.arange(n)
    e["valid_mask"][:n] = True
    return e, n


def _close(name, got, ref, rtol, atol):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = np.abs(got - ref)
    rel = (err / np.maximum(np.abs(ref), 1e-300)).max() if err.size else 0.0
    print(f"{name}: max abs err {err.max() if err.size else 0.0:.3e}, max rel err {rel:.3e}, max|ref| "
          f"{np.abs(ref).max() if ref.size else 0.0:.3e}")
    bad = ~(err <= atol + rtol * np.abs(ref))
    assert not bad.any(), f"{name}: {bad.sum()} / {bad.size} outside tol; worst {err.max():.3e}"


@pytest.mark.parametrize("case", ["A", "B"])
def test_candidate_counts_are_the_references(fx, runs, case):
    assert np.array_equal(runs[case]["diag"]["n_pt"], fx[f"{case}_n_pt"])


def test_route_a_case_a_bitwise_order_statistics(fx, runs):
    d = runs["A"]["diag"]
    for k in ("z_med", "mad"):   # NaN where Route A does not apply, in both
        ok = np.isfinite(fx[f"A_{k}"])
        assert np.array_equal(np.isfinite(d[k]), ok), k
        assert np.array_equal(d[k][ok].view(np.int64), fx[f"A_{k}"][ok].view(np.int64)), k
    _close("A Lambda_A", d["Lambda_A"], fx["A_Lambda_A"], 1e-9, 0.0)
    _close("A theta_A", d["theta_A"], fx["A_theta_A"], 1e-9, 0.0)


def test_route_a_case_b(fx, runs):
    d = runs["B"]["diag"]
    for k in ("z_med", "mad"):
        ok = np.isfinite(fx[f"B_{k}"])
        assert np.array_equal(np.isfinite(d[k]), ok), k
        _close(f"B {k}", d[k][ok], fx[f"B_{k}"][ok], 1e-9, 1e-12)
    _close("B Lambda_A", d["Lambda_A"], fx["B_Lambda_A"], 1e-9, 1e-12)
    _close("B theta_A", d["theta_A"], fx["B_theta_A"], 1e-9, 1e-12)


@pytest.mark.parametrize("case", ["A", "B"])
def test_route_b_fusion_and_batch_arrays(fx, runs, case):
    r = runs[case]
    d = r["diag"]
    for k in ("Lambda_B", "theta_B", "z_f"):
        ref = fx[f"{case}_{k}"]
        _close(f"{case} {k}", d[k], ref, 1e-7, 1e-7 * np.abs(ref).max())
    assert np.array_equal(d["fused"].astype(bool), fx[f"{case}_fused"])
    e, n = _expected_slice(fx, case, r["n_feat"], r["n_feat"] + r["n_surfel"])
    assert r["n_camera_valid"] == n == 96 and r["n_lidar_valid"] == 0
    for k in BATCH_F64:
        _close(f"{case} {k}", r["batch"][k], e[k], 1e-7, 1e-7 * np.abs(e[k]).max())
    for k in ("valid_mask", "sources", "source_indices"):
        assert np.array_equal(r["batch"][k], e[k]), k
    for k in BATCH_F64:   # padding rows and the untouched LiDAR slice: exact zeros
        assert not r["batch"][k][n:].any(), k


def test_truncation_to_n_feat(fx, runs):
    b = _run(fx, "B", n_feat=64, want_diag=False)
    e, n = _expected_slice(fx, "B", 64, 128)
    assert n == 64 and b.n_camera_valid == 64 and b.n_feat == 64
    for k in BATCH_F64:
        got = getattr(b, k).cpu().numpy()
        _close(f"n_feat=64 {k}", got, e[k], 1e-7, 1e-7 * np.abs(e[k]).max())
        assert np.array_equal(got[:64], runs["B"]["batch"][k][:64]), k   # the first 64 features, same bits
    for k in ("valid_mask", "sources", "source_indices"):
        assert np.array_equal(getattr(b, k).cpu().numpy(), e[k]), k


def test_two_calls_are_bitwise_equal(fx, runs):
    b = _run(fx, "B")
    for k, ref in runs["B"]["batch"].items():
        assert np.array_equal(getattr(b, k).cpu().numpy(), ref, equal_nan=True), k
    for k, ref in runs["B"]["diag"].items():
        assert np.array_equal(b.camera_diag[k].cpu().numpy(), ref, equal_nan=True), k


def test_candidate_overflow_raises_and_writes_nothing_valid(fx):
    dense = np.flatnonzero(fx["A_n_pt"] > 32)
    assert dense.size > 0
    bld = CameraSplatBuilder(_config(fx), n_feat=128, n_surfel=64, max_points=8192, max_candidates=32)
    try:
        with pytest.raises(RuntimeError, match=rf"feature {dense[0]} has more than max_candidates=32"):
            _run(fx, "A", builder=bld)
        # the same builder with room for every feature's candidates runs clean afterwards
        feats = _features(fx)
        sparse = np.flatnonzero(fx["A_n_pt"] <= 32)
        sub = {k: v[sparse] for k, v in feats.items()}
        b = bld.build(sub, fx["A_points_base"].astype(np.float64), PinholeIntrinsics(*fx["intrinsics"]),
                      fx["A_R_base_camera"], fx["A_t_base_camera"], float(fx["timestamp"]), want_diag=True)
        assert b.n_camera_valid == sparse.size
        assert np.array_equal(b.camera_diag["n_pt"].cpu().numpy(), fx["A_n_pt"][sparse])
    finally:
        bld.close()


def test_overflow_leaves_no_valid_row(fx):
    """The failing call's output arrays, read through the C-ABI (the Python wrapper raises before it
    returns a batch): every row invalid and zero, n_camera_valid 0."""
    import ctypes as C
    from gcslam import _lib as L
    from gcslam.surfels import create_empty_measurement_batch
    bld = CameraSplatBuilder(_config(fx), n_feat=128, n_surfel=64, max_points=8192, max_candidates=32)
    try:
        fa = bld.device_features(_features(fx))
        p = torch.as_tensor(fx["A_points_base"].astype(np.float64), device=DEV).contiguous()
        batch = create_empty_measurement_batch(128, 64, DEV)
        batch.valid_mask[:] = True          # stale content the failing call must clear
        batch.weights[:] = 1.0
        i, o = L.GcsCamsplatInputs(), L.GcsCamsplatOutputs()
        i.points_base, i.n_points, i.n_features = p.data_ptr(), p.shape[0], fa["u"].shape[0]
        i.R_base_camera[:], i.t_base_camera[:] = np.eye(3).reshape(9).tolist(), [0.0, 0.0, 0.0]
        i.fx, i.fy, i.cx, i.cy = (float(x) for x in fx["intrinsics"])
        for k, v in fa.items():
            setattr(i, k, v.data_ptr())
        for k in L.CAMSPLAT_BATCH_FIELDS:
            x = getattr(batch, k)
            setattr(o, k, (x.view(torch.uint8) if k == "valid_mask" else x).data_ptr())
        torch.cuda.synchronize()
        rc = bld.lib.gcs_camera_splats(bld.h, C.byref(i), C.byref(o))
        assert rc == -4 and o.n_camera_valid == 0
        assert not batch.valid_mask[:128].any() and not batch.weights[:128].any() and not batch.Lambdas[:128].any()
    finally:
        bld.close()


def test_empty_feature_list_gives_the_empty_batch(fx):
    b = camera_batch_from_features([], fx["A_points_base"].astype(np.float64), PinholeIntrinsics(*fx["intrinsics"]),
                                   np.eye(3), np.zeros(3), 1.0, n_feat=128, n_surfel=64)
    assert (b.n_feat, b.n_surfel, b.n_camera_valid, b.n_lidar_valid) == (128, 64, 0, 0)
    for k in BATCH_F64 + ("sources", "source_indices", "valid_mask"):
        x = getattr(b, k)
        assert x.shape[0] == 192 and not x.any(), k
