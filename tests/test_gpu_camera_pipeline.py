"""Camera splats and LiDAR surfels together through the live primitive path: the fixture's camera
batch (tests/golden/camera_splats.npz, case B: a real camera extrinsic) merged with the surfels of a
synthetic scan by extract_lidar_surfels(base_batch=...), then OT association and visual pose evidence on
the mixed batch against the oracle's operators on the same arrays -- camera rows valid and carrying
responsibility mass -- and process_scan_single_hypothesis(camera_batch=..., camera_batch_policy="use")."""

import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import association as OA, primitive_evidence as OE
from gcslam import association as GA, primitive_map as gpm, synthetic
from gcslam.camera import DepthFusionConfig, PinholeIntrinsics, camera_batch_from_features
from gcslam.surfels import SurfelExtractionConfig, extract_lidar_surfels

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORIGIN = (0.0, 0.0, 0.5)
ARRAYS = ("Lambdas", "thetas", "etas", "weights", "sources", "source_indices", "valid_mask", "timestamps", "colors")
cpu = lambda x: x.detach().cpu().numpy()  # noqa: E731


@pytest.fixture(scope="module")
def camera_batch():
    fx = dict(np.load(os.path.join(ROOT, "tests", "golden", "camera_splats.npz")))
    feats = dict(u=fx["u"], v=fx["v"], depth_Lambda_c=fx["depth_Lambda_c"], depth_theta_c=fx["depth_theta_c"],
                 xyz=fx["xyz_in"], cov=fx["cov_in"], weight=fx["weight"], kappa_app=fx["kappa_app"],
                 mu_app=fx["mu_app"], has_mu=fx["has_mu"], color=fx["color"], has_color=fx["has_color"])
    b = camera_batch_from_features(feats, fx["B_points_base"].astype(np.float64), PinholeIntrinsics(*fx["intrinsics"]),
                                   fx["B_R_base_camera"], fx["B_t_base_camera"], float(fx["timestamp"]),
                                   config=DepthFusionConfig(lidar_projection_radius_pix=float(fx["radius"])))
    assert (b.n_feat, b.n_surfel, b.n_camera_valid) == (512, 1024, 96)
    return b


def _host_batch(batch):
    b = {f: cpu(getattr(batch, f)) for f in ("Lambdas", "thetas", "etas", "weights", "valid_mask", "colors", "sources")}
    b["valid_mask"] = b["valid_mask"].astype(bool)
    b["n_valid"] = batch.n_valid
    return b


def _host_view(view, m_tile_view):
    v = {f: cpu(getattr(view, f)) for f in ("positions", "directions", "kappas", "valid_mask",
                                            "last_supported_scan_seq", "candidate_tile_ids", "candidate_slots",
                                            "tile_ids")}
    v.update(m_tile_view=m_tile_view)
    return v


def _host_assoc(res):
    return {f: cpu(getattr(res, f)) for f in ("responsibilities", "candidate_pool_indices", "row_masses",
                                              "candidate_tile_ids", "candidate_slots")}


def test_mixed_batch_association_and_pose_evidence(camera_batch):
    am = gpm.AtlasMap(m_tile=4096, max_tiles=64, max_merge=0)
    cfg = SurfelExtractionConfig(n_surfel=1024, n_feat=512)
    cam = {f: cpu(getattr(camera_batch, f)) for f in ARRAYS}
    for k in range(2):
        sc = synthetic.make_scan(8192, 40 + k)
        z = np.array([0.1 * k, 0.04 * k, 0.0, 0.0, 0.0, 0.02 * k])
        pts, ts, ws = (torch.as_tensor(sc[f], device=DEV) for f in ("points", "timestamps", "weights"))
        batch, _, _ = extract_lidar_surfels(pts, ts, ws, config=cfg, base_batch=camera_batch)
        # both slices: the camera rows are the input's, the LiDAR rows follow them
        assert batch.n_camera_valid == 96 and batch.n_lidar_valid > 100 and batch.n_valid == 96 + batch.n_lidar_valid
        for f in ARRAYS:
            assert np.array_equal(cpu(getattr(batch, f))[:512], cam[f][:512]), f
        assert cpu(batch.valid_mask)[512:512 + batch.n_lidar_valid].all()
        assert (cpu(batch.sources)[512:512 + batch.n_lidar_valid] == 1).all()
        b = _host_batch(batch)
        active = gpm.ma_hex_stencil_tile_ids(z[:3], 2.0, 1, 1)
        gpm.primitive_map_recency_inflate(am, active, 10 + k)
        view = gpm.extract_atlas_map_view(am, active, 1024)
        acfg = GA.AssociationConfig(scan_seq=10 + k, r_stencil_tiles_z=1)
        res, _, _ = GA.associate_primitives_ot(batch, view, acfg)
        ov = _host_view(view, 1024)
        a_ref, _ = OA.associate_primitives_ot(dict(b), ov, OA.AssociationConfig(scan_seq=10 + k, r_stencil_tiles_z=1))
        assert np.array_equal(cpu(res.candidate_pool_indices), a_ref["candidate_pool_indices"])
        np.testing.assert_allclose(cpu(res.responsibilities), a_ref["responsibilities"], rtol=1e-9, atol=1e-15)
        vis, vcert, _ = GA.visual_pose_evidence(res, batch, view, z_lin_pose=z)
        e_ref = OE.visual_pose_evidence(b, ov, _host_assoc(res), z)
        assert vcert.exact == e_ref["exact"] == (k == 0)     # the first scan meets an empty map
        np.testing.assert_allclose(vis.L_pose, e_ref["L_pose"], rtol=1e-10, atol=1e-10 * np.abs(e_ref["L_pose"]).max())
        if k == 1:   # new ground: camera rows associated with the map the first mixed batch built
            mass = cpu(res.responsibilities)[:96].sum(axis=1)
            print(f"camera rows with responsibility mass: {(mass > 0).sum()} / 96, total {mass.sum():.3e}")
            assert (mass > 0).sum() > 0 and a_ref["responsibilities"][:96].sum() > 0
        gpm.primitive_map_update(am, batch, res, z, active, float(sc["scan_end_time"]), 10 + k)
    am.close()


def test_pipeline_uses_the_camera_batch(camera_batch):
    from gcslam.pipeline import (BeliefGaussianInfo, PipelineConfig, datasheet_process_noise_state,
                                 process_noise_state_to_Q, process_scan_single_hypothesis)
    N, m_tile = 8192, 4096
    cfg = PipelineConfig(K_HYP=1, N_POINTS_CAP=N, B_BINS=48, soft_assign_mode="dense", lidar_origin_base=ORIGIN,
                         max_raw_points=N, primitive_map_max_size=m_tile, R_ACTIVE_TILES_Z=1, R_STENCIL_TILES_Z=1,
                         N_ACTIVE_TILES=21, N_STENCIL_TILES=21, camera_batch_policy="use")
    Q = process_noise_state_to_Q(datasheet_process_noise_state())
    cam = {f: cpu(getattr(camera_batch, f)) for f in ARRAYS}
    # two identical (context, map) pairs take scan 0 with the camera batch; scan 1 then runs with it on
    # one and without it on the other
    ctxs = [cfg.make_context(), cfg.make_context()]
    maps = [gpm.create_empty_atlas_map(m_tile=m_tile, max_tiles=64) for _ in range(2)]
    beliefs = [BeliefGaussianInfo.create_identity_prior() for _ in range(2)]
    results = []
    for scan_seq in range(2):
        sc = synthetic.make_scan(N, 70 + scan_seq)
        kw = dict(raw_points=sc["points"], raw_timestamps=sc["timestamps"], raw_weights=sc["weights"],
                  raw_ring=np.zeros(N, np.uint8), raw_tag=np.zeros(N, np.uint8), imu_stamps=sc["imu_stamps"],
                  imu_gyro=sc["imu_gyro"], imu_accel=sc["imu_accel"], odom_pose=sc["odom_pose"],
                  odom_cov_se3=sc["odom_cov_se3"], scan_start_time=sc["scan_start_time"],
                  scan_end_time=sc["scan_end_time"], dt_sec=sc["dt_sec"], t_last_scan=sc["t_last_scan"],
                  t_scan=sc["t_scan"], Q=Q, config=cfg, odom_twist=sc["odom_twist"],
                  odom_twist_cov=sc["odom_twist_cov"], scan_seq=scan_seq)
        results = [process_scan_single_hypothesis(belief_prev=beliefs[i], primitive_map=maps[i], map_bins=ctxs[i],
                                                  camera_batch=camera_batch if (scan_seq == 0 or i == 0) else None,
                                                  **kw) for i in range(2)]
        beliefs = [r.belief_updated for r in results]
        if scan_seq == 0:
            assert np.array_equal(results[0].z_t, results[1].z_t)
    with_cam, without = results
    mb = with_cam.measurement_batch
    assert mb.n_camera_valid == 96 and mb.n_lidar_valid > 100 and without.measurement_batch.n_camera_valid == 0
    for f in ARRAYS:
        assert np.array_equal(cpu(getattr(mb, f))[:512], cam[f][:512]), f
    resp = cpu(with_cam.association.responsibilities)
    assert (resp[:96].sum(axis=1) > 0).sum() > 0
    # the pose evidence: the oracle's operators on the returned batch and view
    b, ov = _host_batch(mb), _host_view(with_cam.map_view, int(cfg.M_TILE_VIEW))
    ocfg = OA.AssociationConfig(k_assoc=cfg.k_assoc, k_sinkhorn=cfg.k_sinkhorn, epsilon=cfg.ot_epsilon, tau_a=cfg.ot_tau_a,
                                tau_b=cfg.ot_tau_b, eps_mass=cfg.eps_mass, h_tile=cfg.H_TILE, r_stencil_tiles_xy=1,
                                r_stencil_tiles_z=1, scan_seq=1, recency_decay_lambda=cfg.RECENCY_DECAY_LAMBDA)
    a_ref, _ = OA.associate_primitives_ot(dict(b), ov, ocfg)
    assert np.array_equal(cpu(with_cam.association.candidate_pool_indices), a_ref["candidate_pool_indices"])
    np.testing.assert_allclose(resp, a_ref["responsibilities"], rtol=1e-9, atol=1e-15)
    e_ref = OE.visual_pose_evidence(b, ov, _host_assoc(with_cam.association), with_cam.z_lin_pose,
                                    eps_lift=cfg.eps_lift, eps_mass=cfg.eps_mass)
    L_pose = with_cam.visual_pose.L_pose
    np.testing.assert_allclose(L_pose, e_ref["L_pose"], rtol=1e-10, atol=1e-10 * np.abs(e_ref["L_pose"]).max())
    L_lidar, _ = GA.build_visual_pose_evidence_22d(with_cam.visual_pose)
    L_lidar_none, _ = GA.build_visual_pose_evidence_22d(without.visual_pose)
    assert not np.array_equal(np.asarray(L_lidar), np.asarray(L_lidar_none))
    assert not np.array_equal(with_cam.L_evidence, without.L_evidence)
    for m in maps:
        m.close()
    for c in ctxs:
        c.close()


def test_use_policy_without_a_primitive_map_warns_like_warn(camera_batch):
    """The bin path consumes no batch: "use" behaves as "warn" there (one warning per process)."""
    import warnings
    from gcslam import pipeline as P
    N = 2048
    cfg = P.PipelineConfig(K_HYP=1, N_POINTS_CAP=N, B_BINS=48, lidar_origin_base=ORIGIN, max_raw_points=N,
                           camera_batch_policy="use")
    sc = synthetic.make_scan(N, 3)
    Q = P.process_noise_state_to_Q(P.datasheet_process_noise_state())
    P._camera_warned = False
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        r = P.process_scan_single_hypothesis(
            belief_prev=P.BeliefGaussianInfo.create_identity_prior(), raw_points=sc["points"],
            raw_timestamps=sc["timestamps"], raw_weights=sc["weights"], raw_ring=None, raw_tag=None,
            imu_stamps=sc["imu_stamps"], imu_gyro=sc["imu_gyro"], imu_accel=sc["imu_accel"], odom_pose=sc["odom_pose"],
            odom_cov_se3=sc["odom_cov_se3"], scan_start_time=sc["scan_start_time"], scan_end_time=sc["scan_end_time"],
            dt_sec=sc["dt_sec"], t_last_scan=sc["t_last_scan"], t_scan=sc["t_scan"], Q=Q, config=cfg,
            odom_twist=sc["odom_twist"], odom_twist_cov=sc["odom_twist_cov"], camera_batch=camera_batch)
    assert r.measurement_batch is None and any("camera_batch ignored" in str(x.message) for x in w)
