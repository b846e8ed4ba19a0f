"""OT association on the GPU at every shape-dependent path of assoc_launch (gcs_assoc.hip:2386-2555):
the three template widths KM = 8, 16, 32 with k_assoc below and at the width, the row counts where the
Sinkhorn's rows-per-thread form changes and where the row capacity is met, view strides that are no
power of two, views past the prep's LDS tile table and past the bucket table, a stencil too large for
LDS, rows short of valid candidates, and rows whose stencil meets no tile of the view.

Every case compares gcslam.association.associate_primitives_ot with the numpy oracle
(oracle/association.py) at test_gpu_association._check's bars.  Before comparing, each case asserts on
the oracle's own output that the scene reaches the branch it is there for (the library's constants are
restated below with their source lines), and that no valid row has two different pool costs among its
K + 1 cheapest closer than 1e-9 relative: bit-exact candidates need the costs apart; exact ties
(invalid entries at 1e12, repeated pool entries, the stray rows) are decided by pool position on both
sides and must match."""
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from assoc_util import make_scene
from oracle import association as OA
from gcslam import association as GA
from test_gpu_association import _batch, _check, _run_both, _view

pytestmark = pytest.mark.gpu

# the library's constants the cases' guards depend on
ROW_SLOTS = 16 * 1024        # kShCR * kShThreads, gcs_assoc.hip:47 (row capacity ROW_SLOTS // KM, :2257)
SH_THREADS_X3 = 3 * 512      # k_as_sinkhorn<8, 3> serves n <= 3 * kShThreads, gcs_assoc.hip:46, :2534
POOL_LDS_MAX_VIEW = 9216     # kPoolLdsMaxView, gcs_assoc.hip:567: lds_slots = 0 past it (:2509)
LDS_TILES = 256              # kLdsTiles, gcs_assoc.hip:264 (k_as_prep's tile table) = kFusedTiles, :697
MAX_BUCKETS = 4096           # kMaxBuckets, gcs_assoc.hip:568: n_tiles + 1 > 4096 leaves the bucketed pool (:2462)
TIE_GAP = 1e-9               # smallest relative gap between different pool costs a case may hold

SMALL = dict(n_feat=64, n_surfel=128, n_valid_cam=40, n_valid_lidar=100, m_tile=64, m_tile_view=64, fill=(0, 50))
RAGGED = dict(SMALL, n_feat=37, n_surfel=61, n_valid_cam=20, n_valid_lidar=33)
ROWS2048 = dict(n_feat=512, n_surfel=1536, n_valid_cam=400, n_valid_lidar=1300, m_tile=128, m_tile_view=128,
                fill=(0, 100))
STRAY_ROWS = (0, 7, 37, 50)  # valid rows of the ragged scene (camera 0..19, LiDAR 37..69)
STRAY_MU = ((500.0, 300.0, 0.5), (-700.0, -20.0, 0.5), (3.0, 3.0, 90.0), (-1e4, 1e4, -1e3))
ZERO_WEIGHT_ROWS = (0, 5, 64, 70)  # valid rows of the small scene (camera 0..39, LiDAR 64..163)


def _km(k):
    return 8 if k <= 8 else (16 if k <= 16 else 32)


def _case(name):
    """(scene kwargs, config kwargs, guard) of a case id; guard(info) asserts the case's condition on
    the oracle's output (info: N, K, n_tiles, S stencil tiles, ref, rc, batch, nvc = per valid row its
    selected candidates whose view entry is valid, the count of candidate_stats)."""
    none = lambda i: True  # noqa: E731
    short = lambda i: (i["nvc"] < i["K"]).any()  # noqa: E731
    if name[0] == "k" and name[1:].isdigit():
        k = int(name[1:])
        guard = (lambda i: short(i)) if k >= 17 else none
        return dict(SMALL, seed=11), dict(k_assoc=k), guard
    if name in ("rows2048", "rows1537"):
        n = int(name[4:])
        sc = dict(ROWS2048, seed=12, n_surfel=n - 512, n_valid_lidar=1300 if n == 2048 else 900)
        return sc, {}, lambda i: i["N"] == n and n > SH_THREADS_X3 and n <= ROW_SLOTS // 8
    if name in ("cap16", "cap32"):
        k = int(name[3:])
        n = ROW_SLOTS // k
        sc = dict(SMALL, seed=22, n_feat=n // 4, n_surfel=n - n // 4, n_valid_cam=n // 5, n_valid_lidar=n // 2)
        return sc, dict(k_assoc=k), lambda i: i["N"] == ROW_SLOTS // _km(i["K"])
    if name == "ragged":
        return dict(RAGGED, seed=13), {}, lambda i: i["N"] == 98
    if name == "one_row":
        sc = dict(SMALL, seed=23, n_feat=1, n_surfel=0, n_valid_cam=1, n_valid_lidar=0)
        return sc, {}, lambda i: i["N"] == 1 and not i["rc"]["exact"]
    if name in ("odd_median", "even_median"):
        k = 7 if name == "odd_median" else 8
        sc = dict(RAGGED, seed=24, n_surfel=60)
        cfg = dict(k_assoc=k, cost_scale_by_median=True, cost_subtract_row_min=False)
        return sc, cfg, lambda i: i["N"] == 97 and (i["N"] * i["K"]) % 2 == (1 if name == "odd_median" else 0)
    if name == "m100":
        return dict(SMALL, seed=14, m_tile=100, m_tile_view=100, fill=(0, 80)), {}, none
    if name == "m_lt_k":
        return dict(SMALL, seed=15, m_tile=4, m_tile_view=4, fill=(0, 4)), {}, short
    if name == "sparse_map":
        return dict(SMALL, seed=16, fill=(0, 2)), {}, lambda i: i["nvc"].min() >= 1 and i["nvc"].max() <= i["K"] - 1
    if name == "tiles290":
        sc = dict(SMALL, seed=17, m_tile=8, m_tile_view=8, fill=(0, 8), tile_span=8)
        return sc, {}, lambda i: i["n_tiles"] > LDS_TILES
    if name in ("tiles257", "tiles256"):
        n = int(name[5:])
        sc = dict(SMALL, seed=17, m_tile=8, m_tile_view=8, fill=(0, 8), tile_span=7, missing_tiles=n - 225)
        return sc, {}, lambda i: i["n_tiles"] == n and (n > LDS_TILES) == (name == "tiles257")
    if name == "tiles4226":
        sc = dict(seed=18, n_feat=32, n_surfel=64, n_valid_cam=20, n_valid_lidar=40, m_tile=2, m_tile_view=2,
                  fill=(0, 2), tile_span=32)
        return sc, {}, lambda i: i["n_tiles"] + 1 > MAX_BUCKETS
    if name == "one_tile":
        return dict(SMALL, seed=26, tile_span=0, missing_tiles=0), {}, lambda i: i["n_tiles"] == 1
    if name == "stream_k8":
        sc = dict(SMALL, seed=19, m_tile=512, m_tile_view=512, fill=(0, 300))
        return sc, dict(r_stencil_tiles_z=1), lambda i: i["S"] == 21 and i["S"] * 512 > POOL_LDS_MAX_VIEW
    if name in ("lobes1", "lobes2"):
        n = int(name[5:])
        return dict(SMALL, seed=20, n_lobes=n), {}, lambda i: i["batch"]["etas"].shape == (i["N"], n, 3)
    if name in ("iters0", "iters1"):
        return dict(SMALL, seed=21), dict(k_sinkhorn=int(name[5:])), none
    if name == "zero_weight":
        return dict(SMALL, seed=25), dict(a_policy="weight_proportional"), none
    if name in ("stray_rows_k5", "stray_rows_k8"):
        k = int(name[12:])
        stray = lambda i: np.array_equal(i["ref"]["candidate_pool_indices"][list(STRAY_ROWS)],  # noqa: E731
                                         np.tile(np.arange(k, dtype=np.int32), (len(STRAY_ROWS), 1)))
        return dict(RAGGED, seed=31), dict(k_assoc=k), stray
    raise KeyError(name)


def _scene(name):
    sc, ck, guard = _case(name)
    batch, view, _ = make_scene(**sc)
    if name == "zero_weight":
        assert batch["valid_mask"][list(ZERO_WEIGHT_ROWS)].all()
        batch["weights"][list(ZERO_WEIGHT_ROWS)] = 0.0
    if name.startswith("stray_rows"):
        assert batch["valid_mask"][list(STRAY_ROWS)].all()
        for r, mu in zip(STRAY_ROWS, STRAY_MU):
            batch["thetas"][r] = batch["Lambdas"][r] @ np.array(mu)
    return batch, view, OA.AssociationConfig(scan_seq=10, **ck), guard


def _tie_gap(dbg, valid, K):
    """Smallest relative gap between different neighbouring costs among each valid row's K + 1 cheapest
    pool entries (equal costs -- the invalid cost, repeated entries -- are ties by pool position)."""
    c = np.take_along_axis(dbg["cost_pool"], dbg["order"][:, :K + 1], axis=1)[valid]
    a, b = c[:, :-1], c[:, 1:]
    d = np.where(b != a, (b - a) / np.maximum(np.abs(b), 1e-300), np.inf)
    return float(d.min()) if d.size else np.inf


def _run_case(name):
    batch, view, cfg, guard = _scene(name)
    dbg = {}
    ref, rc, res, cert, eff = _run_both(batch, view, cfg, debug=dbg)
    valid = np.asarray(batch["valid_mask"]).astype(bool)
    K = int(cfg.k_assoc)
    info = dict(N=valid.shape[0], K=K, n_tiles=len(view["tile_ids"]), S=len(OA.stencil(cfg)), ref=ref, rc=rc,
                batch=batch, nvc=np.asarray(view["valid_mask"])[ref["candidate_pool_indices"]].sum(axis=1)[valid])
    assert bool(guard(info)), (name, "the scene no longer reaches its branch")
    gap = _tie_gap(dbg, valid, K)
    assert gap > TIE_GAP, (name, gap)
    _check(ref, rc, res, cert, eff, batch["valid_mask"])
    g = lambda x: x.cpu().numpy()  # noqa: E731
    if name == "zero_weight":
        rows = list(ZERO_WEIGHT_ROWS)
        assert np.all(ref["responsibilities"][rows] == 0.0) and np.all(g(res.responsibilities)[rows] == 0.0)
        assert np.all(g(res.row_masses)[rows] == 0.0)
    if name.startswith("stray_rows"):
        # the stray rows' costs (~1e8) set _check's atol: the ordinary rows again, at their own scale
        rows = np.setdiff1d(np.arange(valid.shape[0]), STRAY_ROWS)
        Cr, Rr, Mr = ref["cost_matrix"][rows], ref["responsibilities"][rows], ref["row_masses"][rows]
        np.testing.assert_allclose(g(res.cost_matrix)[rows], Cr, rtol=1e-12, atol=1e-12 * np.abs(Cr).max())
        np.testing.assert_allclose(g(res.responsibilities)[rows], Rr, rtol=1e-9, atol=1e-12 * np.abs(Rr).max())
        np.testing.assert_allclose(g(res.row_masses)[rows], Mr, rtol=1e-9, atol=1e-12 * np.abs(Mr).max())
    return batch, view, res


CASES = (["k%d" % k for k in (1, 3, 5, 7, 8, 9, 12, 17, 24, 32)] +
         ["rows2048", "rows1537", "cap16", "cap32", "ragged", "one_row", "odd_median", "even_median", "m100",
          "m_lt_k", "sparse_map", "tiles290", "tiles257", "tiles256", "tiles4226", "one_tile", "stream_k8",
          "lobes1", "lobes2", "iters0", "iters1", "zero_weight", "stray_rows_k5", "stray_rows_k8"])


@pytest.mark.parametrize("name", CASES)
def test_association_shape_case(name):
    _run_case(name)


def test_row_capacity_is_a_value_error_naming_the_limit():
    """One row past the capacity of each width is refused by the host's argument check (nothing is
    launched), and the process then runs the small case at k_assoc = 8 correctly."""
    for k, n in ((8, 2049), (16, 1025), (32, 513)):
        assert n == ROW_SLOTS // _km(k) + 1
        batch, view, _ = make_scene(seed=27, n_feat=1, n_surfel=n - 1, n_valid_cam=1, n_valid_lidar=8, m_tile=8,
                                    m_tile_view=8, tile_span=1, fill=(2, 8))
        with pytest.raises(ValueError, match=r"\b%d\b" % (n - 1)):
            GA.associate_primitives_ot(_batch(batch), _view(view), GA.AssociationConfig(k_assoc=k))
    _run_case("k8")


def test_k32_runs_through_the_default_associator():
    """associate_primitives_ot(k_assoc = 17..32) used to fail in gcs_assoc_ctx_create: the default
    context asked for 1,024 rows where the KM = 32 width holds 512."""
    GA._associators.pop(0, None)
    _run_case("k32")
    assert GA._associators[0].max_k == 32 and GA._associators[0].max_meas == ROW_SLOTS // 32


SHAPE_PATH_CASES = ("k5", "k12", "k32", "rows2048", "sparse_map", "m_lt_k", "tiles290", "odd_median")


def _shape_paths_check():
    """Run in a subprocess with one of the association's A/B knobs set (read once per context)."""
    for name in SHAPE_PATH_CASES:
        _run_case(name)


@pytest.mark.parametrize("env", [{"GCSLAM_POOL_LDS": "0"}, {"GCSLAM_SH_FINSPLIT": "0"}, {"GCSLAM_SH_FINSPLIT": "2"},
                                 {"GCSLAM_PREP_FUSED": "1"}],
                         ids=["pool_l2", "finish_in_wg0", "finish_own_launch", "prep_stage_one_launch"])
def test_association_shape_knob_paths_match_oracle(env):
    """The selectable forms (test_association_knob_paths_match_oracle) at the shapes above: the pool
    from L2 at every width, both other finish forms past the three-row Sinkhorn, the one-launch prep
    with short rows and with a view too large for it."""
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    code = ("import sys; sys.path[:0] = [%r, %r, %r]; import test_gpu_association_shapes as t; t._shape_paths_check()"
            % (here, root, os.path.join(root, "gc-slam_amd")))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True,
                       timeout=110)
    assert r.returncode == 0, r.stderr[-3000:]
