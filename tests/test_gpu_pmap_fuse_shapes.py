"""Step 12b's fuse (fuse_blocks of gcs_pmap.hip: k_ss_block + k_ss_merge or rocPRIM, k_pm_fuse_runs,
k_pm_fuse_apply_blocks) at every row count, sort path and run shape of tests/pmap_shape_util.py's fuse tables,
through primitive_map_update against the numpy oracle (oracle/primitive_map.py) at the suite's step-12b bars:
counts and ids equal, mass statistics at rel 1e-12, tiles at rtol 1e-11.  The two sorts give the same permutation,
so their tiles are compared bitwise; the standalone fuse operator is bitwise against the oracle.

The guards that show a case reaches its branch run without a GPU in tests/test_pmap_shapes.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import pmap_shape_util as U
from oracle import primitive_map as opm
from test_gpu_primitive_map import _same_tile

pytestmark = pytest.mark.gpu


def _check_update(case, am, st):
    d = U.build_fuse_case(case.id)
    tiles, nxt_ref, st_ref = U.fuse_oracle(case.id)
    assert am.next_global_id == nxt_ref
    for k in ("fused_count", "insert_count_total", "evicted_count", "merged_count"):
        assert st[k] == st_ref[k], k
    for k in ("fused_mass_total", "insert_mass_total", "insert_mass_p95", "evicted_mass_total"):
        assert st[k] == pytest.approx(st_ref[k], rel=1e-12, abs=1e-300), k
    for tid in d["active"]:
        _same_tile(am.read_tile(tid), tiles[tid], rtol=1e-11, what=f"{case.id} tile {tid}")
        assert am.counts[tid] == int(tiles[tid]["valid_mask"].sum())


@pytest.mark.parametrize("case", U.FUSE_CASES, ids=[c.id for c in U.FUSE_CASES])
def test_fuse_case_matches_oracle(case):
    am, st = U.fuse_device(case)
    try:
        _check_update(case, am, st)
    finally:
        am.close()


def test_more_than_256_blocks_is_refused():
    """nb = 257 association blocks: an argument error, and no tile is touched."""
    from gcslam import primitive_map as gpm
    case = U.FUSE_REFUSED
    d = U.build_fuse_case(case.id)
    rng = np.random.default_rng(7)
    am = gpm.AtlasMap(m_tile=U.M_FUSE, max_tiles=8, n_lobes=U.NL, max_merge=0)
    try:
        for tid in d["active"]:   # (the call below rewrites the case's own first tile with the same arrays)
            am.write_tile(tid, d["tiles"].get(tid) or U.rand_tile(rng, m=U.M_FUSE, frac=0.5, seq_hi=30))
        before = {tid: am.read_tile(tid) for tid in d["active"]}
        with pytest.raises(ValueError):
            U.fuse_device(case, am)
        for tid in d["active"]:
            _same_tile(am.read_tile(tid), before[tid], what=f"refused: tile {tid}")
        assert am.next_global_id == U.NEXT_ID
    finally:
        am.close()


def test_fuse_sort_paths_give_the_same_bits(tmp_path):
    """k_ss_block + k_ss_merge (default) and rocPRIM's radix sort (GCSLAM_FUSE_SMALLSORT=0, read once per process)
    sort the same distinct (key, row) pairs: every field of every active tile of every fuse case bitwise equal -- a
    mis-sort that stays inside the 1e-11 bar shows here."""
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    out = {}
    for name, env in (("lds", {}), ("rocprim", {"GCSLAM_FUSE_SMALLSORT": "0"})):
        path = str(tmp_path / f"{name}.npz")
        code = ("import sys; sys.path[:0] = [%r, %r, %r]; import pmap_shape_util as U; U.child_fuse_dump(%r)"
                % (here, root, os.path.join(root, "gc-slam_amd"), path))
        e = {k: v for k, v in os.environ.items() if k != "GCSLAM_FUSE_SMALLSORT"}
        r = subprocess.run([sys.executable, "-c", code], env=dict(e, **env), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        out[name] = np.load(path)
    a, b = out["lds"], out["rocprim"]
    assert sorted(a.files) == sorted(b.files) and len(a.files) > 0
    for f in a.files:
        assert np.array_equal(a[f], b[f], equal_nan=True), f


@pytest.mark.parametrize("R", [1, 255, 256, 257, 16384, 16385])
def test_standalone_fuse_then_update(R):
    """primitive_map_fuse_tiles (its own key sort) bitwise against the oracle's fuse, then one step 12b on the same
    map: fuse_impl sized the sort scratch, so fuse_blocks must not take the LDS sort on a scratch too small for
    its runs."""
    from gcslam import primitive_map as gpm
    rng = np.random.default_rng(3000 + R)
    case = U.FUSE_BY_ID["rows1025"]
    d = U.build_fuse_case(case.id)
    act = d["active"]
    m = U.M_FUSE
    tiles = {tid: U.rand_tile(rng, m=m, frac=0.6) for tid in act[:2]}
    am = gpm.AtlasMap(m_tile=m, max_tiles=8, n_lobes=U.NL, max_merge=0)
    try:
        for tid, t in tiles.items():
            am.write_tile(tid, t)
        tile_flat = rng.choice(act[:2] + [U.INACTIVE_ID], size=R)
        slots = rng.integers(0, 300, R)
        Lm = rng.normal(size=(R, 3, 3))
        th, et, w = rng.normal(size=(R, 3)), rng.normal(size=(R, U.NL, 3)), rng.random(R)
        resp, valid = rng.random(R), rng.random(R) < 0.8
        cols, srcs = rng.random((R, 3)) * 1.5 - 0.25, rng.integers(0, 2, R).astype(np.int32)
        fuse_order = [act[1], act[0]]
        res = gpm.primitive_map_fuse_tiles(am, fuse_order, tile_flat, slots, Lm, th, et, w, resp, 9.25, scan_seq=50,
                                           valid_mask=valid, colors_meas=cols, sources_meas=srcs)
        for k, tid in enumerate(fuse_order):
            n = opm.fuse(tiles[tid], slots, Lm, th, et, w, resp, 9.25, scan_seq=50, valid_mask=valid & (tile_flat == tid),
                         colors_meas=cols, sources_meas=srcs)
            assert res[k][0].n_fused == n
            _same_tile(am.read_tile(tid), tiles[tid], what=f"R={R} tile {tid}")      # same sum order: bitwise
        # step 12b on the same map (fuse_device rewrites the case's first tile, the second keeps the fused state)
        from types import SimpleNamespace
        from oracle import se3
        tiles[act[0]] = opm.copy_tile(d["tiles"][act[0]])
        am.write_tile(act[0], tiles[act[0]])
        am.next_global_id = U.NEXT_ID
        Rm, t = se3.so3_exp(U.Z_T[3:]), U.Z_T[:3]
        nxt_ref, st_ref = opm.map_update_step(tiles, U.NEXT_ID, d["batch"], d["assoc"], Rm, t, act, m, U.TS, U.SEQ,
                                              k_insert_tile=U.KINS, h_tile=2.0, block_size=case.B,
                                              merge_max_tile_size=U.MERGE_CAP)
        cfg = gpm.PrimitiveMapUpdateConfig(k_insert_tile=U.KINS, block_size=case.B,
                                           primitive_merge_max_tile_size=U.MERGE_CAP)
        st = gpm.primitive_map_update(am, SimpleNamespace(**d["batch"]), SimpleNamespace(**d["assoc"]), U.Z_T, act,
                                      U.TS, U.SEQ, cfg)
        assert am.next_global_id == nxt_ref
        for k in ("fused_count", "insert_count_total", "evicted_count", "merged_count"):
            assert st[k] == st_ref[k], k
        for k in ("fused_mass_total", "insert_mass_total", "insert_mass_p95", "evicted_mass_total"):
            assert st[k] == pytest.approx(st_ref[k], rel=1e-12, abs=1e-300), k
        for tid in act:
            _same_tile(am.read_tile(tid), tiles[tid], rtol=1e-11, what=f"R={R} update tile {tid}")
            assert am.counts[tid] == int(tiles[tid]["valid_mask"].sum())
    finally:
        am.close()
