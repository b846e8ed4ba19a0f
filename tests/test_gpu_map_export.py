"""GPU tests of map publishing and the splat export (gcs_pmap_export through gcslam.map_export) on seeded
tiles, against tests/map_export_ref.py (the numpy restatement of the reference's publisher and export loop,
pinned by tests/test_map_export_host.py).

Bars: row counts, per-tile counts, source tile ids and slots and the published order equal; copied fields
bit for bit; positions / covariances at test_view_matches_oracle's bars (rtol 1e-12, atol 1e-12 / 1e-13);
kappa / directions at rtol 1e-15, atol 0 / 1e-16 (same sum order, no FMA); the computed rows bitwise equal
to extract_atlas_map_view's of the same slots (the same device arithmetic); Lambda_world against
np.linalg.inv of the device's own Sigma + eps I within the forward-error bound of an LU inverse,
64 cond2(Sigma) 2.2e-16 max|Lambda| per row; x, y, z bytes the float32 of the device's own float64 positions;
intensity bytes the restatement's (NaN rows by isnan)."""

import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import map_export_ref as R

pytestmark = pytest.mark.gpu

NL = 3
EPS_LIFT = 1e-9
COPIED = ("weights", "primitive_ids", "last_supported_scan_seq", "etas", "colors")
SLOT_LOCAL = ("timestamps", "created_timestamps", "cam_mass", "lidar_mass", "rgb_cam_accum", "rgb_cam_denom")

# sizes at which sort_tiles (gcs_pmap.hip) picks another selection kernel for max_primitives = k on a tile of M slots
K_SEL_MAX = 1024          # kSelMax: k above it takes the full radix sort of the tile, not a select
M_REG_SELECT = 8192       # 8 kPmRed: up to here k_pm_select_reg; above, the tree of sorted runs (k_pm_topk)
N_SPARSE_MAX = 2048       # kSpMax: above M_REG_SELECT, a tile with at most this many valid slots is k_pm_topk_sparse's
M_SPARSE_MAX = 65536      # 32 kSpWords: above it no bitmap pass, the tree alone
M_TREE_MAX = 524288       # kTopChunk << (kTopMaxLevels - 1): above it k_pm_select (the one-workgroup radix select)
# the recency order is rocprim::radix_sort_pairs on u64 keys at every size (the path sort_tiles' full sort takes;
# k_ss_block / k_ss_merge take 32-bit keys); rocPRIM itself sorts up to 1,024 rows in one block, up to 2^20 by
# merge sort and more by radix passes
ROCPRIM_BLOCK_SORT = 1024
ROCPRIM_MERGE_SORT = 1 << 20


def cpu(x):
    return x.detach().cpu().numpy()


def _rand_tile(rng, m, frac=0.6, seq_hi=40):
    """tests/test_gpu_primitive_map.py's seeded tile."""
    t = R.create_empty_tile(m)
    v = rng.random(m) < frac
    t["valid_mask"][:] = v
    w = rng.random(m) * 2.0
    w[rng.random(m) < 0.1] = 0.5          # exact ties (stable order by slot)
    w[rng.random(m) < 0.05] = 0.0
    t["weights"][:] = w
    A = rng.normal(size=(m, 3, 3)) * 0.3
    t["Lambdas"][:] = np.einsum("nij,nkj->nik", A, A) + np.eye(3)[None] * rng.uniform(0.5, 4.0, size=(m, 1, 1))
    t["thetas"][:] = rng.normal(size=(m, 3)) * 3.0
    t["etas"][:] = rng.normal(size=(m, NL, 3))
    t["timestamps"][:] = rng.uniform(0, 10, m)
    t["created_timestamps"][:] = rng.uniform(0, 10, m)
    t["last_supported_scan_seq"][:] = rng.integers(0, seq_hi, m)
    t["last_update_scan_seq"][:] = rng.integers(0, seq_hi, m)
    t["primitive_ids"][:] = rng.permutation(10 * m)[:m]
    t["colors"][:] = rng.random((m, 3))
    cam = np.where(rng.random(m) < 0.3, rng.random(m), 0.0)
    t["cam_mass"][:] = cam
    t["lidar_mass"][:] = rng.random(m)
    t["rgb_cam_accum"][:] = rng.random((m, 3)) * cam[:, None]
    t["rgb_cam_denom"][:] = cam
    t["rgb"][:] = np.where((cam > 0)[:, None], rng.random((m, 3)), 0.5)
    return t


def _tile_with_count(rng, m, count):
    """An empty tile of m slots with exactly `count` seeded primitives at random slots (large tiles stay
    cheap to build: only the filled slots are drawn)."""
    t = R.create_empty_tile(m)
    s = np.sort(rng.choice(m, size=count, replace=False))
    d = _rand_tile(rng, count, frac=1.0)
    for f, a in d.items():
        t[f][s] = a
    return t


def _map(tiles, m, max_tiles=8):
    from gcslam.primitive_map import AtlasMap
    am = AtlasMap(m_tile=m, max_tiles=max_tiles, n_lobes=NL, max_merge=0)
    for tid, t in tiles.items():
        am.write_tile(tid, t)
    return am


def _gather(tiles, tids, slots, f):
    any_tile = next(iter(tiles.values()))
    out = np.zeros((len(tids),) + any_tile[f].shape[1:], any_tile[f].dtype)
    for tid in np.unique(tids):
        k = tids == tid
        out[k] = tiles[int(tid)][f][slots[k]]
    return out


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert a.tobytes() == b.tobytes(), what


def _check_lambda_world(g, eps_lift):
    S, Lw = g["covariances"], g["lambda_world"]
    if not len(S):
        return
    ref = np.linalg.inv(S + eps_lift * np.eye(3)[None])
    bar = 64.0 * np.linalg.cond(S) * 2.2e-16 * np.abs(ref).reshape(len(S), -1).max(axis=1)
    err = np.abs(Lw - ref).reshape(len(S), -1).max(axis=1)
    assert (err <= bar).all(), f"Lambda_world: worst err / bar {np.max(err / bar)}"


def _check_points(g, ref):
    pts = g["points"]
    assert pts.dtype == np.float32 and pts.shape == (len(g["positions"]), 4)
    with np.errstate(over="ignore"):
        _same_bits(pts[:, :3], g["positions"].astype(np.float32), "x, y, z bytes")
    want = np.frombuffer(ref["data"], "<f4").reshape(-1, 4)[:, 3]
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(pts[:, 3]), nan)
    _same_bits(pts[~nan, 3], want[~nan], "intensity bytes")


def _check_against_view(am, ids, g):
    """The rows the fixed-size association view computes for the same slots: bitwise."""
    from gcslam.primitive_map import extract_atlas_map_view
    M = am.m_tile
    v = extract_atlas_map_view(am, list(ids), M, EPS_LIFT)
    vs = cpu(v.candidate_slots).reshape(len(ids), M)
    first = {}
    for t, tid in enumerate(ids):
        first.setdefault(int(tid), t)
    row = np.empty(len(g["slots"]), np.int64)
    for tid in np.unique(g["tile_ids"]):
        t = first[int(tid)]
        inv = np.empty(M, np.int64)
        inv[vs[t]] = np.arange(M)
        k = g["tile_ids"] == tid
        row[k] = t * M + inv[g["slots"][k]]
    assert cpu(v.valid_mask)[row].all()
    for f in ("positions", "covariances", "directions", "kappas") + COPIED:
        _same_bits(cpu(getattr(v, f))[row], g[f], f"view {f}")


def _check(am, tiles, ids, maxp=None, order=1, view=True, eps_lift=EPS_LIFT):
    from gcslam import map_export as ME
    r = ME.export_rows(am, ids, maxp, order, eps_lift)
    ref = R.publish(tiles, ids, maxp, eps_lift, order=bool(order))
    g = {k: cpu(x) for k, x in r.rows.items()}
    ids_l = sorted(tiles) if ids is None else list(ids)
    assert r.n_rows == ref["n"] and r.tile_ids == [int(t) for t in ids_l]
    assert np.array_equal(r.tile_rows, ref["tile_rows"])
    for f in ME.ROW_FIELDS:
        assert len(g[f]) == ref["n"], f
    assert np.array_equal(g["tile_ids"], ref["tile_ids"]) and np.array_equal(g["slots"], ref["slots"])
    assert g["slots"].dtype == np.int32 and g["tile_ids"].dtype == np.int64
    for f in COPIED:
        _same_bits(g[f], ref[f], f)
    for f in SLOT_LOCAL:
        _same_bits(g[f], _gather(tiles, ref["tile_ids"], ref["slots"], f), f)
    np.testing.assert_allclose(g["positions"], ref["positions"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(g["covariances"], ref["covariances"], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(g["kappas"], ref["kappas"], rtol=1e-15, atol=0)
    np.testing.assert_allclose(g["directions"], ref["directions"], rtol=1e-15, atol=1e-16)
    _check_lambda_world(g, eps_lift)
    _check_points(g, ref)
    if view and ref["n"]:
        _check_against_view(am, ids_l, g)
    return g, ref


# ---------------------------------------------------------------------- tile sizes, occupancy, tile lists
@pytest.mark.parametrize("m", [1, 192, 4096])      # one slot; three waves, not a multiple of the block; four blocks
def test_tile_sizes_and_occupancies(m):
    rng = np.random.default_rng(100 + m)
    one = _rand_tile(rng, m, frac=1.0)
    one["valid_mask"][:] = False
    one["valid_mask"][m // 2] = True
    tiles = {3: _rand_tile(rng, m, frac=0.0), 4: one, 5: _rand_tile(rng, m, frac=1.0), 6: _rand_tile(rng, m, frac=0.6)}
    if m == 1:
        tiles[6]["valid_mask"][:] = True
    am = _map(tiles, m)
    for order in (0, 1):
        for tid in tiles:
            g, ref = _check(am, tiles, [tid], None, order)
            assert ref["n"] == int(tiles[tid]["valid_mask"].sum())
        _check(am, tiles, None, None, order)           # every tile, sorted ids
    am.close()


def test_tile_lists():
    m = 192
    rng = np.random.default_rng(7)
    tiles = {10 + k: _rand_tile(rng, m, frac=f) for k, f in enumerate((0.6, 0.3, 1.0, 0.0, 0.9, 0.5, 0.6))}
    am = _map(tiles, m, max_tiles=16)
    lists = ([12], [16, 10], [16, 15, 14, 13, 12, 11, 10],
             [11, 999, 12],                 # an id the map lacks, in the middle: skipped, not viewed as empty
             [999],
             [12, 10, 12],                  # an id twice: its rows twice
             [10, 10])
    for ids in lists:
        for order in (0, 1):
            g, ref = _check(am, tiles, ids, None, order)
    g, ref = _check(am, tiles, [12, 10, 12], None, 0)
    assert ref["tile_rows"].tolist() == [192, int(tiles[10]["valid_mask"].sum()), 192]
    assert np.array_equal(g["slots"][:192], g["slots"][-192:])
    am.close()


def test_65_tiles_take_the_offset_prefix_past_one_wave():
    m = 64
    rng = np.random.default_rng(65)
    tiles = {100 + k: _rand_tile(rng, m, frac=rng.uniform(0.0, 1.0)) for k in range(65)}
    am = _map(tiles, m, max_tiles=65)
    ids = [100 + k for k in rng.permutation(65)]
    for order in (0, 1):
        g, ref = _check(am, tiles, ids, None, order)
        _check(am, tiles, ids, 20, order)
    assert (ref["tile_rows"] > 0).sum() > 60
    am.close()


# ---------------------------------------------------------------------- max_primitives
def test_max_primitives_against_count():
    m = 4096
    rng = np.random.default_rng(11)
    t = _rand_tile(rng, m)
    z = np.nonzero(t["weights"] == 0.0)[0]
    t["weights"][z[::2]] = -0.0                   # +-0.0 share the lowest place: the cut at count - 1 is among them
    tiles = {1: t, 2: _rand_tile(rng, m, frac=0.2)}
    am = _map(tiles, m)
    v, w = t["valid_mask"], t["weights"]
    count = int(v.sum())
    n_zero, above_half, at_half = int((v & (w == 0.0)).sum()), int((v & (w > 0.5)).sum()), int((v & (w == 0.5)).sum())
    assert n_zero >= 4 and at_half >= 4 and count > K_SEL_MAX + 1
    cuts = [count,                      # equal to count: the slot-order path
            count - 1,                  # the downselect path, the cut inside the +-0.0 ties
            above_half + at_half // 2,  # the cut inside the 0.5 ties: the lower slots stay
            1, m + 1,                   # one row; above m_tile
            K_SEL_MAX, K_SEL_MAX + 1]   # the select kernel's last size, the full sort's first
    for maxp in cuts:
        for order in (0, 1):
            g, ref = _check(am, tiles, [1], maxp, order)
            assert ref["n"] == min(maxp, count)
    g, ref = _check(am, tiles, [1], count, 0)
    assert np.array_equal(g["slots"], np.nonzero(v)[0])
    g, ref = _check(am, tiles, [1], count - 1, 0)
    assert (np.diff(g["weights"]) <= 0).all() and np.signbit(g["weights"]).any() and g["weights"][-1] == 0.0
    # two tiles, one over max_primitives and one within it, in one call
    c2 = int(tiles[2]["valid_mask"].sum())
    g, ref = _check(am, tiles, [2, 1], c2, 1)
    assert ref["tile_rows"].tolist() == [c2, c2]
    assert _check(am, tiles, [1, 2], 0, 1)[1]["n"] == 0
    am.close()


@pytest.mark.parametrize("m,count", [
    (M_REG_SELECT, 300), (M_REG_SELECT + 1, 300),                   # k_pm_select_reg | k_pm_topk_sparse
    (M_REG_SELECT + 1, N_SPARSE_MAX), (M_REG_SELECT + 1, N_SPARSE_MAX + 1),   # k_pm_topk_sparse | k_pm_topk
    (M_SPARSE_MAX, 300), (M_SPARSE_MAX + 1, 300),                   # bitmap pass | the tree alone
    (M_TREE_MAX, 300), (M_TREE_MAX + 1, 300)])                      # k_pm_topk | k_pm_select
def test_max_primitives_at_the_selection_switch_sizes(m, count):
    rng = np.random.default_rng(m + count)
    tiles = {8: _tile_with_count(rng, m, count)}
    am = _map(tiles, m, max_tiles=1)
    for maxp in (100, count - 1):
        g, ref = _check(am, tiles, [8], maxp, 1, view=m <= M_SPARSE_MAX + 1)
        assert ref["n"] == maxp
    _check(am, tiles, [8], count, 0, view=False)
    am.close()


# ---------------------------------------------------------------------- the recency order
def test_recency_order_keys():
    m = 192
    rng = np.random.default_rng(21)
    a, b = _rand_tile(rng, m, frac=0.8), _rand_tile(rng, m, frac=0.8)
    big = 1 << 32
    for t in (a, b):
        # few distinct recencies (ties broken by id), negative ones, ones above 2^32 and near the int64 ends
        t["last_supported_scan_seq"][:] = rng.choice(
            np.array([-big - 3, -7, -1, 0, 1, 5, big - 1, big, big + 9, (1 << 62) + 1, -(1 << 63) + 1], np.int64), m)
        t["primitive_ids"][:] = rng.choice(
            np.array([-big - 1, -2, 0, 3, big - 1, big + 2, (1 << 63) - 3, -(1 << 63)], np.int64), m) + rng.integers(0, 3, m)
    b["primitive_ids"][: m // 2] = a["primitive_ids"][: m // 2]     # (recency, id) pairs repeated across tiles
    b["last_supported_scan_seq"][: m // 2] = a["last_supported_scan_seq"][: m // 2]
    tiles = {1: a, 2: b}
    am = _map(tiles, m)
    for ids in ([1, 2], [2, 1, 2]):       # a tile twice: every (recency, id) pair of it twice, list order kept
        g, ref = _check(am, tiles, ids, None, 1)
        key = np.stack([-g["last_supported_scan_seq"], g["primitive_ids"]], axis=1)
        assert (np.diff(g["last_supported_scan_seq"]) <= 0).all()
        assert len(np.unique(key, axis=0)) < len(key)               # equal pairs are present
        assert (g["last_supported_scan_seq"] > big).any() and (g["last_supported_scan_seq"] < 0).any()
        assert (g["primitive_ids"] > big).any() and (g["primitive_ids"] < -big).any()
    am.close()


@pytest.mark.parametrize("total", [1, 2, ROCPRIM_BLOCK_SORT, ROCPRIM_BLOCK_SORT + 1])
def test_recency_order_sizes(total):
    m = 600
    rng = np.random.default_rng(total)
    tiles = {1: _tile_with_count(rng, m, min(total, m)), 2: _tile_with_count(rng, m, max(total - m, 0))}
    am = _map(tiles, m)
    g, ref = _check(am, tiles, [2, 1], None, 1)
    assert ref["n"] == total
    am.close()


@pytest.mark.parametrize("extra", [0, 1])    # 2^20 rows: rocPRIM's merge sort; one more: its radix passes
def test_recency_order_past_the_merge_sort(extra):
    from gcslam import map_export as ME
    from gcslam.primitive_map import AtlasMap
    m = (ROCPRIM_MERGE_SORT >> 2) + 1
    rng = np.random.default_rng(5 + extra)
    am = AtlasMap(m_tile=m, max_tiles=4, n_lobes=NL, max_merge=0)
    tiles = {}
    for tid in range(4):
        t = dict(valid_mask=np.ones(m, bool), primitive_ids=rng.integers(-(1 << 40), 1 << 40, m),
                 last_supported_scan_seq=rng.integers(-50, 50, m))
        t["valid_mask"][-1] = bool(extra) and tid == 3
        am.write_tile(tid, t)               # the other fields stay as the empty tile has them
        tiles[tid] = t
    ids = [2, 0, 3, 1]
    r = ME.export_rows(am, ids, None, 1, fields=("primitive_ids", "last_supported_scan_seq", "tile_ids", "slots"))
    assert r.n_rows == ROCPRIM_MERGE_SORT + extra
    cat = {f: np.concatenate([tiles[t][f][tiles[t]["valid_mask"]] for t in ids])
           for f in ("primitive_ids", "last_supported_scan_seq")}
    cat["tile_ids"] = np.concatenate([np.full(int(tiles[t]["valid_mask"].sum()), t, np.int64) for t in ids])
    cat["slots"] = np.concatenate([np.nonzero(tiles[t]["valid_mask"])[0] for t in ids]).astype(np.int32)
    o = R.lexsort_order(cat["primitive_ids"], cat["last_supported_scan_seq"])
    for f, x in cat.items():
        assert np.array_equal(cpu(r.rows[f]), x[o]), f
    am.close()


def test_int64_min_recency_is_refused():
    from gcslam import map_export as ME
    m = 192
    rng = np.random.default_rng(3)
    t = _rand_tile(rng, m, frac=1.0)
    t["last_supported_scan_seq"][77] = np.iinfo(np.int64).min
    tiles = {1: t, 2: _rand_tile(rng, m)}
    am = _map(tiles, m)
    with pytest.raises(ValueError, match="INT64_MIN"):
        ME.publish_map(am, [2, 1])
    _check(am, tiles, [2], None, 1)                  # the other tile alone publishes
    _check(am, tiles, [2, 1], None, 0, view=False)   # concatenation order negates nothing
    t["valid_mask"][77] = False                      # an empty slot's recency is never read
    am.write_tile(1, t)
    _check(am, tiles, [2, 1], None, 1)
    am.close()


# ---------------------------------------------------------------------- totals, capacity
def test_zero_rows():
    from gcslam import map_export as ME
    m = 192
    tiles = {1: R.create_empty_tile(m)}
    am = _map(tiles, m)
    for ids in ([1], [999], [], None):
        r = ME.export_rows(am, ids, None, 1)
        assert r.n_rows == 0 and all(tuple(x.shape[:1]) == (0,) for x in r.rows.values())
        assert tuple(r.rows["etas"].shape) == (0, NL, 3) and tuple(r.rows["points"].shape) == (0, 4)
        cloud, batch = ME.publish_map(am, ids)
        assert cloud.data == b"" and cloud.width == 0 and cloud.row_step == 0 and cloud.height == 1
        assert batch.count == 0 and batch.Lambda_world is None and tuple(batch.Sigma_world.shape) == (0, 3, 3)
    v = ME.extract_primitive_map_view(am, 999)
    assert v.count == 0 and v.tile_id == 999 and v.m_tile == m and tuple(v.slot_indices.shape) == (0,)
    assert ME.renderable_batch_from_view(v).Lambda_world is None
    assert ME.export_splats(am) is None
    am.close()


def test_capacity_one_short_raises_and_writes_nothing():
    from gcslam import _lib as L
    from gcslam import map_export as ME
    m = 192
    rng = np.random.default_rng(9)
    tiles = {1: _rand_tile(rng, m), 2: _rand_tile(rng, m)}
    am = _map(tiles, m)
    total = int(tiles[1]["valid_mask"].sum() + tiles[2]["valid_mask"].sum())
    with pytest.raises(ME.MapExportCapacityError) as e:
        ME.export_rows(am, [1, 2], None, 1, capacity=total - 1)
    assert e.value.n_rows == total and e.value.tile_rows.tolist() == [int(tiles[k]["valid_mask"].sum()) for k in (1, 2)]
    assert ME.export_rows(am, [1, 2], None, 1, capacity=total).n_rows == total
    # the library call on buffers with a guard region behind them
    guard = 64
    idx = np.array([am.index(1, create=False), am.index(2, create=False)], np.int32)
    tids = np.array([1, 2], np.int64)
    n_rows, tile_rows = np.zeros(1, np.int32), np.zeros(2, np.int32)
    for cap in (total - 1, total):
        t, o, buf = ME.export_buffers(NL, total + guard, "cuda:0")
        buf.fill_(0xA5)
        am._stream()
        rc = am.lib.gcs_pmap_export(am.h, L.iptr(idx), tids.ctypes.data_as(L.c_int64_p), 2, 0, 1, EPS_LIFT, 1e-12, cap,
                                    C.byref(o), L.iptr(n_rows), L.iptr(tile_rows))
        assert int(n_rows[0]) == total and int(tile_rows.sum()) == total
        assert rc == (0 if cap == total else -1)
        written = 0 if rc else total
        for f, x in t.items():
            b = cpu(x.reshape(total + guard, -1).view(torch.uint8))
            assert (b[written:] == 0xA5).all(), f
            if written:
                assert not (b[:written] == 0xA5).all(axis=1).any(), f
    am.close()


# ---------------------------------------------------------------------- PointCloud2 records
def test_pointcloud2_record_edge_values():
    from gcslam import map_export as ME
    m = 192
    rng = np.random.default_rng(13)
    t = _rand_tile(rng, m, frac=1.0)
    t["Lambdas"][:16] = np.eye(3)                     # with eps_lift = 0 the LU solve returns theta itself
    half = 1.0 + 2.0 ** -24                           # exactly halfway between two float32: to even, 1.0
    up = 1.0 + 2.0 ** -24 + 2.0 ** -30
    t["thetas"][:16] = 1.0
    t["thetas"][0] = [1e39, -1e39, half]
    t["thetas"][1] = [up, -half, 3.0 + 3 * 2.0 ** -23]    # halfway again, the even neighbour above: 3 + 2^-21
    t["weights"][:10] = [-1.0, 2e6, 1e6, np.inf, np.nan, 1e-40, -0.0, -np.inf, up, 0.5]
    t["last_supported_scan_seq"][:] = np.arange(m)[::-1]     # newest first = slot order
    tiles = {1: t}
    am = _map(tiles, m)
    g, ref = _check(am, tiles, [1], None, 1, eps_lift=0.0, view=False)
    assert np.array_equal(g["slots"], np.arange(m))
    assert np.array_equal(g["positions"][:2], t["thetas"][:2])
    words = g["points"].view(np.uint32)
    assert words[0, :3].tolist() == [0x7f800000, 0xff800000, 0x3f800000]
    assert words[1, :3].tolist() == [0x3f800001, 0xbf800000, 0x40400002]
    # clip(float32(w), 0, 1e6): NaN stays NaN; 1e-40 is a float32 denormal and is kept; numpy's clip keeps -0.0
    assert words[:4, 3].tolist() == [0, 0x49742400, 0x49742400, 0x49742400] and np.isnan(g["points"][4, 3])
    assert words[5, 3] == np.float32(1e-40).view(np.uint32) != 0
    assert words[6:10, 3].tolist() == [0x80000000, 0, 0x3f800001, 0x3f000000]
    cloud, batch = ME.publish_map(am, [1], eps_lift=0.0)
    assert cloud.data == g["points"].tobytes() and cloud.width == m and cloud.row_step == 16 * m
    assert (cloud.point_step, cloud.height, cloud.is_dense, cloud.is_bigendian) == (16, 1, True, False)
    assert [(f.name, f.offset, f.datatype, f.count) for f in cloud.fields] == [
        ("x", 0, 7, 1), ("y", 4, 7, 1), ("z", 8, 7, 1), ("intensity", 12, 7, 1)]
    am.close()


# ---------------------------------------------------------------------- the Python operators
def test_publish_map_view_and_batch_objects():
    from gcslam import map_export as ME
    m = 192
    rng = np.random.default_rng(17)
    tiles = {4: _rand_tile(rng, m), 9: _rand_tile(rng, m, frac=0.3), 2: _rand_tile(rng, m, frac=0.9)}
    am = _map(tiles, m)
    for ids, maxp in ((None, None), ([9, 77, 4], 40)):
        cloud, batch = ME.publish_map(am, ids, maxp)
        ref = R.publish(tiles, ids, maxp)
        assert isinstance(cloud.data, bytes) and cloud.width == ref["n"] == batch.count
        xyz = np.frombuffer(cloud.data, "<f4").reshape(-1, 4)
        _same_bits(xyz[:, :3], cpu(batch.mu_world).astype(np.float32), "cloud xyz")
        _same_bits(xyz[:, 3], np.frombuffer(ref["data"], "<f4").reshape(-1, 4)[:, 3], "cloud intensity")
        for f, k in (("mass", "weights"), ("eta", "etas"), ("color", "colors"), ("primitive_ids", "primitive_ids"),
                     ("source_tile_ids", "tile_ids"), ("source_slots", "slots"),
                     ("last_supported_scan_seq", "last_supported_scan_seq")):
            _same_bits(cpu(getattr(batch, f)), ref[k], f)
        np.testing.assert_allclose(cpu(batch.mu_world), ref["positions"], rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(cpu(batch.Sigma_world), ref["covariances"], rtol=1e-12, atol=1e-13)
        _check_lambda_world(dict(covariances=cpu(batch.Sigma_world), lambda_world=cpu(batch.Lambda_world)), EPS_LIFT)
        assert batch.valid_mask.dtype == torch.bool and bool(batch.valid_mask.all()) and batch.mu_world.is_cuda
    for tid, maxp in ((4, None), (4, 50), (9, 1000)):
        v = ME.extract_primitive_map_view(am, tid, maxp)
        ref = R.extract_primitive_map_view(tiles[tid], tid, maxp)
        assert (v.tile_id, v.m_tile, v.count) == (tid, m, len(ref["slot_indices"]))
        assert np.array_equal(cpu(v.slot_indices), ref["slot_indices"]) and v.slot_indices.dtype == torch.int32
        for f in ("weights", "primitive_ids", "colors", "etas"):
            _same_bits(cpu(getattr(v, f)), ref[f], f)
        np.testing.assert_allclose(cpu(v.positions), ref["positions"], rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(cpu(v.covariances), ref["covariances"], rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(cpu(v.kappas), ref["kappas"], rtol=1e-15, atol=0)
        np.testing.assert_allclose(cpu(v.directions), ref["directions"], rtol=1e-15, atol=1e-16)
        b = ME.renderable_batch_from_view(v)
        rb = R.renderable_batch_from_view(ref)
        assert sorted(k for k in rb) == ["Lambda_world", "Sigma_world", "color", "eta", "mass", "mu_world", "primitive_ids"]
        _same_bits(cpu(b.mass), rb["mass"], "mass")
        _same_bits(cpu(b.Sigma_world), cpu(v.covariances), "Sigma_world")
        _check_lambda_world(dict(covariances=cpu(b.Sigma_world), lambda_world=cpu(b.Lambda_world)), EPS_LIFT)
        with pytest.raises(ValueError):
            ME.renderable_batch_from_view(v, eps_lift=1e-6)
    am.close()


def test_export_splats(tmp_path):
    from gcslam import map_export as ME
    m = 192
    rng = np.random.default_rng(19)
    tiles = {30: _rand_tile(rng, m), 10: _rand_tile(rng, m, frac=0.0), 20: _rand_tile(rng, m, frac=0.9)}
    am = _map(tiles, m)
    path = str(tmp_path / "out" / "splats.npz")
    got = ME.export_splats(am, path)
    ref = R.export_splats(tiles)
    assert tuple(got) == tuple(ref) == R.SPLAT_KEYS == ME.SPLAT_KEYS and got["n"] == ref["n"] > 0
    for k in R.SPLAT_KEYS[:-1]:
        assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype, k
    for k in ("colors", "rgb", "weights", "timestamps", "created_timestamps", "primitive_ids", "cam_mass", "lidar_mass",
              "rgb_cam_accum", "rgb_cam_denom"):
        _same_bits(got[k], ref[k], k)
    np.testing.assert_allclose(got["positions"], ref["positions"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(got["covariances"], ref["covariances"], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(got["kappas"], ref["kappas"], rtol=1e-15, atol=0)
    np.testing.assert_allclose(got["directions"], ref["directions"], rtol=1e-15, atol=1e-16)
    with np.load(path) as z:
        assert sorted(z.files) == sorted(R.SPLAT_KEYS) and int(z["n"]) == got["n"]
        for k in R.SPLAT_KEYS[:-1]:
            _same_bits(z[k], got[k], k)
    am.close()


def test_render_of_the_export_equals_render_of_the_view():
    from gcslam import map_export as ME
    from gcslam import rendering as RD
    from gcslam.primitive_map import extract_atlas_map_view
    m = 192
    rng = np.random.default_rng(23)
    tiles = {1: _rand_tile(rng, m), 2: _rand_tile(rng, m, frac=0.8)}
    am = _map(tiles, m)
    kw = dict(bev=RD.BEVPushforwardConfig(n_views=3), cfg=RD.SplatRenderingConfig(tile_size=32, max_splats_per_tile=16),
              width=80, height=48, pixels_per_metre=6.0, centre_xy=(0.0, 0.0))
    cloud, batch = ME.publish_map(am, [1, 2], order=ME.ORDER_CONCAT)
    a = RD.render_map_view(batch, **kw)
    b = RD.render_map_view(extract_atlas_map_view(am, [1, 2], m), **kw)
    # the rows are bitwise the same and no two are bit-identical, so every image tile lists the same splats in
    # the same distance order; the view's row numbers differ (it is ordered by weight and keeps invalid rows)
    assert np.array_equal(cpu(a.tile_counts), cpu(b.tile_counts)) and int(a.tile_counts.max()) == 16
    np.testing.assert_allclose(cpu(a.images), cpu(b.images), rtol=1e-12, atol=1e-12)
    assert cpu(a.images).any()
    am.close()
