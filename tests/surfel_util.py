"""Surfel extraction test kit: seeded scenes (numpy), the restated launch dispatch of
gc-slam_amd/csrc/gcs_surfels.hip, the case table of the shape sweep with its guards, and the comparison
of a device result with the numpy oracle (oracle/surfels.py).

Shared by tests/test_surfels.py (CPU: every case is built and its guards run on the oracle alone, so a case
is known to reach its branch before it reaches a GPU), tests/test_gpu_surfels.py and
tests/test_gpu_surfel_shapes.py.

Bars (none set from a device result): cell buckets, clipped counts and the selected cell ids bit-exact (the
oracle hashes around the device's centre; the centre itself at 1e-12); positions, weights and timestamps at
rtol 1e-9; covariances and the information form at 1e-7 of the matrix norm; normals at 1e-7 absolute and
kappas at rtol 1e-6 where the cell's smallest eigenvalue is separated (gap > 1e-6 of the largest) -- the
guards of every value case assert that this holds for every selected cell.
"""

from __future__ import annotations

import functools
import os
import sys
from dataclasses import dataclass, field
from typing import Callable, Optional

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "gc-slam_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle import surfels as OS  # noqa: E402

SQ3H = OS.SQRT3_HALF
LADDER = (1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 300)   # raw occupants per cell
CONFIG_LADDER = (3, 4, 5, 6, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193)  # no cell below 3 points
LADDER_GRID = (8, 8, 2)


# --------------------------------------------------------------------------------------------------
# scenes
# --------------------------------------------------------------------------------------------------

def _lattice_to_xyz(s):
    """(s1, s2, sz) = (x, x/2 + sqrt3/2 y, z) -> (x, y, z)."""
    s = np.asarray(s, np.float64)
    x = s[..., 0]
    return np.stack([x, (s[..., 1] - 0.5 * x) / SQ3H, s[..., 2]], axis=-1)


def _patch(rng, centre, n, h, normal_noise):
    """n points of a planar patch: +-0.1 h in the plane, normal_noise * h (1 sigma) along a random normal."""
    nrm = rng.normal(size=3)
    nrm /= np.linalg.norm(nrm)
    e1, e2 = OS.orthonormal_basis_from_normal(nrm)
    uv = rng.uniform(-0.1 * h, 0.1 * h, (n, 2))
    d = rng.normal(size=(n, 1)) * (normal_noise * h)
    return centre[None, :] + uv[:, :1] * e1[None, :] + uv[:, 1:] * e2[None, :] + d * nrm[None, :]


def _assemble(patches, rng):
    """Every patch and its point-mirror through the origin (patch k -> label k, its mirror -> K + k), weights
    in [0.5, 1) and timestamps in [0, 0.1) drawn per point, everything shuffled together."""
    K = len(patches)
    pts = np.concatenate(patches + [-p for p in patches], axis=0)
    lab = np.concatenate([np.full(len(p), k) for k, p in enumerate(patches)] +
                         [np.full(len(p), K + k) for k, p in enumerate(patches)])
    n = len(pts)
    t, w = rng.uniform(0.0, 0.1, n), rng.uniform(0.5, 1.0, n)
    perm = rng.permutation(n)
    return np.ascontiguousarray(pts[perm]), t[perm], w[perm], lab[perm]


def _frozen(*arrs):
    for a in arrs:
        a.flags.writeable = False
    return arrs


@functools.lru_cache(maxsize=None)
def _ladder(counts, lattice, h, seed, normal_noise):
    rng = np.random.default_rng(seed)
    cells = [(a, b, c) for a in range((lattice[0] + 1) // 2) for b in range((lattice[1] + 1) // 2)
             for c in range((lattice[2] + 1) // 2)]
    assert len(counts) <= len(cells), "one cell of the lattice's positive octant per count"
    patches = [_patch(rng, _lattice_to_xyz((np.array(cells[k]) + 0.5) * h), n, h, normal_noise)
               for k, n in enumerate(counts)]
    return _frozen(*_assemble(patches, rng))


def ladder_scene(counts, lattice, h, seed, normal_noise=0.002, labels=False):
    """One planar patch of counts[k] points at the centre of the k-th cell of the lattice's positive octant
    (lattice coordinates (x, x/2 + sqrt3/2 y, z), cell size h), and its point-mirror through the origin: the
    weighted centre stays near 0, every patch stays in one cell, and 2 len(counts) cells hold exactly the
    prescribed raw counts.  Points are shuffled: a cell's occupants are scattered over the index range.
    Returns read-only (points, timestamps, weights) (and the per-point patch label: k, mirror len(counts) + k)."""
    r = _ladder(tuple(int(c) for c in counts), tuple(lattice), float(h), int(seed), float(normal_noise))
    return r if labels else r[:3]


@functools.lru_cache(maxsize=None)
def _grid(n_clusters, per_cluster, dims, h, seed):
    rng = np.random.default_rng(seed)
    cells = np.stack([rng.integers(-(n // 2), n - n // 2, n_clusters) for n in dims], axis=1)
    patches = [_patch(rng, _lattice_to_xyz((cells[k] + 0.5) * h), per_cluster, h, 0.002) for k in range(n_clusters)]
    return _frozen(*_assemble(patches, rng))


def grid_scene(n_clusters, per_cluster, dims, h, seed):
    """n_clusters planar patches of per_cluster points in random lattice cells over the signed range
    [-n/2, n/2) of each dimension (drawn with replacement: a few cells hold two patches; the negative half
    reaches its grid cell through the modulo wrap), mirrored and shuffled as ladder_scene.
    Returns read-only (points, timestamps, weights): 2 n_clusters per_cluster points."""
    return _grid(int(n_clusters), int(per_cluster), tuple(dims), float(h), int(seed))[:3]


def _head(scene, n):
    return tuple(np.ascontiguousarray(a[:n]) for a in scene)


def _masked(scene, step=7):
    """Every step-th point at the parse sentinel (masked: key n_cells, sorted last)."""
    p = scene[0].copy()
    p[::step] = OS.GC_NONFINITE_SENTINEL
    return p, scene[1], scene[2]


# --------------------------------------------------------------------------------------------------
# the launch dispatch, restated
# --------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class Dispatch:
    end_bit: int
    npass: int
    sort: str     # "none", "lds13", "lds14" or "rocprim"
    per: int


def dispatch(n, n_cells, lds_sort=True):
    """What a call with n points on a grid of n_cells cells launches (gcs_surfels.hip)."""
    end_bit = 1
    while (1 << end_bit) <= n_cells:                       # :684  keys 0..n_cells (n_cells: masked points)
        end_bit += 1
    npass = (end_bit + 7 - 1) // 7                         # :493  LSD passes of kSortDigitBits = 7
    if n <= 0:
        sort = "none"                                      # :751-757  every branch asks n > 0
    elif lds_sort and n <= (1 << 13) and end_bit + 13 <= 32:
        sort = "lds13"                                     # :751  k_sf_sort_lds<13>, kSortMax = 8,192
    elif lds_sort and n <= (1 << 14) and end_bit + 13 + 1 <= 32:
        sort = "lds14"                                     # :754  k_sf_sort_lds<14>, kSortMaxWide = 16,384
    else:
        sort = "rocprim"                                   # :757-762  radix_sort_pairs + k_sf_bounds
    per = (n_cells + 1024 - 1) // 1024                     # :363  cells per thread of k_sf_slots (kSelThreads)
    return Dispatch(end_bit, npass, sort, per)


SEL_BATCH = 16                                             # :367  kSelBatch: flags loaded together


# --------------------------------------------------------------------------------------------------
# oracle-side measurements used by the guards
# --------------------------------------------------------------------------------------------------

def raw_counts(ref, n_cells):
    """Unclipped occupants per cell of an oracle result."""
    return np.bincount(ref["linear"][ref["mask"]], minlength=n_cells)


def eigen_gaps(points, weights, ref):
    """(ev1 - ev0) / ev2 of the oracle's cell covariance (recomputed from the members) per selected cell."""
    p, wt = np.asarray(points), np.asarray(weights)
    out = np.zeros(len(ref["cell_ids"]))
    for s, k in enumerate(ref["cell_ids"]):
        idx = ref["bucket"][k, :ref["count"][k]]
        pc = p[idx] - ref["center"]
        w = wt[idx]
        ws = w.sum() + 1e-12
        m = (pc * w[:, None]).sum(0) / ws
        d = pc - m
        ev = np.linalg.eigvalsh((d * w[:, None]).T @ d / ws + 1e-12 * np.eye(3))
        out[s] = (ev[1] - ev[0]) / ev[2]
    return out


# --------------------------------------------------------------------------------------------------
# cases
# --------------------------------------------------------------------------------------------------

@dataclass
class Case:
    id: str
    group: str
    scene: Callable[[], tuple]                  # () -> (points, timestamps, weights)
    cfg: dict                                   # oracle configuration fields
    guard: Optional[Callable] = None            # (case, ref, points, t, w) -> None: asserts on the oracle alone
    mode: str = "value"                         # "value": n_valid > 0, every selected cell's normal determined
    #                                             "flat": compare what does not depend on the plane normal
    #                                             "empty": n_valid == 0 (padding rows only)
    max_points: Optional[int] = None            # context capacity (default: the cloud's size)
    knob: Optional[str] = None                  # environment A/B knob: also run at "0", bitwise equal
    want: dict = field(default_factory=dict)    # expected dispatch: sort / npass / per

    def ocfg(self):
        return OS.SurfelExtractionConfig(**self.cfg)

    def oracle(self, center=None):
        p, t, w = self.scene()
        return OS.extract_surfels_mahex3d(p, t, w, self.ocfg(), center=center, only_occupied=True)


def guards(case: Case, ref):
    """Assertions on the oracle's output alone that show the case reaches its branch."""
    p, t, w = case.scene()
    ocfg = case.ocfg()
    d = dispatch(len(p), ocfg.n_cells)
    for k, v in case.want.items():
        assert getattr(d, k) == v, (case.id, k, getattr(d, k), v)
    if case.mode == "value":
        assert ref["n_valid"] > 0
        gaps = eigen_gaps(p, w, ref)
        assert len(gaps) == ref["n_valid"] and gaps.min() > 1e-6, (case.id, gaps.min())
    elif case.mode == "empty":
        assert ref["n_valid"] == 0
    if case.guard is not None:
        case.guard(case, ref, p, t, w)


def _ladder_cfg(**kw):
    c = dict(n_surfel=32, n_feat=4, voxel_size_m=0.5, hex3d_num_cells_1=LADDER_GRID[0],
             hex3d_num_cells_2=LADDER_GRID[1], hex3d_num_cells_z=LADDER_GRID[2], hex3d_max_occupants=64)
    c.update(kw)
    return c


def _grid_cfg(dims, h=0.25, **kw):
    c = dict(voxel_size_m=h, hex3d_num_cells_1=dims[0], hex3d_num_cells_2=dims[1], hex3d_num_cells_z=dims[2],
             hex3d_max_occupants=8)
    c.update(kw)
    return c


LADDER_SEED = 0


def _ladder_scene():
    return ladder_scene(LADDER, LADDER_GRID, 0.5, LADDER_SEED)


def _config_scene():
    return ladder_scene(CONFIG_LADDER, LADDER_GRID, 0.5, LADDER_SEED)


# ---- occupancy: k_sf_moments' three forms (:228-254) and the bucket fill (:217, k_sf_cells :162-172)

def _occupancy_guard(max_occ):
    def g(case, ref, p, t, w):
        raw = raw_counts(ref, case.ocfg().n_cells)
        assert sorted(raw[raw > 0]) == sorted(LADDER + LADDER)
        assert np.array_equal(ref["count"], np.minimum(raw, max_occ))
        if max_occ >= 65:
            assert ref["count"].max() >= 65          # the second 64-lane step (register cache, u = 1)
        if max_occ >= 129:
            assert ref["count"].max() >= 129         # the reload path (u >= 2)
        assert int((raw > max_occ).sum()) == 2 * sum(c > max_occ for c in LADDER)
        assert ref["n_valid"] == 2 * sum(min(c, max_occ) >= 3 for c in LADDER)
        if max_occ >= 32:
            assert ref["n_valid"] == 28
        assert np.abs(ref["center"]).max() < 0.05 * 0.5   # patches (+-0.14 h about a cell centre) stay in their cell
    return g


def _occupancy_cases():
    out = []
    for m in (1, 32, 64, 65, 128, 129, 192, 256, 1024):
        out.append(Case(f"occupancy-{m}", "occupancy", _ladder_scene, _ladder_cfg(hex3d_max_occupants=m),
                        guard=_occupancy_guard(m), mode="empty" if m == 1 else "value",
                        knob="GCSLAM_SF_FOLD_CELLS" if m in (65, 129, 1024) else None,
                        want=dict(sort="lds13", npass=2, per=1)))
    return out


# ---- grid size and slot selection: k_sf_slots' batch and tail (:370-388), pass counts (:493)

GRID_SEEDS = {(1, 1, 1): 0, (4, 4, 4): 0, (5, 7, 3): 0, (32, 16, 32): 0, (33, 32, 16): 1, (64, 64, 16): 2,
              (64, 64, 64): 0, (128, 64, 64): 0}
GRID_CLUSTERS = {(1, 1, 1): 3, (4, 4, 4): 40, (5, 7, 3): 30}


def _grid_scene_of(dims):
    return functools.partial(grid_scene, GRID_CLUSTERS.get(dims, 500), 4, dims, 0.25, GRID_SEEDS[dims])


def _grid_guard(truncates):
    def g(case, ref, p, t, w):
        ocfg = case.ocfg()
        d = dispatch(len(p), ocfg.n_cells)
        n_valid_cells = int(ref["cell_valid"].sum())
        if truncates:
            assert n_valid_cells > ocfg.n_surfel and ref["n_valid"] == ocfg.n_surfel
        else:
            assert ref["n_valid"] == n_valid_cells
        ids = ref["cell_ids"]
        if d.per > SEL_BATCH:                         # the one-by-one tail of both loops
            assert (ids % d.per >= SEL_BATCH).any() and ids[-1] % d.per >= SEL_BATCH
        occ = np.flatnonzero(raw_counts(ref, ocfg.n_cells))
        top = 7 * (d.npass - 1)
        if (ocfg.n_cells - 1) >> top:                 # the top pass sorts a non-zero digit of an occupied cell
            assert occ.max() >> top > 0               # (on 2^14 cells only the masked key reaches it)
    return g


def _grid_cases():
    spec = [((1, 1, 1), 1, False, 1, 1), ((4, 4, 4), 64, False, 1, 1), ((5, 7, 3), 20, True, 1, 1),
            ((32, 16, 32), 700, True, 3, 16), ((33, 32, 16), 700, True, 3, 17),
            ((64, 64, 16), 700, True, 3, 64), ((64, 64, 16), 1, True, 3, 64),
            ((64, 64, 64), 700, True, 3, 256), ((64, 64, 64), 1, True, 3, 256),
            ((128, 64, 64), 700, True, 3, 512), ((128, 64, 64), 1, True, 3, 512)]
    return [Case(f"grid-{d[0]}x{d[1]}x{d[2]}-s{ns}", "grid", _grid_scene_of(d), _grid_cfg(d, n_surfel=ns),
                 guard=_grid_guard(tr), want=dict(sort="rocprim" if d == (128, 64, 64) else "lds13", npass=npass, per=per))
            for d, ns, tr, npass, per in spec]


# ---- sort path and capacity edges (:751-762): every seventh point masked, LDS sort against rocPRIM

SORT_SEED = 0


def _sort_scene(dims, n):
    def f():
        return _masked(_head(grid_scene((n + 7) // 8 + 1, 4, dims, 0.25, SORT_SEED), n))
    return f


def _sort_guard(idx_bits):
    def g(case, ref, p, t, w):
        n = len(p)
        assert int((~ref["mask"]).sum()) == (n + 6) // 7 > 0        # masked points carry key n_cells
        d = dispatch(n, case.ocfg().n_cells)
        if idx_bits:                                                # at the packed word's capacity: bit 31 is set
            assert d.end_bit + idx_bits == 32 and (case.ocfg().n_cells << idx_bits) >> 31 == 1
        assert dispatch(n, case.ocfg().n_cells, lds_sort=False).sort == "rocprim"
    return g


def _sort_cases():
    spec = [("lds13-limit", (64, 64, 64), 8192, 1024, "lds13", 13), ("past-lds13", (64, 64, 64), 8193, 1024, "rocprim", 0),
            ("lds14-limit", (64, 64, 63), 12000, 1024, "lds14", 14), ("past-lds14", (128, 64, 64), 4000, 1024, "rocprim", 0),
            ("one-pass", (4, 4, 4), 300, 64, "lds13", 0)]
    return [Case(f"sort-{name}", "sort", _sort_scene(d, n), _grid_cfg(d, n_surfel=ns), guard=_sort_guard(bits),
                 knob="GCSLAM_SF_LDS_SORT", want=dict(sort=sort, npass=1 if name == "one-pass" else 3))
            for name, d, n, ns, sort, bits in spec]


# ---- point counts around the sort's seams: 64 lanes a step, 512 / 1,024 entries a wave, 8,192 / 16,384

COUNT_GRID = (16, 16, 4)
COUNT_SEED = 0
POINT_COUNTS = (1, 2, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 8191, 8192, 8193, 16383, 16384, 16385)


@functools.lru_cache(maxsize=None)
def _count_base():
    """16,400 points: 8 whole clusters and their mirrors shuffled among the first 64 (so the slices of a few
    dozen points hold valid cells), the rest shuffled behind them."""
    a, b = grid_scene(8, 4, COUNT_GRID, 0.25, COUNT_SEED), grid_scene(2042, 4, COUNT_GRID, 0.25, COUNT_SEED + 1)
    return _frozen(*(np.concatenate([x, y]) for x, y in zip(a, b)))


def _count_cases():
    out = []
    for i, n in enumerate(POINT_COUNTS):
        sort = "lds13" if n <= 8192 else "lds14" if n <= 16384 else "rocprim"
        out.append(Case(f"count-{n}", "count", functools.partial(lambda n: _head(_count_base(), n), n),
                        _grid_cfg(COUNT_GRID, n_surfel=1024, hex3d_max_occupants=32),
                        mode="empty" if n < 3 else "value", max_points=n + 3000 if i % 2 else None,
                        want=dict(sort=sort, npass=2, per=1)))
    return out


# ---- adversarial key distributions

KEY_GRID = (16, 16, 4)


@functools.lru_cache(maxsize=None)
def _one_cell_patch():
    rng = np.random.default_rng(11)
    p = _patch(rng, np.array([0.3, -0.2, 0.1]), 8192, 0.5, 0.002)
    return _frozen(p, rng.uniform(0.0, 0.1, 8192), rng.uniform(0.5, 1.0, 8192))


@functools.lru_cache(maxsize=None)
def _one_cell_stacked():
    """8,192 points at one position: whichever cell the centred position falls in, it holds them all (a patch
    of distinct points around its own weighted centre would straddle the lattice corner at the origin)."""
    rng = np.random.default_rng(12)
    p = np.tile(np.array([[0.7, -1.3, 0.4]]), (8192, 1))
    return _frozen(p, rng.uniform(0.0, 0.1, 8192), rng.uniform(0.5, 1.0, 8192))


def _all_masked():
    rng = np.random.default_rng(13)
    return np.full((300, 3), OS.GC_NONFINITE_SENTINEL), np.linspace(0, 0.1, 300), rng.uniform(0.5, 1.0, 300)


@functools.lru_cache(maxsize=None)
def _one_per_cell():
    rng = np.random.default_rng(14)
    half = [(a, b, c) for a in range(KEY_GRID[0] // 2) for b in range(-(KEY_GRID[1] // 2), KEY_GRID[1] // 2)
            for c in range(-(KEY_GRID[2] // 2), KEY_GRID[2] // 2)]
    cells = np.array(half)[rng.permutation(len(half))[:300]]
    patches = [_lattice_to_xyz((c + 0.5) * 0.25 + rng.uniform(-0.025, 0.025, 3))[None, :] for c in cells]
    return _frozen(*_assemble(patches, rng))[:3]


@functools.lru_cache(maxsize=None)
def _descending_keys():
    p, t, w = grid_scene(500, 4, KEY_GRID, 0.25, 15)
    ocfg = OS.SurfelExtractionConfig(**_grid_cfg(KEY_GRID, n_surfel=1024))
    mask, _, c = OS.point_mask_and_center(p, w, ocfg.eig_min)
    order = np.argsort(-OS.bin_points_3d(p - c[None, :], mask, ocfg)[2].astype(np.int64), kind="stable")
    return _frozen(np.ascontiguousarray(p[order]), t[order].copy(), w[order].copy())


def _key_cases():
    def one_cell(case, ref, p, t, w):
        raw = raw_counts(ref, case.ocfg().n_cells)
        assert (raw > 0).sum() == 1 and raw.max() == 8192
        k = int(raw.argmax())
        assert np.array_equal(ref["bucket"][k], np.arange(32)) and ref["count"][k] == 32   # the 32 lowest indices

    def all_masked(case, ref, p, t, w):
        assert not ref["mask"].any() and np.all(ref["center"] == 0.0) and np.all(ref["bucket"] == -1)

    def one_per_cell(case, ref, p, t, w):
        raw = raw_counts(ref, case.ocfg().n_cells)
        assert raw.max() == 1 and raw.sum() == 600 and ref["n_valid"] == 600

    def descending(case, ref, p, t, w):
        lin = ref["linear"].astype(np.int64)
        assert np.all(np.diff(lin) <= 0) and len(np.unique(lin)) > 300

    return [
        Case("keys-one-cell", "keys", _one_cell_patch, _grid_cfg((1, 1, 1), h=0.5, n_surfel=1, hex3d_max_occupants=32),
             guard=one_cell, want=dict(sort="lds13", npass=1)),
        Case("keys-one-cell-stacked", "keys", _one_cell_stacked, _grid_cfg(KEY_GRID, n_surfel=64, hex3d_max_occupants=32),
             guard=one_cell, mode="flat", want=dict(sort="lds13", npass=2)),
        Case("keys-all-masked", "keys", _all_masked, _grid_cfg((8, 8, 4), n_surfel=64, hex3d_max_occupants=32),
             guard=all_masked, mode="empty", want=dict(sort="lds13", npass=2)),
        Case("keys-one-per-cell", "keys", _one_per_cell,
             _grid_cfg(KEY_GRID, n_surfel=1024, min_points_per_voxel=1), guard=one_per_cell, mode="flat"),
        Case("keys-descending", "keys", _descending_keys, _grid_cfg(KEY_GRID, n_surfel=1024), guard=descending),
    ]


# ---- weight edges: validity through ws > 0 (:347)

@functools.lru_cache(maxsize=None)
def _zero_weight_cells():
    p, t, w, lab = ladder_scene(LADDER, LADDER_GRID, 0.5, LADDER_SEED, labels=True)
    w = w.copy()
    k33, k65 = LADDER.index(33), LADDER.index(65)
    w[(lab == k33) | (lab == len(LADDER) + k33)] = 0.0          # the cell and its mirror: the centre stays put
    w[np.flatnonzero(lab == k65)[0]] = 0.0                      # one zero-weight occupant of a live cell
    return _frozen(p, t, w)


def _all_zero_weights():
    p, t, w = _ladder_scene()
    return p, t, np.zeros_like(w)


def _weight_cases():
    def zero_cell(case, ref, p, t, w):
        _, _, _, lab = ladder_scene(LADDER, LADDER_GRID, 0.5, LADDER_SEED, labels=True)
        k = int(ref["linear"][np.flatnonzero(lab == LADDER.index(33))[0]])
        assert raw_counts(ref, case.ocfg().n_cells)[k] == 33 and ref["count"][k] == 33
        assert not ref["cell_valid"][k] and ref["n_valid"] == 26          # 33 >= min_points, yet ws = 0
        j = int(np.flatnonzero(lab == LADDER.index(65))[0])
        kk = int(ref["linear"][j])
        assert ref["cell_valid"][kk] and j in ref["bucket"][kk] and w[j] == 0.0

    def all_zero(case, ref, p, t, w):
        assert ref["count"].max() == 64 and not ref["cell_valid"].any() and np.all(ref["center"] == 0.0)

    return [Case("weights-zero-cell", "weights", _zero_weight_cells, _ladder_cfg(), guard=zero_cell),
            Case("weights-all-zero", "weights", _all_zero_weights, _ladder_cfg(), guard=all_zero, mode="empty")]


# ---- non-default configurations of k_sf_fit (:282-347) and k_sf_write (:437-444)

def _planar_scene():
    return ladder_scene(CONFIG_LADDER, LADDER_GRID, 0.5, LADDER_SEED, normal_noise=0.0)


def _config_cases():
    def kappa_inside(case, ref, p, t, w):
        o, k = case.ocfg(), ref["kappas"][:ref["n_valid"]]
        assert ((k > o.kappa_min) & (k < o.kappa_max)).sum() > 0.5 * ref["n_valid"]

    def kappa_floor(case, ref, p, t, w):
        o, k = case.ocfg(), ref["kappas"][:ref["n_valid"]]
        assert (k == o.kappa_min).sum() > 0.5 * ref["n_valid"]

    def min_points(n_valid, lo_valid):
        def g(case, ref, p, t, w):
            raw = raw_counts(ref, case.ocfg().n_cells)
            assert ref["n_valid"] == n_valid
            for c in (3, 4, 5):
                assert all(bool(ref["cell_valid"][k]) == (c >= lo_valid) for k in np.flatnonzero(raw == c))
            assert not ref["cell_valid"][raw == 0].any() and (raw == 0).any()     # empty: 0 >= 0, yet ws = 0
        return g

    def planar(case, ref, p, t, w):
        sps = ref["cell_fit"]["sigma_perp_sq"][ref["cell_ids"]]
        assert (sps == case.ocfg().eig_min).any() and sps.max() < 1.001 * case.ocfg().eig_min   # the floor is active

    L = _ladder_cfg
    return [
        Case("config-kappa-inside", "config", _ladder_scene, L(kappa_main_scale=0.01), guard=kappa_inside),
        Case("config-kappa-min", "config", _ladder_scene, L(kappa_main_scale=1e-4, kappa_min=0.2, kappa_max=50.0),
             guard=kappa_floor),
        Case("config-wishart-nu-0", "config", _config_scene, L(wishart_nu=0.0, sensor_noise_var_per_axis=1e-4)),
        Case("config-wishart-psi-0", "config", _config_scene, L(wishart_psi_scale=0.0)),
        Case("config-eps-lift", "config", _config_scene, L(eps_lift=1e-6)),
        Case("config-min-points-0", "config", _config_scene, L(min_points_per_voxel=0), guard=min_points(32, 0)),
        Case("config-min-points-5", "config", _config_scene, L(min_points_per_voxel=5), guard=min_points(28, 5)),
        Case("config-planar", "config", _planar_scene, L(), guard=planar),
    ]


CASES = (_occupancy_cases() + _grid_cases() + _sort_cases() + _count_cases() + _key_cases() + _weight_cases() +
         _config_cases())


# ---- one context, many calls

def _scene300():
    return _head(grid_scene(40, 4, KEY_GRID, 0.25, 16), 300)


def _empty_cloud():
    return np.zeros((0, 3)), np.zeros(0), np.zeros(0)


def _seq_base():
    return grid_scene(2500, 4, KEY_GRID, 0.25, 17)                 # 20,000 points


@dataclass
class Sequence:
    id: str
    cfg: dict
    max_points: int
    calls: tuple            # scene functions, in call order
    sorts: tuple            # the sort each call takes
    modes: tuple            # per call, as Case.mode


SEQUENCES = (
    Sequence("large-small-empty-large", _grid_cfg(KEY_GRID, n_surfel=64, hex3d_max_occupants=32), 20000,
             (_one_cell_stacked, _scene300, _empty_cloud, _one_cell_stacked), ("lds13", "lds13", "none", "lds13"),
             ("flat", "value", "empty", "flat")),
    Sequence("three-sort-paths", _grid_cfg(KEY_GRID, n_surfel=1024, hex3d_max_occupants=32), 20000,
             tuple(functools.partial(lambda n: _head(_seq_base(), n), n) for n in (12000, 20000, 5000)),
             ("lds14", "rocprim", "lds13"), ("value", "value", "value")),
)


def sequence_cases(seq: Sequence):
    """The calls of a sequence as cases (each is also compared with the oracle on its own)."""
    return [Case(f"{seq.id}-{i}", "sequence", f, seq.cfg, mode=m, max_points=seq.max_points, want=dict(sort=s))
            for i, (f, s, m) in enumerate(zip(seq.calls, seq.sorts, seq.modes))]


# --------------------------------------------------------------------------------------------------
# device runs and the comparison with the oracle
# --------------------------------------------------------------------------------------------------

def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _cfg(o: OS.SurfelExtractionConfig):
    from gcslam.surfels import SurfelExtractionConfig
    return SurfelExtractionConfig(**{k: getattr(o, k) for k in o.__dataclass_fields__})


def _compare(got, ref, cfg: OS.SurfelExtractionConfig, points, weights):
    """Returns the number of selected cells whose normal and kappa were compared (the determined ones)."""
    n = ref["n_valid"]
    assert got["n_valid"] == n
    assert np.array_equal(_np(got["bucket"]), ref["bucket"])
    assert np.array_equal(_np(got["count"]), ref["count"])
    ids = _np(got["cell_ids"])
    assert np.array_equal(ids[:n], ref["cell_ids"]) and np.all(ids[n:] == -1)
    for k in ("positions", "weights", "timestamps"):
        np.testing.assert_allclose(_np(got[k]), ref[k], rtol=1e-9, atol=1e-12, err_msg=k)
    cov = _np(got["covariances"]).reshape(-1, 3, 3)
    for i in range(cfg.n_surfel):
        sc = max(np.abs(ref["covariances"][i]).max(), 1e-300)
        np.testing.assert_allclose(cov[i], ref["covariances"][i], rtol=1e-7, atol=1e-7 * sc)
    # normals / kappas where the plane normal is determined
    nrm, kap = _np(got["normals"]), _np(got["kappas"])
    checked = 0
    for s, k in enumerate(ref["cell_ids"]):
        cnt = ref["count"][k]
        idx = ref["bucket"][k, :cnt]
        # eigen gap of the oracle's covariance (recomputed from the members)
        pc = np.asarray(points)[idx] - ref["center"]
        w = np.asarray(weights)[idx]
        ws = w.sum() + 1e-12
        m = (pc * w[:, None]).sum(0) / ws
        d = pc - m
        cv = (d * w[:, None]).T @ d / ws + 1e-12 * np.eye(3)
        ev = np.linalg.eigvalsh(cv)
        if ev[1] - ev[0] > 1e-6 * ev[2]:
            np.testing.assert_allclose(nrm[s], ref["normals"][s], rtol=0, atol=1e-7)
            np.testing.assert_allclose(kap[s], ref["kappas"][s], rtol=1e-6)
            checked += 1
    return checked


def compare_flat(got, ref):
    """What does not depend on an undetermined plane normal: buckets, counts, cell ids, n_valid, positions,
    weights, timestamps, kappas (same bars as _compare)."""
    n = ref["n_valid"]
    assert got["n_valid"] == n
    assert np.array_equal(_np(got["bucket"]), ref["bucket"])
    assert np.array_equal(_np(got["count"]), ref["count"])
    ids = _np(got["cell_ids"])
    assert np.array_equal(ids[:n], ref["cell_ids"]) and np.all(ids[n:] == -1)
    for k in ("positions", "weights", "timestamps"):
        np.testing.assert_allclose(_np(got[k]), ref[k], rtol=1e-9, atol=1e-12, err_msg=k)
    np.testing.assert_allclose(_np(got["kappas"]), ref["kappas"], rtol=1e-6, err_msg="kappas")


def compare_info(got, ref, cfg: OS.SurfelExtractionConfig):
    """The LiDAR slice in information form (k_sf_write) against measurement_batch_add_lidar_surfels on the
    oracle's surfels: 1e-7 of the array's scale (the bar of test_reference_smoke_two_clusters_on_gpu)."""
    rb = OS.lidar_measurement_batch(ref, cfg)
    sl = slice(cfg.n_feat, cfg.n_feat + cfg.n_surfel)
    for k in ("Lambdas", "thetas", "etas", "colors"):
        r = rb[k][sl]
        np.testing.assert_allclose(_np(got[k]), r, rtol=1e-7, atol=1e-7 * max(np.abs(r).max(), 1.0), err_msg=k)
    assert np.array_equal(_np(got["valid_mask"]).astype(bool), rb["valid_mask"][sl])
    assert np.array_equal(_np(got["source_indices"]), rb["source_indices"][sl])


def snapshot(r):
    """Host copies of one extract() result (its tensors belong to the extractor)."""
    return {k: (_np(v).copy() if hasattr(v, "cpu") else np.asarray(v)) for k, v in r.items()}


def assert_bitwise_equal(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


def writable(*arrs):
    """Copies of the cached read-only scene arrays for the host-to-device upload."""
    return tuple(np.array(a) for a in arrs)


def device_run(points, t, w, ocfg, max_points=None):
    """One call on a fresh context -> snapshot (intermediates included)."""
    from gcslam.surfels import SurfelExtractor
    ex = SurfelExtractor(_cfg(ocfg), max_points=max_points or max(len(points), 16))
    try:
        return snapshot(ex.extract(*writable(points, t, w), want_intermediates=True))
    finally:
        ex.close()


def check_center(got, points, w, ocfg):
    mask, w_eff, c_np = OS.point_mask_and_center(points, w, ocfg.eig_min)
    # sums of +-metres cancel in a near-zero component: absolute bar 1e-13 of the coordinate scale
    scale = max(np.abs(np.asarray(points)[mask]).max(initial=0.0), 1.0)
    np.testing.assert_allclose(got["center"], c_np, rtol=1e-12, atol=1e-13 * scale)


def _run(points, t, w, ocfg, device_center=True, max_points=None, only_occupied=False):
    from gcslam.surfels import SurfelExtractor
    ex = SurfelExtractor(_cfg(ocfg), max_points=max_points or max(len(points), 16))
    try:
        got = ex.extract(points, t, w, want_intermediates=True)
    finally:
        ex.close()
    check_center(got, points, w, ocfg)
    ref = OS.extract_surfels_mahex3d(points, t, w, ocfg, center=got["center"] if device_center else None,
                                     only_occupied=only_occupied)
    return got, ref
