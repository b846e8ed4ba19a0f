"""A numpy restatement of the grid keypoint detector's definition (include/gcslam_hip.h, "keypoints spread over a
grid of cells", G1-G4) and the fixtures of tests/test_keypoints_grid_host.py and tests/test_gpu_keypoints_grid.py.
Written from the definition on tests/keypoints_ref.py and tests/keypoints_pyramid_ref.py (imported, not edited):
every level's survivors from their whole-image steps, then cells, budgets and the fair share with lexsort.  A
fixture whose restated result misses its stated condition fails by assertion where it is built, so no comparison
can pass on an empty set."""

import functools

import numpy as np

import keypoints_pyramid_ref as PR
import keypoints_ref as KR

MAX_LEVELS = PR.MAX_LEVELS
DEFAULTS = dict(PR.DEFAULTS, cell_size=32, redistribute=1)


def ramp(W, H, block, seed):
    """KR._blocks with its contrast ramped from 1.0 to 0.12 left to right."""
    return np.clip(128 + (KR._blocks(W, H, block, seed).astype(np.float64) - 128)
                   * np.linspace(1.0, 0.12, W)[None, :, None], 0, 255).astype(np.uint8)


def cells(W_l, H_l, edge, cell_size):
    """G1: (n_cx, n_cy); (0, 0) for a level whose kept area is empty."""
    if W_l <= 2 * edge or H_l <= 2 * edge:
        return 0, 0
    return -(-(W_l - 2 * edge) // cell_size), -(-(H_l - 2 * edge) // cell_size)


def budgets(quota, surv, redistribute):
    """G2."""
    b = [min(q, s) for q, s in zip(quota, surv)]
    if redistribute:
        spare = sum(q - x for q, x in zip(quota, b))
        for l in range(len(b)):
            give = min(spare, surv[l] - b[l])
            b[l] += give
            spare -= give
    return b


def fair_share(resp, raster, cell, b):
    """G3 on one level: (kept mask, t, rem)."""
    n = len(resp)
    if n == 0:
        return np.zeros(0, bool), 0, 0
    order = np.lexsort((raster, -resp.astype(np.float64), cell))   # by cell, then response descending, then raster
    rank = np.empty(n, np.int64)
    sc = cell[order]
    start = np.r_[0, np.nonzero(np.diff(sc))[0] + 1]
    first = np.repeat(start, np.diff(np.r_[start, n]))
    rank[order] = np.arange(n) - first + 1
    n_c = np.bincount(cell)
    t = 0
    while t < n_c.max() and np.minimum(n_c, t + 1).sum() <= b:
        t += 1
    rem = b - int(np.minimum(n_c, t).sum())
    keep = rank <= t
    nxt = np.nonzero(rank == t + 1)[0]
    best = nxt[np.lexsort((raster[nxt], -resp[nxt].astype(np.float64)))][:rem]
    keep[best] = True
    assert keep.sum() == b
    return keep, t, rem


def detect(image, fast_threshold=20, edge_threshold=31, max_keypoints=4096, harris_k=0.04, n_levels=8,
           scale_num=6, scale_den=5, cell_size=32, redistribute=1, **_):
    g0 = KR.grey(image)
    H, W = g0.shape
    e = edge_threshold
    sizes = PR.level_sizes(W, H, n_levels, scale_num, scale_den)
    quota = PR.quotas(max_keypoints, n_levels, scale_num, scale_den)
    found, corners, grid = [], [], []
    for l, (W_l, H_l) in enumerate(sizes):
        grid.append(cells(W_l, H_l, e, cell_size) if W_l >= 1 and H_l >= 1 else (0, 0))
        if W_l < 1 or H_l < 1:
            found.append(None)
            corners.append(0)
            continue
        g = g0 if l == 0 else PR.resample(g0, W_l, H_l)
        score = KR.fast_scores(g, fast_threshold)
        ys, xs = KR.survivors(score, e)
        found.append((ys, xs, KR.responses(g, ys, xs, harris_k)))
        corners.append(int((score > 0).sum()))
    surv = [0 if f is None else len(f[0]) for f in found]
    b = budgets(quota, surv, redistribute)
    rows = dict(u=[], v=[], response=[], level=[])
    level_counts = np.zeros((MAX_LEVELS, 6), np.int32)
    rem, occupied = [0] * n_levels, [0] * n_levels
    for l, (W_l, H_l) in enumerate(sizes):
        level_counts[l, 3] = quota[l]
        if found[l] is None:
            continue
        ys, xs, r = found[l]
        cell = (ys - e) // cell_size * grid[l][0] + (xs - e) // cell_size
        assert len(ys) == 0 or (cell.max() < grid[l][0] * grid[l][1] and np.bincount(cell).max() <= 1024)
        keep, t, rem[l] = fair_share(r, ys * W_l + xs, cell, b[l])
        level_counts[l] = (keep.sum(), surv[l], corners[l], quota[l], b[l], t)
        occupied[l] = len(set(cell[keep].tolist()))
        rows["u"].append(PR.coord(xs[keep], W, W_l))
        rows["v"].append(PR.coord(ys[keep], H, H_l))
        rows["response"].append(r[keep])
        rows["level"].append(np.full(int(keep.sum()), l, np.int32))
    out = {k: np.concatenate(v) if v else np.zeros(0, np.int32 if k == "level" else np.float32) for k, v in rows.items()}
    out["level"] = out["level"].astype(np.int32)
    out["counts"] = tuple(int(v) for v in level_counts[:, :3].sum(0)) + (n_levels,)
    out["level_counts"] = level_counts
    out["sizes"], out["quota"], out["grid"], out["rem"], out["occupied"] = sizes, quota, grid, rem, occupied
    out["nonempty"] = [0 if f is None or len(f[0]) == 0 else
                       len(set(((f[0] - e) // cell_size * grid[l][0] + (f[1] - e) // cell_size).tolist()))
                       for l, f in enumerate(found)]
    return out


def layout(W, H, edge_threshold=31, max_keypoints=4096, n_levels=8, scale_num=6, scale_den=5, cell_size=32, **_):
    """gcs_keypoint_grid_layout's rows: W_l, H_l, quota_l, n_cx, n_cy."""
    out = np.zeros((MAX_LEVELS, 5), np.int32)
    sizes = PR.level_sizes(W, H, n_levels, scale_num, scale_den)
    quota = PR.quotas(max_keypoints, n_levels, scale_num, scale_den)
    for l, (W_l, H_l) in enumerate(sizes):
        out[l] = (W_l, H_l, quota[l]) + (cells(W_l, H_l, edge_threshold, cell_size) if W_l >= 1 and H_l >= 1 else (0, 0))
    return out


def occupied_pyramid(name):
    """The cells (of the fixture's grid) that the pyramid detector's kept keypoints fall into, per level."""
    cfg = config(name)
    e, cs = cfg["edge_threshold"], cfg["cell_size"]
    img = image(name)
    H, W = img.shape[:2]
    ref = PR.detect(img, **cfg)
    out = []
    for l, (W_l, H_l) in enumerate(ref["sizes"]):
        m = ref["level"] == l
        # the level's own pixel from the level-0 coordinate: x = ((u + 0.5) 2 W_l / W - 1) / 2
        x = np.rint(((ref["u"][m].astype(np.float64) + 0.5) * 2 * W_l / W - 1) / 2).astype(np.int64)
        y = np.rint(((ref["v"][m].astype(np.float64) + 0.5) * 2 * H_l / H - 1) / 2).astype(np.int64)
        assert (PR.coord(x, W, W_l) == ref["u"][m]).all() and (PR.coord(y, H, H_l) == ref["v"][m]).all()
        out.append(len(set(zip(((x - e) // cs).tolist(), ((y - e) // cs).tolist()))))
    return out


# ---- fixtures

E4 = dict(edge_threshold=4)
_R96 = lambda: ramp(96, 64, 5, 31)
_R200 = lambda: ramp(200, 150, 6, 32)
ONE_CELL = dict(E4, cell_size=64, redistribute=0)
# name: (image name in keypoints_ref, or a builder; config overrides)
_BUILD = {
    "ramp_vga_k512": (lambda: ramp(640, 480, 16, 30), dict(max_keypoints=512)),
    "ramp_96x64_l3_k48_c16": (_R96, dict(E4, n_levels=3, max_keypoints=48, cell_size=16)),
    "ramp_96x64_l3_k24_c8": (_R96, dict(E4, n_levels=3, max_keypoints=24, cell_size=8)),
    "blocks_61x97_l3_k200_c16": ("blocks_61x97", dict(E4, n_levels=3, max_keypoints=200, cell_size=16)),
    "ramp_200x150_k256_c16": (_R200, dict(max_keypoints=256, cell_size=16)),
    "ramp_200x150_k256_c16_off": (_R200, dict(max_keypoints=256, cell_size=16, redistribute=0)),
    "ramp_200x150_k512_c16": (_R200, dict(max_keypoints=512, cell_size=16)),
    "ramp_200x150_k512_c16_off": (_R200, dict(max_keypoints=512, cell_size=16, redistribute=0)),
    "dots_64x96_l3_k16_c16": ("dots_64x96", dict(E4, n_levels=3, max_keypoints=16, cell_size=16)),
    "blocks_48x64_one_cell": ("blocks_48x64", dict(ONE_CELL, n_levels=3)),
    "noise_48x64_one_cell": ("noise_48x64", dict(ONE_CELL, n_levels=3)),
    "noise_48x64_one_cell_k40": ("noise_48x64", dict(ONE_CELL, n_levels=3, max_keypoints=40)),
    "dot_9x9_l8": ("dot_9x9", dict(ONE_CELL)),
    "tiny_6x6_l8": ("tiny_6x6", dict(ONE_CELL)),
    "one_1x1_l8": (lambda: np.full((1, 1), 200, np.uint8), dict(ONE_CELL)),
    "tiny_64x48_edge31": ("tiny_64x48_edge31", dict()),
}
NAMES = tuple(_BUILD)
ONE_CELL_NAMES = ("blocks_48x64_one_cell", "noise_48x64_one_cell", "noise_48x64_one_cell_k40", "dot_9x9_l8")
EMPTY = ("tiny_6x6_l8", "one_1x1_l8", "tiny_64x48_edge31")


def config(name, **over):
    """The fixture's full config as keyword arguments (GridConfig's fields)."""
    c = dict(DEFAULTS)
    c.update(_BUILD[name][1])
    c.update(over)
    return c


@functools.lru_cache(maxsize=None)
def image(name):
    src = _BUILD[name][0]
    if isinstance(src, str):
        return KR.image(src)
    img = src()
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _expected(name, over):
    ref = detect(image(name), **config(name, **dict(over)))
    for k in ("u", "v", "response", "level", "level_counts"):
        ref[k].setflags(write=False)
    return ref


def expected(name, **over):
    """The restated result of a fixture (computed once per config and left unchanged)."""
    ref = _expected(name, tuple(sorted(over.items())))
    if not over:
        _check_condition(name, ref)
    return ref


def _check_condition(name, ref):
    lc = ref["level_counts"]
    kept, surv, quota, b, t = (lc[:, j].tolist() for j in (0, 1, 3, 4, 5))
    rem, occ = ref["rem"], ref["occupied"]
    cfg = config(name)
    L = cfg["n_levels"]
    assert ref["counts"][0] == sum(kept) == len(ref["u"]) and kept == b and sum(quota) == cfg["max_keypoints"], name
    assert sum(b) == (min(cfg["max_keypoints"], sum(surv)) if cfg["redistribute"] else sum(min(q, s) for q, s in zip(quota, surv)))
    for l in range(L):   # G3's last sentence
        if b[l] >= ref["nonempty"][l]:
            assert occ[l] == ref["nonempty"][l], (name, l)
    if name == "ramp_vga_k512":
        assert surv == [766, 574, 603, 493, 466, 384, 294, 136], (name, surv)
        assert b == quota == [114, 92, 77, 64, 53, 44, 37, 31], (name, b)
        assert t == [0, 0, 0, 1, 1, 1, 1, 2] and rem == [114, 92, 77, 0, 7, 14, 17, 8], (name, t, rem)
        assert occ == [114, 92, 77, 64, 46, 30, 20, 12], (name, occ)
        assert occupied_pyramid(name) == [49, 33, 21, 18, 14, 10, 8, 5]
    if name == "ramp_96x64_l3_k48_c16":
        assert surv[:3] == [100, 67, 61] and quota[:3] == [20, 15, 13], (name, surv, quota)
        assert t[:3] == [1, 1, 1] and rem[:3] == [2, 3, 3], (name, t, rem)
        assert occ[:3] == [18, 12, 10] == ref["nonempty"][:3], (name, occ)
        assert occupied_pyramid(name) == [6, 4, 3]
        assert ref["grid"][0] == (6, 4) and (96 - 8) % 16 and (64 - 8) % 16   # a partial last column and row of cells
    if name == "ramp_96x64_l3_k24_c8":
        assert t[:3] == [0, 0, 0] and rem[:3] == quota[:3] == [11, 7, 6] and occ[:3] == [11, 7, 6], (name, t, rem, occ)
    if name == "blocks_61x97_l3_k200_c16":   # the deep cap with a remainder
        assert surv[:3] == [147, 100, 67] and quota[:3] == [81, 65, 54], (name, surv, quota)
        assert t[:3] == [3, 4, 7] and rem[:3] == [14, 8, 4], (name, t, rem)
    if name.startswith("ramp_200x150"):
        assert surv == [223, 131, 74, 34, 5, 0, 0, 0], (name, surv)
        assert ref["grid"][4][0] > 0 and ref["grid"][5] == (0, 0) and ref["sizes"][5][0] >= 1   # levels without cells
    if name.startswith("ramp_200x150_k256"):
        assert quota == [59, 46, 38, 32, 26, 22, 18, 15], (name, quota)
    if name == "ramp_200x150_k256_c16_off":
        assert b == [59, 46, 38, 32, 5, 0, 0, 0] and sum(b) == 180, (name, b)
        assert t[:4] == [1, 1, 2, 9] and rem[:4] == [10, 19, 9, 0], (name, t, rem)
    if name == "ramp_200x150_k256_c16":
        assert b == [135, 46, 38, 32, 5, 0, 0, 0] and sum(b) == 256, (name, b)
        assert t[0] == 3 and rem[0] == 1, (name, t, rem)
    if name == "ramp_200x150_k512_c16":   # every survivor is kept: no remainder on any level
        assert b == surv and sum(b) == 467 and rem == [0] * 8, (name, b, rem)
        assert t == [9, 11, 10, 11, 3, 0, 0, 0], (name, t)   # G3: no larger than max_c n_c, the fullest cell's count
    if name == "dots_64x96_l3_k16_c16":   # equal responses: the ties go to the lowest raster indices among the cells' firsts
        assert surv[:3] == [35, 35, 35] and quota[:3] == [7, 5, 4] == kept[:3], (name, surv, quota)
        full = KR.expected("dots_64x96")
        assert len(set(full["response"].tolist())) == 1 and t[0] == 0 and rem[0] == 7
        firsts = {}
        for x, y in sorted(zip(full["u"].astype(int).tolist(), full["v"].astype(int).tolist()), key=lambda p: (p[1], p[0])):
            firsts.setdefault(((y - 4) // 16, (x - 4) // 16), (x, y))
        want = sorted(firsts.values(), key=lambda p: (p[1], p[0]))[:7]
        assert list(zip(ref["u"][:7].astype(int).tolist(), ref["v"][:7].astype(int).tolist())) == want, name
    if name in ONE_CELL_NAMES:   # G5: the pyramid detector's result
        pyr = PR.detect(image(name), **cfg)
        assert all(g in ((1, 1), (0, 0)) for g in ref["grid"]), (name, ref["grid"])
        assert all(ref[k].tobytes() == pyr[k].tobytes() for k in ("u", "v", "response", "level")), name
        assert lc[:, :4].tobytes() == pyr["level_counts"].tobytes() and ref["counts"] == pyr["counts"] and ref["counts"][0] > 0
    if name == "noise_48x64_one_cell_k40":
        assert all(s > q for s, q in zip(surv[:3], quota[:3])), (name, surv, quota)   # the one cell's cap bites
    if name in EMPTY:
        assert ref["counts"][0] == 0, (name, ref["counts"])
    if name == "tiny_64x48_edge31":
        assert ref["grid"][0] == (0, 0) and ref["sizes"][0] == (64, 48), name
