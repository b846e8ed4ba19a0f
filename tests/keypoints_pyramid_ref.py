"""A numpy restatement of the pyramid keypoint detector's definition (include/gcslam_hip.h, "keypoints over a
scale pyramid") and the fixtures of tests/test_keypoints_pyramid_host.py and tests/test_gpu_keypoints_pyramid.py.
Written from the definition: the level sizes and quotas in Python integers, every level as wy @ I_0 @ wx.T with the
dense overlap-weight matrices, and per level tests/keypoints_ref.py's detect on the resampled array.  A fixture
whose restated result misses its stated condition fails by assertion where it is built, so no comparison can pass
on an empty set."""

import functools

import numpy as np

import keypoints_ref as KR

MAX_LEVELS = 8
DEFAULTS = dict(KR.DEFAULTS, n_levels=8, scale_num=6, scale_den=5)


def level_sizes(W, H, n_levels, scale_num, scale_den):
    out = []
    for l in range(n_levels):
        N, D = scale_num ** l, scale_den ** l
        out.append(((2 * W * D + N) // (2 * N), (2 * H * D + N) // (2 * N)))
    return out


def quotas(K, n_levels, scale_num, scale_den):
    w = [scale_den ** l * scale_num ** (n_levels - 1 - l) for l in range(n_levels)]
    q = [0] + [(K * w[l]) // sum(w) for l in range(1, n_levels)]
    q[0] = K - sum(q)
    return q


def weights(W, W_l):
    """wx[x, j]: the overlap of [x W, (x + 1) W) and [j W_l, (j + 1) W_l); every row sums to W."""
    x, j = np.arange(W_l, dtype=np.int64)[:, None], np.arange(W, dtype=np.int64)[None, :]
    w = np.clip(np.minimum((x + 1) * W, (j + 1) * W_l) - np.maximum(x * W, j * W_l), 0, None)
    assert (w.sum(1) == W).all()
    return w


def resample(g0, W_l, H_l):
    """Level image of size H_l x W_l from the level-0 grey image: the exact pixel-area mean, rounded half up."""
    H, W = g0.shape
    assert 255 * W * H < 2 ** 53   # every partial sum below is then an integer that float64 holds exactly
    s = weights(H, H_l).astype(np.float64) @ g0.astype(np.float64) @ weights(W, W_l).astype(np.float64).T
    out = (s.astype(np.int64) + (W * H) // 2) // (W * H)
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def coord(x, W, W_l):
    q = ((2 * x.astype(np.int64) + 1) * W).astype(np.float64) / np.float64(2 * W_l)
    return (q - 0.5).astype(np.float32)


def detect(image, fast_threshold=20, edge_threshold=31, max_keypoints=4096, harris_k=0.04, n_levels=8,
           scale_num=6, scale_den=5, **_):
    g0 = KR.grey(image)
    H, W = g0.shape
    sizes = level_sizes(W, H, n_levels, scale_num, scale_den)
    quota = quotas(max_keypoints, n_levels, scale_num, scale_den)
    rows = dict(u=[], v=[], response=[], level=[])
    level_counts = np.zeros((MAX_LEVELS, 4), np.int32)
    images = []
    for l, (W_l, H_l) in enumerate(sizes):
        level_counts[l, 3] = quota[l]
        if W_l < 1 or H_l < 1:
            images.append(None)
            continue
        g = g0 if l == 0 else resample(g0, W_l, H_l)
        images.append(g)
        ref = KR.detect(g, fast_threshold, edge_threshold, quota[l], harris_k)
        level_counts[l, :3] = ref["counts"]
        rows["u"].append(coord(ref["u"], W, W_l))
        rows["v"].append(coord(ref["v"], H, H_l))
        rows["response"].append(ref["response"])
        rows["level"].append(np.full(len(ref["u"]), l, np.int32))
    out = {k: np.concatenate(v) if v else np.zeros(0, np.int32 if k == "level" else np.float32) for k, v in rows.items()}
    out["counts"] = tuple(int(v) for v in level_counts[:, :3].sum(0)) + (n_levels,)
    out["level_counts"] = level_counts
    out["sizes"], out["quota"], out["images"] = sizes, quota, images
    return out


# ---- fixtures

def _big():
    return KR._blocks(1024, 704, 16, 21)


E4 = dict(edge_threshold=4)
# name: (image name in keypoints_ref, or a builder; config overrides)
_BUILD = {
    "vga_k4096": ("vga", dict()),
    "vga_k512": ("vga", dict(max_keypoints=512)),
    "blocks_64x96_l4_k64": ("blocks_64x96", dict(E4, n_levels=4, max_keypoints=64)),
    "blocks_61x97_l3": ("blocks_61x97", dict(E4, n_levels=3)),
    "wide_130x35_l3": ("wide_130x35", dict(E4, n_levels=3)),
    "noise_48x64_l3": ("noise_48x64", dict(E4, n_levels=3)),
    "dots_64x96_l3": ("dots_64x96", dict(E4, n_levels=3)),
    "dots_64x96_l3_k16": ("dots_64x96", dict(E4, n_levels=3, max_keypoints=16)),
    "dot_9x9_l8": ("dot_9x9", dict(E4)),
    "tiny_6x6_l8": ("tiny_6x6", dict(E4)),
    "one_1x1_l8": (lambda: np.full((1, 1), 200, np.uint8), dict(E4)),
    "blocks_60x96_l3_s2": (lambda: np.ascontiguousarray(KR.image("blocks_61x97")[:96, :60]),
                           dict(E4, n_levels=3, scale_num=2, scale_den=1)),
    "big_1024x704": (_big, dict()),
}
NAMES = tuple(_BUILD)
LARGE = ("vga_k4096", "vga_k512", "big_1024x704")
SMALL = tuple(n for n in NAMES if n not in LARGE)
NO_QUOTA_BITES = ("blocks_61x97_l3", "wide_130x35_l3", "noise_48x64_l3", "dots_64x96_l3")


def config(name, **over):
    """The fixture's full config as keyword arguments (PyramidConfig's fields)."""
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
    lc, sizes = ref["level_counts"], ref["sizes"]
    kept, surv, quota = lc[:, 0].tolist(), lc[:, 1].tolist(), lc[:, 3].tolist()
    L = len(sizes)
    assert ref["counts"][0] == sum(kept) == len(ref["u"]) and sum(quota) == config(name)["max_keypoints"], name
    if name == "vga_k4096":   # every level has more survivors than its quota
        assert list(zip(surv, quota)) == [(1387, 894), (1153, 741), (1179, 617), (941, 514), (853, 428), (702, 357),
                                          (490, 297), (292, 248)], (name, surv, quota)
        assert sizes[7] == (179, 134) and kept == quota, (name, sizes)
    if name == "vga_k512":
        assert quota == [114, 92, 77, 64, 53, 44, 37, 31] and kept == quota, (name, quota, kept)
    if name == "blocks_64x96_l4_k64":
        assert quota[:4] == [22, 17, 14, 11] and kept == quota and all(s > q for s, q in zip(surv[:4], quota)), (name, surv)
        assert sizes[1:] == [(53, 80), (44, 67), (37, 56)], (name, sizes)
    if name in NO_QUOTA_BITES:
        assert kept == surv and min(kept[:L]) >= 30, (name, kept)
    if name == "blocks_61x97_l3":
        assert sizes[1:] == [(51, 81), (42, 67)], sizes
    if name == "wide_130x35_l3":
        assert sizes[1:] == [(108, 29), (90, 24)], sizes
    if name == "noise_48x64_l3":
        assert sizes[2] == (33, 44), sizes
    if name == "dots_64x96_l3_k16":   # level 0: 35 equal responses, the first 7 lattice points in raster order stay
        assert quota[:3] == [7, 5, 4] and surv[0] == 35 and kept[0] == 7, (name, quota, surv, kept)
        full = KR.expected("dots_64x96")
        assert len(set(full["response"].tolist())) == 1
        lattice = [(x, y) for y in range(8, 92, 12) for x in range(8, 60, 12)]
        assert list(zip(ref["u"][:7].astype(int).tolist(), ref["v"][:7].astype(int).tolist())) == lattice[:7]
    if name in ("dot_9x9_l8", "tiny_6x6_l8", "one_1x1_l8"):
        assert ref["counts"][0] <= 1 and min(sizes) < (4, 4), (name, sizes, ref["counts"])
    if name == "dot_9x9_l8":
        assert ref["counts"][0] == 1 and (ref["u"][0], ref["v"][0], ref["level"][0]) == (4.0, 4.0, 0), name
    if name == "one_1x1_l8":
        assert [w >= 1 for w, _ in sizes] == [True] * 4 + [False] * 4, sizes
    if name == "blocks_60x96_l3_s2":   # the even part of blocks_61x97: exact 2 x 2 and 4 x 4 box means
        g0 = ref["images"][0].astype(np.int64)
        for l, b in ((1, 2), (2, 4)):
            assert sizes[l] == (60 // b, 96 // b), sizes
            box = g0.reshape(96 // b, b, 60 // b, b).sum((1, 3))
            assert (ref["images"][l] == (box + b * b // 2) // (b * b)).all(), (name, l)
        assert min(kept[:3]) > 0, (name, kept)
    if name == "big_1024x704":   # more strips of 2048 keys than the scan's workgroup has threads
        strips = sum((w * h + 2047) // 2048 for w, h in sizes)
        assert strips > 1024 and ref["counts"][0] > 1000, (name, strips, ref["counts"])
