"""A numpy restatement of the keypoint detector's definition (include/gcslam_hip.h, steps 1-6) and the fixtures
of tests/test_keypoints_host.py and tests/test_gpu_keypoints.py, built from fixed seeds.  Written from the
definition, not from the C++: whole-image array operations, no per-pixel code shared with the library.
A fixture whose restated result misses its stated condition fails by assertion where it is built, so no
comparison can pass on an empty set."""

import functools

import numpy as np

RING = ((0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3),
        (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1), (-2, -2), (-1, -3))
DEFAULTS = dict(fast_threshold=20, edge_threshold=31, max_keypoints=4096, max_width=1920, max_height=1080,
                harris_k=0.04)


def grey(image):
    """Step 1."""
    a = np.asarray(image, np.uint8)
    if a.ndim == 2:
        return a.copy()
    r, g, b = (a[:, :, j].astype(np.int64) for j in range(3))
    return ((4899 * r + 9617 * g + 1868 * b + 8192) >> 14).astype(np.uint8)


def fast_scores(g, fast_threshold):
    """Step 2: the one-byte score image."""
    H, W = g.shape
    out = np.zeros((H, W), np.uint8)
    if H < 7 or W < 7:
        return out
    im = g.astype(np.int32)
    centre = im[3:H - 3, 3:W - 3]
    d = np.stack([im[3 + dy:H - 3 + dy, 3 + dx:W - 3 + dx] - centre for dx, dy in RING])
    d = np.concatenate([d, d[:8]])
    m = np.full(centre.shape, -256, np.int32)
    for s in range(16):
        arc = d[s:s + 9]
        m = np.maximum(m, np.maximum(arc.min(0), (-arc).min(0)))
    out[3:H - 3, 3:W - 3] = np.where(m > fast_threshold, m, 0)
    return out


def survivors(score, edge_threshold):
    """Steps 3 and 4: the raster indices' (y, x) of the corners that survive suppression and the border."""
    H, W = score.shape
    p = np.zeros((H + 2, W + 2), np.int32)
    p[1:-1, 1:-1] = score
    c = p[1:-1, 1:-1]
    keep = c > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                keep &= c > p[1 + dy:H + 1 + dy, 1 + dx:W + 1 + dx]
    yy, xx = np.mgrid[0:H, 0:W]
    e = edge_threshold
    keep &= (xx >= e) & (xx < W - e) & (yy >= e) & (yy < H - e)
    return np.nonzero(keep)   # raster order


def responses(g, ys, xs, harris_k):
    """Step 5."""
    if len(ys) == 0:
        return np.zeros(0, np.float32)
    im = np.pad(g.astype(np.int64), 1)   # (the padding is never inside a survivor's block: edge_threshold >= 4)
    H, W = g.shape
    ix = (im[0:H, 2:] + 2 * im[1:H + 1, 2:] + im[2:, 2:]) - (im[0:H, 0:W] + 2 * im[1:H + 1, 0:W] + im[2:, 0:W])
    iy = (im[2:, 0:W] + 2 * im[2:, 1:W + 1] + im[2:, 2:]) - (im[0:H, 0:W] + 2 * im[0:H, 1:W + 1] + im[0:H, 2:])
    o = np.arange(-3, 4)
    by = ys[:, None, None] + o[None, :, None]
    bx = xs[:, None, None] + o[None, None, :]
    wx, wy = ix[by, bx], iy[by, bx]
    a, b, c = (wx * wx).sum((1, 2)), (wy * wy).sum((1, 2)), (wx * wy).sum((1, 2))
    s = 1.0 / (4 * 7 * 255)
    s4 = ((s * s) * s) * s
    det = (a * b - c * c).astype(np.float64)
    tr2 = ((a + b) * (a + b)).astype(np.float64)
    return ((det - np.float64(harris_k) * tr2) * s4).astype(np.float32)


def detect(image, fast_threshold=20, edge_threshold=31, max_keypoints=4096, harris_k=0.04, **_):
    """Steps 1-6: dict of u, v, response (float32, raster order), counts (n_keypoints, n_survivors, n_corners),
    and the score image."""
    g = grey(image)
    H, W = g.shape
    score = fast_scores(g, fast_threshold)
    ys, xs = survivors(score, edge_threshold)
    r = responses(g, ys, xs, harris_k)
    n = len(ys)
    if n > max_keypoints:
        raster = ys * W + xs
        order = np.lexsort((raster, -r.astype(np.float64)))   # response descending, then raster index ascending
        kept = np.sort(order[:max_keypoints])
        ys, xs, r = ys[kept], xs[kept], r[kept]
    return dict(u=xs.astype(np.float32), v=ys.astype(np.float32), response=r,
                counts=(len(ys), n, int((score > 0).sum())), score=score)


# ---- fixtures

def _blocks(W, H, block, seed, noise=6):
    g = np.random.default_rng(seed)
    colours = g.integers(0, 256, ((H + block - 1) // block, (W + block - 1) // block, 3))
    img = np.repeat(np.repeat(colours, block, 0), block, 1)[:H, :W]
    if noise:
        img = img + g.integers(-noise, noise + 1, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


def _dots(W, H):
    img = np.full((H, W), 40, np.uint8)
    img[8::12, 8::12] = 220
    return img


def _single(W, H, x, y):
    img = np.zeros((H, W), np.uint8)
    img[y, x] = 255
    return img


def _noise(W, H, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W), dtype=np.uint8)


# name: (image builder, config overrides, least keypoints the restatement must find)
_BUILD = {
    "blocks_48x64": (lambda: _blocks(48, 64, 8, 11), dict(edge_threshold=4), 30),
    "blocks_61x97": (lambda: _blocks(61, 97, 6, 12), dict(edge_threshold=4), 100),
    "blocks_64x96": (lambda: _blocks(64, 96, 5, 13), dict(edge_threshold=4), 150),
    "blocks_clean": (lambda: _blocks(61, 97, 6, 12, noise=0), dict(edge_threshold=4), 0),
    "dots_64x96": (lambda: _dots(64, 96), dict(edge_threshold=4), 30),
    "noise_48x64": (lambda: _noise(48, 64, 14), dict(edge_threshold=4), 150),
    "dot_9x9": (lambda: _single(9, 9, 4, 4), dict(edge_threshold=4), 1),
    "tiny_6x6": (lambda: _noise(6, 6, 15), dict(edge_threshold=4), 0),
    "tiny_7x200": (lambda: _noise(7, 200, 16), dict(edge_threshold=4), 0),
    "tiny_200x8": (lambda: _noise(200, 8, 17), dict(edge_threshold=4), 0),
    "tiny_64x48_edge31": (lambda: _blocks(64, 48, 8, 18), dict(edge_threshold=31), 0),
    "wide_130x35": (lambda: _blocks(130, 35, 6, 19), dict(edge_threshold=4), 30),
    "vga": (lambda: _blocks(640, 480, 16, 20), dict(), 513),
}
NAMES = tuple(_BUILD)
SMALL = tuple(n for n in NAMES if n != "vga")
TINY = tuple(n for n in NAMES if n.startswith("tiny"))
RGB = tuple(n for n in NAMES if n.startswith(("blocks", "wide", "vga", "tiny_64x48")))


def config(name, **over):
    """The fixture's full config as keyword arguments (KeypointConfig's fields)."""
    c = dict(DEFAULTS)
    c.update(_BUILD[name][1])
    c.update(over)
    return c


@functools.lru_cache(maxsize=None)
def image(name):
    img = _BUILD[name][0]()
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _expected(name, over):
    ref = detect(image(name), **config(name, **dict(over)))
    for a in (ref["u"], ref["v"], ref["response"], ref["score"]):
        a.setflags(write=False)
    return ref


def expected(name, **over):
    """The restated result of a fixture (computed once per config and left unchanged)."""
    ref = _expected(name, tuple(sorted(over.items())))
    if not over:
        _check_condition(name, ref)
    return ref


def _check_condition(name, ref):
    n, n_surv, n_corners = ref["counts"]
    least = _BUILD[name][2]
    assert n >= least, (name, n, least)
    if name.startswith("blocks_") and name != "blocks_clean":
        assert (ref["response"] < 0).any(), name
    if name == "blocks_clean":   # the strict-tie rule: corners, and every one of them tied with a neighbour
        assert n_corners > 100 and n == 0, (name, ref["counts"])
    if name == "dots_64x96":
        assert len(set(ref["response"].tobytes()[4 * i:4 * i + 4] for i in range(n))) == 1, name
    if name == "dot_9x9":
        assert n == 1 and (ref["u"][0], ref["v"][0]) == (4.0, 4.0) and ref["score"][4, 4] == 255, name
    if name in TINY:
        assert n == 0, (name, n)
