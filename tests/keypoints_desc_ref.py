"""A numpy restatement of the keypoint describer's and the descriptor matcher's definition (include/gcslam_hip.h,
"keypoint descriptors", D1-D7) and the fixtures of tests/test_keypoints_desc_host.py and
tests/test_gpu_keypoints_desc.py.  Written from the definition on tests/keypoints_ref.py, keypoints_pyramid_ref.py and
keypoints_grid_ref.py (imported, not edited): the level images are the pyramid restatement's, the keypoints of the
detector fixtures are the grid restatement's, the direction table is recomputed from cos and sin, and the pattern
comes from tools/gen_brief_pattern.py.  A fixture whose restated result misses its stated condition fails by
assertion where it is built, so no comparison can pass on an empty set."""

import functools
import math
import os
import sys

import numpy as np

import keypoints_grid_ref as GR
import keypoints_pyramid_ref as PR
import keypoints_ref as KR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_brief_pattern as GEN   # noqa: E402

DEFAULTS = dict(n_levels=8, scale_num=6, scale_den=5, max_width=1920, max_height=1080, max_keypoints=4096)
MARGIN, NONE = 16, 257


# ---- D3, D5: the table and the steering

def directions():
    """The 32 rows (C_k, S_k): 0..7 rounded from cos and sin, the rest by quarter turns."""
    t = [(round(2 ** 14 * math.cos(math.radians(11.25 * k))), round(2 ** 14 * math.sin(math.radians(11.25 * k))))
         for k in range(8)]
    assert t == [(16384, 0), (16069, 3196), (15137, 6270), (13623, 9102), (11585, 11585), (9102, 13623), (6270, 15137),
                 (3196, 16069)]
    for k in range(8, 32):
        t.append((-t[k - 8][1], t[k - 8][0]))
    return np.array(t, np.int64)


DIR = directions()
PATTERN = np.array(GEN.pattern(), np.int64)   # (256, 4): ax, ay, bx, by


def rnd14(n):
    """n / 2^14 rounded half away from zero, in integers."""
    n = np.asarray(n, np.int64)
    return np.sign(n) * ((np.abs(n) + 8192) >> 14)


def steer(x, y, k):
    C, S = DIR[k]
    return rnd14(x * C - y * S), rnd14(x * S + y * C)


def scores(m10, m01):
    return int(m10) * DIR[:, 0] + int(m01) * DIR[:, 1]   # int64: |m| < 2^23, |C| <= 2^14


def level_pixel(u, W_l, W_0):
    """D1; u a float32 array of finite values."""
    return np.floor((u.astype(np.float64) + 0.5) * np.float64(W_l) / np.float64(W_0))


# ---- D1-D6

_DY, _DX = np.mgrid[-15:16, -15:16]
_DISC = _DX * _DX + _DY * _DY <= 225


def describe(image, u, v, level=None, n_levels=8, scale_num=6, scale_den=5, **_):
    """dict of desc (n, 32) uint8, angle float32, angle_bin int32, and, for the condition checks, x, y (level pixel,
    -1 on an invalid row), m10, m01 and tie (the argmax of D3 is not unique)."""
    g0 = KR.grey(image)
    H, W = g0.shape
    sizes = PR.level_sizes(W, H, n_levels, scale_num, scale_den)
    images = {}
    n = len(u)
    u, v = np.asarray(u, np.float32), np.asarray(v, np.float32)
    level = np.zeros(n, np.int32) if level is None else np.asarray(level, np.int32)
    out = dict(desc=np.zeros((n, 32), np.uint8), angle=np.full(n, np.nan, np.float32), angle_bin=np.full(n, -1, np.int32),
               x=np.full(n, -1, np.int64), y=np.full(n, -1, np.int64), m10=np.zeros(n, np.int64), m01=np.zeros(n, np.int64),
               tie=np.zeros(n, bool))
    for i in range(n):
        l = int(level[i])
        if not (np.isfinite(u[i]) and np.isfinite(v[i])) or l < 0 or l >= n_levels:
            continue
        W_l, H_l = sizes[l]
        if W_l < 1 or H_l < 1:
            continue
        x, y = level_pixel(u[i:i + 1], W_l, W)[0], level_pixel(v[i:i + 1], H_l, H)[0]
        if x < MARGIN or x >= W_l - MARGIN or y < MARGIN or y >= H_l - MARGIN:
            continue
        x, y = int(x), int(y)
        if l not in images:
            images[l] = (g0 if l == 0 else PR.resample(g0, W_l, H_l)).astype(np.int64)
        g = images[l]
        patch = g[y - 15:y + 16, x - 15:x + 16]
        m10, m01 = int((_DX * patch)[_DISC].sum()), int((_DY * patch)[_DISC].sum())
        s = scores(m10, m01)
        k = int(np.argmax(s))   # the first of the largest: ties to the lowest k
        ax, ay = steer(PATTERN[:, 0], PATTERN[:, 1], k)
        bx, by = steer(PATTERN[:, 2], PATTERN[:, 3], k)
        assert max(np.abs(ax).max(), np.abs(ay).max(), np.abs(bx).max(), np.abs(by).max()) <= 14

        def B(px, py):
            return np.array([g[y + q - 2:y + q + 3, x + p - 2:x + p + 3].sum() for p, q in zip(px.tolist(), py.tolist())])

        bits = (B(ax, ay) < B(bx, by)).astype(np.uint8)
        out["desc"][i] = np.packbits(bits, bitorder="little")
        out["angle"][i] = np.float32(np.arctan2(np.float64(m01), np.float64(m10)))
        out["angle_bin"][i] = k
        out["x"][i], out["y"][i], out["m10"][i], out["m01"][i] = x, y, m10, m01
        out["tie"][i] = int((s == s.max()).sum()) > 1
    return out


# ---- D7

def match(q, t, q_bin=None, t_bin=None):
    """(idx, dist, dist2), int32."""
    q, t = np.asarray(q, np.uint8).reshape(-1, 32), np.asarray(t, np.uint8).reshape(-1, 32)
    n_q, n_t = len(q), len(t)
    idx, dist, dist2 = np.full(n_q, -1, np.int32), np.full(n_q, NONE, np.int32), np.full(n_q, NONE, np.int32)
    qv = np.ones(n_q, bool) if q_bin is None else np.asarray(q_bin) >= 0
    tv = np.ones(n_t, bool) if t_bin is None else np.asarray(t_bin) >= 0
    if n_q == 0 or not tv.any():
        return idx, dist, dist2
    d = np.zeros((n_q, n_t), np.int64)
    for lo in range(0, n_q, 64):
        d[lo:lo + 64] = np.unpackbits(q[lo:lo + 64, None, :] ^ t[None, :, :], axis=2).sum(2)
    d[:, ~tv] = NONE
    best = np.argmin(d, axis=1)   # the first of the smallest: ties to the lowest index
    rows = np.arange(n_q)
    idx[qv], dist[qv] = best[qv], d[rows, best][qv]
    d[rows, best] = NONE
    dist2[qv] = d.min(axis=1)[qv]
    return idx, dist, dist2


def match_filtered(a, b, max_distance=64, ratio=(4, 5), cross_check=True):
    """gcslam.descriptors.match_descriptors' filters on match's outputs; a, b: describe's dicts."""
    idx, dist, dist2 = match(a["desc"], b["desc"], a["angle_bin"], b["angle_bin"])
    keep = (idx >= 0) & (dist <= max_distance) & (dist.astype(np.int64) * ratio[1] < ratio[0] * dist2.astype(np.int64))
    if cross_check:
        back = match(b["desc"], a["desc"], b["angle_bin"], a["angle_bin"])[0]
        keep &= back[np.clip(idx, 0, None)] == np.arange(len(idx)) if len(back) else False
    at = np.nonzero(keep)[0]
    return at.astype(np.int32), idx[at], dist[at]


# ---- describer fixtures: name -> (image, config overrides, u, v, level or None)

def _noise(W, H, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W), dtype=np.uint8)


def _from_grid(name, **over):
    ref = GR.expected(name, **over)
    cfg = GR.config(name, **over)
    return GR.image(name), {k: cfg[k] for k in ("n_levels", "scale_num", "scale_den")}, ref["u"], ref["v"], ref["level"]


def _hand_40():
    u = np.array([15, 16, 23, 24, np.nan, 20, 20, 20, 20, np.inf], np.float32)
    v = np.array([20, 20, 20, 20, 20, 20, 15, 16, 23, 20], np.float32)
    level = np.array([0, 0, 0, 0, 0, -1, 0, 0, 0, 0], np.int32)
    return _noise(40, 40, 41), dict(n_levels=1), u, v, level


def _quarter(turned):
    """A 64 x 64 level-0 noise image with 13 keypoints, or its np.rot90 with the keypoints at the turned places: the
    pixel (x, y) of m is the pixel (y, N - 1 - x) of np.rot90(m)."""
    N = 64
    img = _noise(N, N, 42)
    g = np.random.default_rng(43)
    x, y = g.integers(16, N - 16, 13), g.integers(16, N - 16, 13)
    if turned:
        img, x, y = np.ascontiguousarray(np.rot90(img)), y, N - 1 - x
    return img, dict(n_levels=1), x.astype(np.float32), y.astype(np.float32), None


SHIFT = (5, 3)   # the end-to-end pair: ramp_vga_k512 and the same image moved by 5 pixels in x and 3 in y
VGA = "ramp_vga_k512"


def shifted_image():
    return np.ascontiguousarray(np.roll(np.array(GR.image(VGA)), (SHIFT[1], SHIFT[0]), axis=(0, 1)))


def _vga_shifted():
    ref = GR.detect(shifted_image(), **GR.config(VGA))
    return shifted_image(), {}, ref["u"], ref["v"], ref["level"]


_BUILD = {
    "ramp_96x64_l3_k48_c16": lambda: _from_grid("ramp_96x64_l3_k48_c16", edge_threshold=16),
    "blocks_61x97_l3_k200_c16": lambda: _from_grid("blocks_61x97_l3_k200_c16", edge_threshold=16),
    "hand_40x40": _hand_40,
    "flat_48x48": lambda: (np.full((48, 48), 77, np.uint8), dict(n_levels=1), np.array([24, 16, 31], np.float32),
                           np.array([24, 31, 16], np.float32), None),
    "centre_33x33": lambda: (_noise(33, 33, 44), dict(n_levels=1), np.array([16], np.float32), np.array([16], np.float32),
                             np.array([0], np.int32)),
    "none_40x40": lambda: (_noise(40, 40, 41), dict(n_levels=1), np.zeros(0, np.float32), np.zeros(0, np.float32),
                           np.zeros(0, np.int32)),
    "quarter_64": lambda: _quarter(False),
    "quarter_64_turned": lambda: _quarter(True),
    VGA: lambda: _from_grid(VGA),
    "ramp_vga_k512_shifted": _vga_shifted,
}
NAMES = tuple(_BUILD)
SMALL = tuple(n for n in NAMES if "vga" not in n)


@functools.lru_cache(maxsize=None)
def fixture(name):
    """(image, config as DescriptorConfig's n_levels / scale_num / scale_den, u, v, level), all left unchanged."""
    img, over, u, v, level = _BUILD[name]()
    cfg = dict(n_levels=8, scale_num=6, scale_den=5)
    cfg.update(over)
    for a in (img, u, v) + (() if level is None else (level,)):
        a.setflags(write=False)
    return img, cfg, u, v, level


@functools.lru_cache(maxsize=None)
def expected(name):
    img, cfg, u, v, level = fixture(name)
    ref = describe(img, u, v, level, **cfg)
    for a in ref.values():
        a.setflags(write=False)
    _check_condition(name, ref)
    return ref


def _on_margin(name, ref):
    """Rows whose level pixel is exactly on D1's margin, on any side."""
    img, cfg, u, v, level = fixture(name)
    sizes = PR.level_sizes(img.shape[1], img.shape[0], cfg["n_levels"], cfg["scale_num"], cfg["scale_den"])
    lv = np.zeros(len(u), int) if level is None else level
    return sum(1 for i in range(len(u)) if ref["angle_bin"][i] >= 0 and
               (ref["x"][i] in (MARGIN, sizes[lv[i]][0] - MARGIN - 1) or ref["y"][i] in (MARGIN, sizes[lv[i]][1] - MARGIN - 1)))


def _check_condition(name, ref):
    img, cfg, u, v, level = fixture(name)
    valid = ref["angle_bin"] >= 0
    assert (ref["desc"][~valid] == 0).all() and np.isnan(ref["angle"][~valid]).all(), name
    if name in ("ramp_96x64_l3_k48_c16", "blocks_61x97_l3_k200_c16", VGA, "ramp_vga_k512_shifted"):
        # a detector with edge_threshold >= 16 emits no invalid row; every level is there
        assert valid.all() and len(u) > 0, name
        assert sorted(set(level.tolist())) == list(range(cfg["n_levels"])), (name, set(level.tolist()))
        assert len(set(ref["angle_bin"].tolist())) >= 8, name   # the bins are spread
    if name == "ramp_96x64_l3_k48_c16":
        assert len(u) == 48 and _on_margin(name, ref) >= 1, (name, len(u), _on_margin(name, ref))
    if name == "blocks_61x97_l3_k200_c16":
        assert img.shape[:2] == (97, 61) and len(u) % 4 != 0 and _on_margin(name, ref) >= 1, (name, len(u))
    if name == "hand_40x40":
        assert valid.tolist() == [False, True, True, False, False, False, False, True, True, False], (name, valid)
        assert len(u) % 4 != 0
    if name == "flat_48x48":
        assert valid.all() and (ref["angle_bin"] == 0).all() and (ref["angle"] == 0).all() and (ref["desc"] == 0).all(), name
        assert (ref["m10"] == 0).all() and (ref["m01"] == 0).all()
    if name == "centre_33x33":
        assert img.shape == (33, 33) and valid.tolist() == [True] and ref["desc"].any(), name
    if name == "none_40x40":
        assert ref["desc"].shape == (0, 32), name
    if name.startswith("quarter_64"):
        assert valid.all() and len(u) == 13 and not ref["tie"].any(), (name, ref["tie"])
        assert len(set(ref["angle_bin"].tolist())) >= 6, name
    if name == VGA:
        assert len(u) == 512, name


# ---- the end-to-end pair

# Of the 512 keypoints of ramp_vga_k512, the restated match_filtered (the defaults of match_descriptors) against the
# shifted image pairs VGA_PAIRS; VGA_PAIRS_LEVEL0 of the pairs have both keypoints on level 0, and VGA_PAIRS_EXACT of
# those differ by exactly the shift.  Computed with this module alone on the CPU; the device must return the same
# pairs, so these are its figures as well.  The three level-0 pairs that miss the shift are keypoints whose partner the
# detector did not keep in the other image (the cells of the grid do not move with the picture); their nearest
# row is another corner of the block pattern with the same brightness order, at distances 11, 14 and 16.
VGA_PAIRS, VGA_PAIRS_LEVEL0, VGA_PAIRS_EXACT = 241, 81, 78
VGA_UNMATCHED_CAP = 512 - VGA_PAIRS   # at most this many of the 512 keypoints stay without a partner


@functools.lru_cache(maxsize=None)
def vga_pair_matches():
    """(idx_a, idx_b, dist, both0, exact): the restated pairs, which of them have both keypoints on level 0 and which
    differ by exactly SHIFT in level-0 pixels."""
    a, b = expected(VGA), expected("ramp_vga_k512_shifted")
    ia, ib, dist = match_filtered(a, b)
    fa, fb = fixture(VGA), fixture("ramp_vga_k512_shifted")
    both0 = (fa[4][ia] == 0) & (fb[4][ib] == 0)
    exact = (fb[2][ib] - fa[2][ia] == SHIFT[0]) & (fb[3][ib] - fa[3][ia] == SHIFT[1])
    got = (len(ia), int(both0.sum()), int((both0 & exact).sum()))
    assert got == (VGA_PAIRS, VGA_PAIRS_LEVEL0, VGA_PAIRS_EXACT), got
    assert 512 - len(ia) <= VGA_UNMATCHED_CAP and both0.sum() >= 1
    return ia, ib, dist, both0, exact


# The same pair through the pyramid detector (the fixture's fields it has, max_keypoints 512), whose choice on level 0
# moves with the picture -- the quota's best responses, no cells -- so that every level-0 keypoint away from the frame
# has its partner: 290 pairs, 112 of them on level 0, and all 112 differ by exactly the shift.
VGA_PYRAMID_PAIRS, VGA_PYRAMID_LEVEL0 = 290, 112
VGA_PYRAMID_UNMATCHED_CAP = 512 - VGA_PYRAMID_PAIRS   # at most this many of the 512 keypoints stay without a partner


@functools.lru_cache(maxsize=None)
def vga_pyramid_pair():
    """(ra, rb, idx_a, idx_b, dist): the pyramid restatement's keypoints of both images and the restated pairs."""
    cfg = {k: v for k, v in GR.config(VGA).items() if k in PR.DEFAULTS}
    a_img, b_img = np.array(GR.image(VGA)), shifted_image()
    ra, rb = PR.detect(a_img, **cfg), PR.detect(b_img, **cfg)
    a, b = (describe(i, r["u"], r["v"], r["level"]) for i, r in ((a_img, ra), (b_img, rb)))
    ia, ib, dist = match_filtered(a, b)
    both0 = (ra["level"][ia] == 0) & (rb["level"][ib] == 0)
    exact = (rb["u"][ib] - ra["u"][ia] == SHIFT[0]) & (rb["v"][ib] - ra["v"][ia] == SHIFT[1])
    assert (len(ia), int(both0.sum()), int((both0 & exact).sum())) == (VGA_PYRAMID_PAIRS, VGA_PYRAMID_LEVEL0, VGA_PYRAMID_LEVEL0)
    assert len(ra["u"]) == 512 and 512 - len(ia) <= VGA_PYRAMID_UNMATCHED_CAP and both0.sum() >= 1
    return ra, rb, ia, ib, dist


# ---- matcher fixtures: name -> (q, t, q_bin or None, t_bin or None)

def _rows(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, 32), dtype=np.uint8)


def _flip(rows, seed, bits):
    """rows with up to `bits` random bits flipped in each."""
    g = np.random.default_rng(seed)
    out = rows.copy()
    for r in out:
        for b in g.integers(0, 256, bits):
            r[b // 8] ^= np.uint8(1 << (b % 8))
    return out


def _m_257x513():
    t = _rows(513, 51)
    pick = np.random.default_rng(52).integers(0, 513, 257)
    pick[0] = 512   # the only row of the last chunk
    return _flip(t[pick], 53, 20), t, None, None


def _m_dup():
    base = _rows(300, 54)
    base[1::2] = base[0::2]            # every row twice side by side (one chunk of train rows, mostly one tile) ...
    t = np.concatenate([base, base])   # ... and again 300 rows on, in another chunk
    return _flip(base, 55, 10), t, None, None


def _m_invalid():
    q, t = _rows(70, 56), _rows(140, 57)
    t[100:] = q[:40]   # exact partners, some of them invalid
    g = np.random.default_rng(58)
    q_bin, t_bin = g.integers(-1, 32, 70).astype(np.int32), g.integers(-1, 32, 140).astype(np.int32)
    q_bin[:3], t_bin[100:103] = (-1, 5, -1), (7, -1, -1)
    return q, t, q_bin, t_bin


def _m_self():
    q = _rows(300, 59)
    b = np.random.default_rng(60).integers(-1, 32, 300).astype(np.int32)
    return q, q, b, b


_MATCH = {
    "1x1": lambda: (_rows(1, 61), _rows(1, 62), None, None),
    "3x0": lambda: (_rows(3, 63), np.zeros((0, 32), np.uint8), None, None),
    "0x3": lambda: (np.zeros((0, 32), np.uint8), _rows(3, 64), None, None),
    "257x513": _m_257x513,
    "duplicates": _m_dup,
    "invalid_rows": _m_invalid,
    "self": _m_self,
    "none_valid": lambda: (_rows(5, 65), _rows(4, 66), None, np.full(4, -1, np.int32)),
}
MATCH_NAMES = tuple(_MATCH)


@functools.lru_cache(maxsize=None)
def match_fixture(name):
    out = _MATCH[name]()
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def match_expected(name):
    q, t, q_bin, t_bin = match_fixture(name)
    idx, dist, dist2 = match(q, t, q_bin, t_bin)
    for a in (idx, dist, dist2):
        a.setflags(write=False)
    n_q = len(q)
    if name == "1x1":
        assert idx.tolist() == [0] and dist2.tolist() == [NONE] and 0 < dist[0] < 256
    if name in ("3x0", "none_valid"):
        assert (idx == -1).all() and (dist == NONE).all() and (dist2 == NONE).all() and n_q > 0
    if name == "0x3":
        assert n_q == 0
    if name == "257x513":   # workgroups of 64 queries and a partial one, chunks of 128 train rows and one of a single row
        assert n_q == 257 and len(t) == 513 and (dist <= 20).all() and (idx >= 384).any() and (idx < 128).any()
        assert (idx == 512).any()   # the last chunk's only row is somebody's nearest
        assert len(set(idx.tolist())) > 100
    if name == "duplicates":   # the nearest row exists four times: the lowest index wins, dist2 = dist
        assert (idx == np.arange(300) // 2 * 2).all() and (dist2 == dist).all() and (dist > 0).any()
    if name == "invalid_rows":
        assert idx[0] == idx[2] == -1 and dist[0] == NONE and (q_bin < 0).sum() >= 3 and (t_bin < 0).sum() >= 3
        assert idx[1] != 101 and dist[1] > 0   # its exact partner is invalid
        ok = (q_bin >= 0) & (np.arange(70) < 40) & (t_bin[100 + np.clip(np.arange(70), 0, 39)] >= 0)
        assert ok.sum() > 10 and (idx[ok] == 100 + np.arange(70)[ok]).all() and (dist[ok] == 0).all()
        assert (t_bin[idx[idx >= 0]] >= 0).all()
    if name == "self":
        v = q_bin >= 0
        assert (idx[v] == np.arange(300)[v]).all() and (dist[v] == 0).all() and (idx[~v] == -1).all() and (~v).sum() > 3
        assert (dist2[v] > 60).all()
    return idx, dist, dist2
