"""A numpy restatement of the gated matcher's and the pairs' definition (include/gcslam_hip.h, "keypoint
descriptors", D8 and D9) and the fixtures of tests/test_keypoints_gate_host.py and tests/test_gpu_keypoints_gate.py.
Written from the definition on tests/keypoints_desc_ref.py (imported, not edited): the descriptors, the Hamming
distances' convention and the end-to-end pair are that module's.  Every fixture asserts its own condition where it is
built, so a fixture that stops exercising its case fails here and not silently.

A gate is a dict of q_u, q_v, q_level, t_u, t_v, t_level, q_pu, q_pv (arrays or None), radius and max_level_diff;
None is no gate."""

import functools

import numpy as np

import keypoints_desc_ref as DR

NONE = DR.NONE
PAIR_BLOCK = 256   # kPcThreads of gc-slam_amd/csrc/gcs_descriptors.hip: the query rows one compaction workgroup covers
FILTERS = (dict(), dict(cross_check=False), dict(ratio=None), dict(max_distance=256))


def gate_of(q_u=None, q_v=None, q_level=None, t_u=None, t_v=None, t_level=None, q_pu=None, q_pv=None, radius=16.0,
            max_level_diff=1):
    return dict(q_u=q_u, q_v=q_v, q_level=q_level, t_u=t_u, t_v=t_v, t_level=t_level, q_pu=q_pu, q_pv=q_pv,
                radius=radius, max_level_diff=max_level_diff)


# ---- D8

def distances(q, t):
    """(n_q, n_t) int64 Hamming distances."""
    q, t = np.asarray(q, np.uint8).reshape(-1, 32), np.asarray(t, np.uint8).reshape(-1, 32)
    d = np.zeros((len(q), len(t)), np.int64)
    for lo in range(0, len(q), 64):
        d[lo:lo + 64] = np.unpackbits(q[lo:lo + 64, None, :] ^ t[None, :, :], axis=2).sum(2)
    return d


def candidates(n_q, n_t, gate=None, q_bin=None, t_bin=None):
    """C(i, j) as an (n_q, n_t) bool matrix."""
    qv = np.ones(n_q, bool) if q_bin is None else np.asarray(q_bin) >= 0
    tv = np.ones(n_t, bool) if t_bin is None else np.asarray(t_bin) >= 0
    C = qv[:, None] & tv[None, :]
    if gate is None:
        return C
    pu = np.asarray(gate["q_u"] if gate["q_pu"] is None else gate["q_pu"], np.float32)
    pv = np.asarray(gate["q_v"] if gate["q_pv"] is None else gate["q_pv"], np.float32)
    tu, tv_ = np.asarray(gate["t_u"], np.float32), np.asarray(gate["t_v"], np.float32)
    ql = np.zeros(n_q, np.int64) if gate["q_level"] is None else np.asarray(gate["q_level"], np.int64)
    tl = np.zeros(n_t, np.int64) if gate["t_level"] is None else np.asarray(gate["t_level"], np.int64)
    r = np.float32(gate["radius"])
    with np.errstate(invalid="ignore"):   # inf - inf; a NaN compares false
        du, dv = tu[None, :] - pu[:, None], tv_[None, :] - pv[:, None]   # one float32 subtraction each
        assert du.dtype == np.float32 and dv.dtype == np.float32
        C = C & (np.abs(du) <= r) & (np.abs(dv) <= r)
    return C & (np.abs(tl[None, :] - ql[:, None]) <= int(gate["max_level_diff"]))


def _search(d, C):
    """idx, dist, dist2, n_cand of every row of d over the columns C allows: the minimum over (distance, index)."""
    n = d.shape[0]
    idx, dist, dist2 = np.full(n, -1, np.int32), np.full(n, NONE, np.int32), np.full(n, NONE, np.int32)
    n_cand = C.sum(1).astype(np.int32)
    if d.shape[1] == 0:
        return idx, dist, dist2, n_cand
    e = np.where(C, d, NONE)
    best = np.argmin(e, axis=1)   # the first of the smallest: ties to the lowest index
    rows = np.arange(n)
    has = n_cand > 0
    idx[has], dist[has] = best[has], e[rows, best][has]
    e[rows, best] = NONE
    dist2[has] = e.min(axis=1)[has]
    return idx, dist, dist2, n_cand


def match_gated(q, t, gate=None, q_bin=None, t_bin=None, d=None):
    """(idx, dist, dist2, n_cand), int32, of every query row; d: distances(q, t) where the caller has them."""
    d = distances(q, t) if d is None else d
    return _search(d, candidates(d.shape[0], d.shape[1], gate, q_bin, t_bin))


def match_backward(q, t, gate=None, q_bin=None, t_bin=None, d=None):
    """The backward search: for every train row j the query row i with C(i, j) of least (distance, i), or -1."""
    d = distances(q, t) if d is None else d
    return _search(d.T.copy(), candidates(d.shape[0], d.shape[1], gate, q_bin, t_bin).T)[0]


# ---- D9

def pairs(q, t, gate=None, q_bin=None, t_bin=None, max_distance=64, ratio=(4, 5), cross_check=True, d=None):
    """(pair_a, pair_b, pair_dist, count): the padded arrays of n_query entries and the count as a one-entry array."""
    d = distances(q, t) if d is None else d
    idx, dist, dist2, _ = match_gated(q, t, gate, q_bin, t_bin, d)
    n = len(idx)
    keep = idx >= 0
    if max_distance is not None:
        keep &= dist <= max_distance
    if ratio is not None:
        keep &= dist.astype(np.int64) * int(ratio[1]) < int(ratio[0]) * dist2.astype(np.int64)
    if cross_check:
        back = match_backward(q, t, gate, q_bin, t_bin, d)
        keep &= (back[np.clip(idx, 0, None)] == np.arange(n)) if len(back) else False
    at = np.nonzero(keep)[0]
    a, b, pd = np.full(n, -1, np.int32), np.full(n, -1, np.int32), np.full(n, NONE, np.int32)
    a[:len(at)], b[:len(at)], pd[:len(at)] = at, idx[at], dist[at]
    return a, b, pd, np.array([len(at)], np.int32)


def _frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
        elif isinstance(a, dict):
            _frozen(*a.values())
    return arrays


# ---- gated fixtures: name -> (q, t, q_bin, t_bin, gate)

def _g_257x513():
    q, t, _, _ = DR.match_fixture("257x513")
    pick = np.random.default_rng(52).integers(0, 513, 257)   # DR._m_257x513's choice of rows
    pick[0] = 512
    g = np.random.default_rng(71)
    tp = (g.random((513, 2)) * 200).astype(np.float32)
    tp[512] = (230.0, 40.0)   # the last chunk's only row, away from the others: query 0's only candidate
    qp = (tp[pick] + g.uniform(-12, 12, (257, 2)).astype(np.float32)).astype(np.float32)
    qp[0] = (236.0, 37.0)
    tl = g.integers(0, 3, 513).astype(np.int32)
    return q, t, None, None, gate_of(qp[:, 0].copy(), qp[:, 1].copy(), tl[pick].copy(), tp[:, 0].copy(), tp[:, 1].copy(), tl,
                                     radius=8.0, max_level_diff=1)


F8 = np.float32(np.nextafter(np.float32(8), np.float32(np.inf)))
_EDGE_Q = dict(   # six query rows
    u=[0, 50, np.nan, 0, 0, np.inf], v=[0, 50, 0, 0, 0, 0], level=[1, 0, 1, 1, 1, 1], bin=[3, 3, 3, -1, 3, 3],
    pu=[0, 58, 0, 0, np.nan, 0], pv=[0, 50, 0, 0, 0, 0])
_EDGE_T = dict(   # eleven train rows
    u=[8, F8, -8, 0, 3, 3, 3, np.nan, np.inf, 50, 0], v=[0, 0, 0, -F8, 3, 3, 3, 3, 0, 50, 0],
    level=[1, 1, 1, 1, 2, 3, 1, 1, 1, 0, 0], bin=[0, 0, 0, 0, 0, 0, -1, 0, 0, 0, 0])
# The candidate matrices by hand (rows: queries, columns: train rows).  Radius 8, level diff 1, null prediction:
# query 0 at (0, 0) on level 1 takes |du| = 8 on both sides (rows 0, 2), not nextafter(8) in u (1) or in v (3), level 2
# (4) but not level 3 (5), not the invalid row (6), the NaN row (7) or the infinite one (8), and the row on its own
# place one level down (10); query 1 its own place (9); the NaN, invalid and infinite queries (2, 3, 5) nothing; query
# 4 is query 0 again.
_E = lambda *on: [1 if j in on else 0 for j in range(11)]   # noqa: E731
EDGE_CANDIDATES = {
    "edges": [_E(0, 2, 4, 10), _E(9), _E(), _E(), _E(0, 2, 4, 10), _E()],
    # the prediction given: query 1 expected at (58, 50), so that row 9 is at du = -8 exactly; query 4's is NaN; query
    # 2's position is NaN but its prediction (0, 0) is not, so it sees what query 0 sees
    "edges_predicted": [_E(0, 2, 4, 10), _E(9), _E(0, 2, 4, 10), _E(), _E(), _E(0, 2, 4, 10)],
    # radius 0: equal positions only
    "edges_radius0": [_E(10), _E(9), _E(), _E(), _E(10), _E()],
    # null level arrays: every row on level 0, so row 5 comes in
    "edges_no_levels": [_E(0, 2, 4, 5, 10), _E(9), _E(), _E(), _E(0, 2, 4, 5, 10), _E()],
    # level diff 0: query 0 (level 1) loses rows 4 (level 2) and 10 (level 0)
    "edges_level0": [_E(0, 2), _E(9), _E(), _E(), _E(0, 2), _E()],
}


def _g_edges(name):
    f32, i32 = (lambda x: np.array(x, np.float32)), (lambda x: np.array(x, np.int32))
    q, t = DR._rows(6, 72), DR._rows(11, 73)
    lv = name != "edges_no_levels"
    pred = name == "edges_predicted"
    gate = gate_of(f32(_EDGE_Q["u"]), f32(_EDGE_Q["v"]), i32(_EDGE_Q["level"]) if lv else None, f32(_EDGE_T["u"]),
                   f32(_EDGE_T["v"]), i32(_EDGE_T["level"]) if lv else None, f32(_EDGE_Q["pu"]) if pred else None,
                   f32(_EDGE_Q["pv"]) if pred else None, radius=0.0 if name == "edges_radius0" else 8.0,
                   max_level_diff=0 if name == "edges_level0" else 1)
    return q, t, i32(_EDGE_Q["bin"]), i32(_EDGE_T["bin"]), gate


def _g_predicted():
    """36 train rows 40 pixels apart; every query is a flipped copy of one of them, seen where the row was before a
    motion that differs row to row and exceeds the radius.  Queries 36 and 37 are further copies of the rows of
    queries 0 and 1 with more bits flipped, predicted onto the same places."""
    g = np.random.default_rng(74)
    t = DR._rows(36, 75)
    tp = np.stack([40.0 * (np.arange(36) % 6) + 20, 40.0 * (np.arange(36) // 6) + 20], 1).astype(np.float32)
    src = np.concatenate([g.permutation(36), [0, 0]])
    src[36], src[37] = src[0], src[1]
    q = DR._flip(t[src], 76, 8)
    q[36:] = DR._flip(t[src[36:]], 77, 40)
    k = np.arange(38)
    motion = np.stack([10.0 + k % 7, -9.0 - k % 5], 1).astype(np.float32)
    qp = (tp[src] - motion).astype(np.float32)
    pred = (qp + motion).astype(np.float32)
    return q, t, None, None, gate_of(qp[:, 0].copy(), qp[:, 1].copy(), None, tp[:, 0].copy(), tp[:, 1].copy(), None,
                                     pred[:, 0].copy(), pred[:, 1].copy(), radius=8.0), src


def _g_ties():
    q, t, _, _ = DR.match_fixture("duplicates")
    one = lambda n: np.full(n, 10.0, np.float32)   # noqa: E731
    return q, t, None, None, gate_of(one(300), one(300), None, one(600), one(600), None, radius=8.0)


_GATED = {
    "gate_257x513": _g_257x513,
    **{n: functools.partial(_g_edges, n) for n in EDGE_CANDIDATES},
    "predicted": lambda: _g_predicted()[:5],
    "predicted_null": lambda: (lambda f: f[:4] + (dict(f[4], q_pu=None, q_pv=None),))(_g_predicted()),
    "ties": _g_ties,
}
GATED_NAMES = tuple(_GATED)


@functools.lru_cache(maxsize=None)
def gated_fixture(name):
    return _frozen(*_GATED[name]())


@functools.lru_cache(maxsize=None)
def gated_expected(name):
    q, t, q_bin, t_bin, gate = gated_fixture(name)
    idx, dist, dist2, n_cand = _frozen(*match_gated(q, t, gate, q_bin, t_bin))
    if name == "gate_257x513":
        free = DR.match_expected("257x513")[0]
        C = candidates(257, 513, gate)
        assert (n_cand == 0).any() and (idx[n_cand == 0] == -1).all() and (dist[n_cand == 0] == NONE).all()
        assert (n_cand == 1).any() and (dist2[n_cand == 1] == NONE).all() and (dist[n_cand == 1] < NONE).all()
        assert (n_cand > 2).any()
        assert (~C[np.arange(257), free]).any() and ((idx != free) & (idx >= 0)).any()   # the gate changes idx
        assert n_cand[0] == 1 and idx[0] == 512 and C[0].nonzero()[0].tolist() == [512]   # only the last chunk's row
    if name in EDGE_CANDIDATES:
        C = candidates(6, 11, gate, q_bin, t_bin)
        assert C.astype(int).tolist() == EDGE_CANDIDATES[name], (name, C.astype(int).tolist())
        assert n_cand.tolist() == [sum(r) for r in EDGE_CANDIDATES[name]]
        assert float(F8) > 8.0 and float(F8) - 8.0 < 1e-6
    if name == "predicted":
        src = _g_predicted()[5]
        null = gated_expected("predicted_null")
        assert (null[3] == 0).all() and (null[0] == -1).all()   # the motion exceeds the radius: nothing without the prediction
        assert (idx == src).all() and (n_cand == 1).all()
        back = match_backward(q, t, gate)
        assert back[src[36]] == 0 and back[src[37]] == 1   # rows 36 and 37 chose them forward and lose them backward
        assert pairs(q, t, gate)[3][0] == 36 and pairs(q, t, gate, cross_check=False)[3][0] == 38
    if name == "ties":
        assert (idx == np.arange(300) // 2 * 2).all() and (dist2 == dist).all() and (n_cand == 600).all()
        assert DR.match_expected("duplicates")[0].tobytes() == idx.tobytes()
    return idx, dist, dist2, n_cand


# ---- pairs fixtures: name -> (q, t, q_bin, t_bin, gate)

def _p_build(n_q, n_t, seed, spoil=True):
    """q: flipped copies (10 bits) of a permutation's rows of t, seen within 6 pixels of the row's place and on its
    level.  With spoil, in every 64 query rows: row 5 is invalid, row 17 differs from its train row in exactly 70 bits (beyond max_distance, within the ratio),
    row 40 is a second, worse copy of row 39's train row (the cross check drops it), row 29 lies 20 pixels off (outside
    the gate) and row 50 two levels off."""
    g = np.random.default_rng(seed)
    t = DR._rows(n_t, seed + 1)
    src = g.permutation(n_t)[:n_q] if n_q <= n_t else g.integers(0, n_t, n_q)
    k = np.arange(n_q) % 64
    on = lambda r: (k == r) & spoil & (np.arange(n_q) >= r)   # noqa: E731
    if n_q > 1:
        src[on(40)] = src[np.nonzero(on(40))[0] - 1]
    q = DR._flip(t[src], seed + 2, 10)
    far, worse = t[src].copy(), DR._flip(t[src], seed + 4, 30)
    far[:, :8] ^= np.uint8(0xFF)
    far[:, 8] ^= np.uint8(0x3F)
    q[on(17)], q[on(40)] = far[on(17)], worse[on(40)]
    q_bin = np.where(on(5), -1, 7).astype(np.int32)
    t_bin = np.full(n_t, 9, np.int32)
    tp = (g.random((n_t, 2)) * 400).astype(np.float32)
    qp = (tp[src] + g.uniform(-6, 6, (n_q, 2)).astype(np.float32)).astype(np.float32)
    qp[on(29), 0] += np.float32(20)
    tl = g.integers(0, 4, n_t).astype(np.int32)
    ql = tl[src].copy()
    ql[on(50)] += 2
    return q, t, q_bin, t_bin, gate_of(qp[:, 0].copy(), qp[:, 1].copy(), ql, tp[:, 0].copy(), tp[:, 1].copy(), tl, radius=8.0)


_PAIRS = {
    "pairs_1x1": lambda: _p_build(1, 1, 80),
    "pairs_63x70": lambda: _p_build(63, 70, 81),
    "pairs_64x64": lambda: _p_build(64, 64, 82),
    "pairs_65x129": lambda: _p_build(65, 129, 83),
    "pairs_256x300": lambda: _p_build(PAIR_BLOCK, 300, 84),       # exactly one compaction workgroup
    "pairs_257x300": lambda: _p_build(PAIR_BLOCK + 1, 300, 85),   # one row into the second
    "pairs_1100x1100": lambda: _p_build(1100, 1100, 86),
    "pairs_all_70x70": lambda: _p_build(70, 70, 87, spoil=False),
    "pairs_none_70x70": lambda: (lambda f: f[:2] + (np.full(70, -1, np.int32),) + f[3:])(_p_build(70, 70, 88)),
    "pairs_3x0": lambda: _p_build(3, 3, 89)[:1] + (np.zeros((0, 32), np.uint8), None, None, None),
    "pairs_0x3": lambda: (np.zeros((0, 32), np.uint8),) + _p_build(3, 3, 90)[1:2] + (None, None, None),
}
PAIRS_NAMES = tuple(_PAIRS)


@functools.lru_cache(maxsize=None)
def pairs_fixture(name):
    return _frozen(*_PAIRS[name]())


def pairs_cases(name):
    """The (gated, filter arguments) combinations a fixture is run with."""
    gates = (False, True) if pairs_fixture(name)[4] is not None else (False,)
    return [(gated, kw) for gated in gates for kw in FILTERS]


@functools.lru_cache(maxsize=None)
def _pairs_distances(name):
    return _frozen(distances(*pairs_fixture(name)[:2]))[0]


@functools.lru_cache(maxsize=None)
def _pairs_expected(name, gated, case):
    q, t, q_bin, t_bin, gate = pairs_fixture(name)
    return _frozen(*pairs(q, t, gate if gated else None, q_bin, t_bin, d=_pairs_distances(name), **FILTERS[case]))


def pairs_expected(name, gated, kw):
    out = _pairs_expected(name, bool(gated), FILTERS.index(kw))
    _check_pairs(name)
    return out


@functools.lru_cache(maxsize=None)
def _check_pairs(name):
    q = pairs_fixture(name)[0]
    n_q = len(q)
    counts = {(g, c): int(_pairs_expected(name, g, c)[3][0]) for g, kw in pairs_cases(name) for c in [FILTERS.index(kw)]}
    for (g, c), n in counts.items():
        a, b, d, _ = _pairs_expected(name, g, c)
        assert (a[n:] == -1).all() and (b[n:] == -1).all() and (d[n:] == NONE).all() and (np.diff(a[:n]) > 0).all()
    if name in ("pairs_65x129", "pairs_256x300", "pairs_257x300", "pairs_1100x1100"):
        assert all(0 < n < n_q for n in counts.values()), (name, counts)
        assert counts[(True, 0)] < counts[(False, 0)] < counts[(False, 1)], (name, counts)   # the gate and the cross check each drop something
        assert counts[(False, 0)] < counts[(False, 3)], (name, counts)   # and so does max_distance
        for g in (False, True):
            kept = np.zeros(n_q, bool)
            kept[_pairs_expected(name, g, 0)[0][:counts[(g, 0)]]] = True
            for edge in range(64, n_q, 64):
                assert kept[edge - 1] and kept[edge], (name, g, edge)
    if name == "pairs_all_70x70":
        assert counts[(False, 0)] == n_q == 70 and counts[(True, 0)] == 70, counts
    if name in ("pairs_none_70x70", "pairs_3x0", "pairs_0x3"):
        assert set(counts.values()) == {0}, counts
    if name == "pairs_1x1":
        assert counts[(False, 0)] == 1
    return True


# ---- the end-to-end pair

# ramp_vga_k512 and the same frame moved by (5, 3), through `pairs` with radius 8, level diff 1, a null prediction and
# the default filters: (pairs, pairs with both keypoints on level 0, those of them that differ by exactly the shift).
# Computed with this module alone on the CPU; the device must return the same pairs, so these are its figures as well.
# The four level-0 grid pairs that miss the shift are keypoints whose partner the grid did not keep: the window bounds
# their error to its radius and does not remove them.
VGA_GATE = dict(radius=8.0, max_level_diff=1)
VGA_GATED_PYRAMID = (305, 112, 112)
VGA_GATED_GRID = (284, 82, 78)


def _vga_check(ua, va, la, ub, vb, lb, got, want, ungated):
    a, b, d, count = got
    n = int(count[0])
    ia, ib = a[:n], b[:n]
    both0 = (la[ia] == 0) & (lb[ib] == 0)
    du, dv = ub[ib] - ua[ia], vb[ib] - va[ia]
    exact = (du == DR.SHIFT[0]) & (dv == DR.SHIFT[1])
    assert (n, int(both0.sum()), int((both0 & exact).sum())) == want, (n, int(both0.sum()), int((both0 & exact).sum()))
    assert 512 - n <= 512 - want[0]   # no more keypoints stay without a partner than here
    assert (np.abs(du) <= VGA_GATE["radius"]).all() and (np.abs(dv) <= VGA_GATE["radius"]).all()   # every pair, on any level
    assert (np.abs(lb[ib] - la[ia]) <= VGA_GATE["max_level_diff"]).all()
    assert n >= ungated


@functools.lru_cache(maxsize=None)
def vga_pyramid_gated():
    """(a, b, gate, pairs): describe's dicts of both images' pyramid keypoints, the gate and the restated pairs."""
    ra, rb = DR.vga_pyramid_pair()[:2]
    import keypoints_grid_ref as GR
    a_img, b_img = np.array(GR.image(DR.VGA)), DR.shifted_image()
    a, b = (DR.describe(i, r["u"], r["v"], r["level"]) for i, r in ((a_img, ra), (b_img, rb)))
    gate = gate_of(ra["u"], ra["v"], ra["level"], rb["u"], rb["v"], rb["level"], **VGA_GATE)
    got = _frozen(*pairs(a["desc"], b["desc"], gate, a["angle_bin"], b["angle_bin"]))
    _vga_check(ra["u"], ra["v"], ra["level"], rb["u"], rb["v"], rb["level"], got, VGA_GATED_PYRAMID, DR.VGA_PYRAMID_PAIRS)
    assert VGA_GATED_PYRAMID[0] >= DR.VGA_PYRAMID_PAIRS == 290
    return a, b, gate, got


@functools.lru_cache(maxsize=None)
def vga_grid_gated():
    """The same through the grid detector's keypoints (DR.fixture's and DR.expected's)."""
    a, b = DR.expected(DR.VGA), DR.expected("ramp_vga_k512_shifted")
    fa, fb = DR.fixture(DR.VGA), DR.fixture("ramp_vga_k512_shifted")
    gate = gate_of(fa[2], fa[3], fa[4], fb[2], fb[3], fb[4], **VGA_GATE)
    got = _frozen(*pairs(a["desc"], b["desc"], gate, a["angle_bin"], b["angle_bin"]))
    _vga_check(fa[2], fa[3], fa[4], fb[2], fb[3], fb[4], got, VGA_GATED_GRID, DR.VGA_PAIRS)
    return a, b, gate, got
