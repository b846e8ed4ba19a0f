"""Primitive-map test kit: seeded tile builders (numpy), the restated dispatch of gc-slam_amd/csrc/gcs_pmap.hip
(sort_tiles, fuse_blocks), the case tables of the shape sweep with their guards, and the comparison of a device
result with the numpy oracle (oracle/primitive_map.py).

Shared by tests/test_pmap_shapes.py (CPU: every case is built, its guards run on the inputs and the oracle's
outputs alone, so a case is known to reach its branch before it reaches a GPU), tests/test_gpu_primitive_map.py
(the tile builder), tests/test_gpu_pmap_select_shapes.py and tests/test_gpu_pmap_fuse_shapes.py.  Nothing here
imports torch or the device library at module level.

Bars (none set from a device result): the select cases are exact -- slots, ids, masks, integer fields, weights and,
after an insert, every field of every tile bitwise; view positions at rtol = atol = 1e-12 (LU rounding).  The fuse
cases run step 12b: counts and ids equal, mass statistics at rel 1e-12, tiles at rtol 1e-11 (the world transform's
so3_exp / LU rounding and, for runs of more than 32 rows, the wave's summation order) -- the suite's existing
step-12b bars.

Weights: no NaN and none <= -1e30.  numpy's stable argsort puts NaN last whatever its sign and the oracle's
invalid-slot score -1e30 would tie with such a weight, while the device orders the keys by their bits; the map
never holds either (weights are sums of non-negative masses).
"""

from __future__ import annotations

import functools
import os
import sys
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "gc-slam_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle import primitive_map as opm  # noqa: E402
from oracle import se3  # noqa: E402

# The switch points of gcs_pmap.hip, named once (sort_tiles / k_pm_topk / k_pm_topk_sparse / k_pm_select_reg):
TOP_CHUNK = 4096     # kTopChunk: slots per leaf of the tree of sorted runs (k_pm_topk)
SP_MAX = 2048        # kSpMax: entries besides the empty slots that k_pm_topk_sparse sorts itself
REG_MAX = 8192       # 8 * kPmRed: the register select's tile size (k_pm_select_reg<8, 1024>)
SEL_MAX = 1024       # kSelMax: the largest k of the select / tree; above it the rocPRIM full sort
SP_BITS = 65536      # 32 * kSpWords: the largest tile whose bitmap k_pm_topk_sparse reads
TOP_MAX_LEAVES = 128  # 1 << (kTopMaxLevels - 1)
# fuse_blocks / k_ss_block / k_ss_merge / k_pm_fuse_runs:
SS_RUN = 1024        # kSsRun: rows per sorted run
SS_MAX = 16384       # kSsMax: one LDS group of 16 runs
SS_WIDE_MAX = 65536  # kSsWideMax: four groups; above it rocPRIM's radix sort
FUSE_CHUNK = 32      # kFuseChunk: a (tile, slot, block) run longer than this is summed ahead by one wave
FUSE_THREADS = 256   # kPmThreads: positions per workgroup of k_pm_fuse_runs
MAX_FUSE_BLOCKS = 256  # kMaxFuseBlocks
NOKEY = 0xFFFFFFFF   # kNoKey

NL = 3
SCAN_SEQ = 41        # eviction cases: last_supported_scan_seq is drawn below it, so the decay varies
PATTERNS = ("random", "all_equal", "hiword_ties", "extremes")


# --------------------------------------------------------------------------------------------------
# tiles
# --------------------------------------------------------------------------------------------------

def rand_tile(rng, m=4096, frac=0.6, seq_hi=40, n_valid=None):
    """A tile with every field drawn: weights in [0, 2) with 10 % exact ties (0.5) and 5 % zeros, SPD Lambdas,
    camera mass on 30 % of the slots.  valid_mask: a Bernoulli(frac) draw, or with n_valid exactly that many
    slots chosen by permutation."""
    t = opm.create_empty_tile(m)
    if n_valid is None:
        v = rng.random(m) < frac
    else:
        v = np.zeros(m, bool)
        v[rng.permutation(m)[:int(n_valid)]] = True
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


def pattern_tile(rng, m, n_valid, pattern, k, mode):
    """rand_tile with exactly n_valid valid slots and the weights of `pattern`:
      random       as rand_tile
      all_equal    0.75 everywhere: slot order alone decides (and, in the eviction order, the decay)
      hiword_ties  a group of min(n_valid, k + 5) valid slots with weights 1 + j 2^-52 (one high key word, distinct
                   low words), shuffled over the slots; the other weights are multiples of 2^-6 (many exact ties),
                   k // 3 of the valid ones on the side of the group the order starts from (view: above 1,
                   eviction: below 1) so that the k-th entry falls inside the group.  Eviction: the tile's
                   last_supported_scan_seq is the scan's, so the decay is exactly 1 and the products keep their bits
      extremes     random with three valid slots each of 0.0, the smallest denormal, 1e300 and inf."""
    assert pattern in PATTERNS and mode in ("view", "evict")
    t = rand_tile(rng, m, n_valid=n_valid)
    vs = np.flatnonzero(t["valid_mask"])
    if pattern == "all_equal":
        t["weights"][:] = 0.75
    elif pattern == "hiword_ties":
        far = np.round(rng.random(m) * 60.0) / 64.0              # [0, 0.9375]: below the group
        near = 1.0 + (1.0 + np.round(rng.random(m) * 60.0)) / 64.0   # [1.016, 1.95]: above it
        first, rest = (near, far) if mode == "view" else (far, near)
        w = rest.copy()
        vs = rng.permutation(vs)
        g = min(len(vs), k + 5)
        a = min(k // 3, len(vs) - g)
        w[vs[:g]] = 1.0 + rng.permutation(g).astype(np.float64) * 2.0 ** -52
        w[vs[g:g + a]] = first[vs[g:g + a]]
        t["weights"][:] = w
        if mode == "evict":
            t["last_supported_scan_seq"][:] = SCAN_SEQ
    elif pattern == "extremes":
        sel = rng.permutation(vs)[:12]
        t["weights"][sel] = np.resize(np.array([0.0, 5e-324, 1e300, np.inf]), len(sel))
    w = t["weights"]
    assert not np.isnan(w).any() and (w > -1e30).all()
    return t


def ord_key(x):
    """ord_key of gcs_pmap.hip: ascending order of doubles as unsigned bits, -0.0 folded onto 0.0."""
    u = (np.asarray(x, np.float64) + 0.0).view(np.uint64)
    return np.where((u >> np.uint64(63)) != 0, ~u, u | np.uint64(1 << 63))


def tile_keys(t, mode, lam=opm.GC_RECENCY_DECAY_LAMBDA):
    """k_pm_keys' keys of a tile and the mode's empty-slot key."""
    if mode == "view":
        return ord_key(-np.where(t["valid_mask"], t["weights"], -1e30)), ord_key(1e30)
    dt = np.maximum(0, SCAN_SEQ - t["last_supported_scan_seq"]).astype(np.float64)
    with np.errstate(invalid="ignore"):
        ret = t["weights"] * np.exp(-lam * dt)
    return ord_key(np.where(t["valid_mask"], ret, -np.inf)), ord_key(-np.inf)


# --------------------------------------------------------------------------------------------------
# select cases (extract_atlas_map_view / primitive_map_insert_masked_tiles)
# --------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class TileSpec:
    n_valid: int
    pattern: str = "random"


@dataclass(frozen=True)
class SelectCase:
    id: str
    M: int
    k: int
    mode: str                                   # "view" | "evict"
    tiles: Tuple[Optional[TileSpec], ...]       # the call's tile list; None: an id the map does not hold
    seed: int


def select_path(M, k):
    """sort_tiles' choice with no knob set."""
    if not 1 <= k <= SEL_MAX:
        return "fullsort"
    if M <= REG_MAX:
        return "reg8"
    G = -(-M // TOP_CHUNK)
    if 1 < G <= TOP_MAX_LEAVES:
        return "tree+sparse" if M <= SP_BITS else "tree"
    return "radix"


def _select_cases():
    cases, seed = [], [1000]

    def add(M, k, mode, counts, patterns, tag=""):
        seed[0] += 1
        specs = []
        for c, p in zip(counts, patterns):
            specs.append(None if c is None else TileSpec(int(min(max(c, 0), M)), p if M >= 64 else "random"))
        assert 4 <= len(specs) <= 6 and None in specs[1:-1] and any(s is not None and s.n_valid == 0 for s in specs)
        cases.append(SelectCase(f"{mode}-M{M}-k{k}{tag}", M, k, mode, tuple(specs), seed[0]))

    P = ("hiword_ties", "extremes", "random", "all_equal", "random", "random")
    # the register select: M <= 8,192 (last register slot partly / fully used at 8,191 / 8,192), k from 1 to M
    for M, ks in ((1, (1,)), (2, (1, 2)), (1023, (1, 64, 1023)), (1024, (2, 1023, 1024)), (1025, (64, 1024)),
                  (8191, (1, 1023, 1024)), (8192, (2, 64, 1024))):
        for k in ks:
            # view: a full tile of high-word ties; eviction: the same with no empty slot, so the K lowest are chosen
            add(M, k, "view", (M, (3 * M) // 5, None, M // 3, 0, k + 1), P)
            add(M, k, "evict", (M, M - 1, None, M // 3, 0, M - k + 1), P)
    # the tree, the sparse pass and the full tile: view counts from {0, 1, k-1, k, k+1, 2047, 2048, 2049, M}
    big = (8193, 8209, 12289, 16384, 65535, 65536)
    small_menu = lambda k: (1, k - 1, k, k + 1)  # noqa: E731
    i = 0
    for M in big:
        for k in (1, 63, 1024):
            dense = (2049, M)[i % 2]
            edge = (2047, 2048)[(i // 2) % 2]
            lo = small_menu(k)[i % 4]
            pats = ("hiword_ties", "all_equal", "random", "extremes", "random", "hiword_ties")
            add(M, k, "view", (dense, edge, None, lo, 0, (M, 2049)[i % 2]), pats)
            i += 1
    # past the sparse pass: 17 leaves, every tile (the empty one too) on the tree
    for k in (1, 1024):
        add(65537, k, "view", (65537, 2048, None, 2049, 0, k + 1),
            ("hiword_ties", "random", "random", "all_equal", "random", "extremes"))
    # eviction: empty-slot counts 0 / K-1 / K / K+1 on tiles with more than 2,048 valid slots (the dense-tile
    # shortcut from K on), a sparse tile, an empty one; all_equal tiles draw last_supported_scan_seq below the
    # scan's, so the decay alone orders them
    for j, (M, K) in enumerate(((8193, 1024), (8209, 1), (8209, 64), (8209, 1024), (12289, 64), (16384, 64),
                                (65535, 1024), (65536, 1), (65536, 64), (65537, 64), (65537, 1024))):
        ea = (0, K + 1)[j % 2]
        add(M, K, "evict", (M - ea, M - (K - 1), None, M - K, 0, 300),
            ("hiword_ties" if ea == 0 else "random", "all_equal", "random", "extremes", "random", "random"))
    # every realignment of k_pm_topk_sparse's bitmap: tile sizes just above 8,192 whose multiples cover the bit
    # offsets 1..31 on tiles the sparse pass sorts itself
    for j, M in enumerate(SH_SWEEP_M):
        add(M, 63, ("view", "evict")[j % 2], (700, 62, None, 2048, 0, 64),
            ("random", "extremes", "random", ("hiword_ties", "random")[j % 2], "random", "all_equal"), tag="-sh")
    # k above the select's capacity: the rocPRIM full sort by size
    for M in (4096, 8209):
        add(M, 1025, "view", (M, 1024, None, 1026, 0, 2049), P)
        add(M, 1025, "evict", (M, M - 1024, None, M - 1026, 0, 300), P)
    return tuple(cases)


def _sh_sweep_sizes():
    """Greedy: the fewest tile sizes from 8,193 up whose positions 1, 3, 5 of the tile list (the populated tiles
    behind the first) reach every bit offset (t M) & 31 in 1..31."""
    need, out = set(range(1, 32)), []
    for least in (3, 2, 1):                     # sizes that bring three new offsets first, then two, then one
        for M in range(REG_MAX + 1, REG_MAX + 33):
            got = {(t * M) & 31 for t in (1, 3, 5)} & need
            if len(got) >= least:
                out.append(M)
                need -= got
    assert not need
    return tuple(sorted(out))


SH_SWEEP_M = _sh_sweep_sizes()
SELECT_CASES = _select_cases()
SELECT_BY_ID = {c.id: c for c in SELECT_CASES}
ABSENT_ID = 9999


def tile_id(pos):
    return 100 + 7 * pos


def build_select_case(case):
    """(tiles dict id -> tile, the call's id list, proposals or None).  Proposals (eviction): K per listed tile, all
    valid, with distinct weights, so a wrong order of the target slots shows in the tile."""
    rng = np.random.default_rng(case.seed)
    tiles, order = {}, []
    for pos, s in enumerate(case.tiles):
        if s is None:
            order.append(ABSENT_ID)
            continue
        tiles[tile_id(pos)] = pattern_tile(rng, case.M, s.n_valid, s.pattern, case.k, case.mode)
        order.append(tile_id(pos))
    P = None
    if case.mode == "evict":
        n, K = len(order), case.k
        w = np.stack([(1.0 + rng.permutation(K)) / K for _ in range(n)])
        P = dict(L=rng.normal(size=(n, K, 3, 3)), th=rng.normal(size=(n, K, 3)), e=rng.normal(size=(n, K, NL, 3)), w=w,
                 v=np.ones((n, K), bool), c=rng.random((n, K, 3)) * 1.4 - 0.2,
                 s=rng.integers(0, 2, (n, K)).astype(np.int32))
    return tiles, order, P


def select_oracle(case, tiles, order, P, next_id=1000):
    """The oracle's answer: the view dict, or (per listed tile (n, ids), next id) with `tiles` updated in place."""
    if case.mode == "view":
        return opm.extract_atlas_map_view(tiles, order, case.k, case.M)
    out, nxt = [], next_id
    for i, tid in enumerate(order):
        t = tiles.setdefault(tid, opm.create_empty_tile(case.M))
        n, ids, dropped, nxt = opm.insert_masked(t, nxt, P["L"][i], P["th"][i], P["e"][i], P["w"][i], 5.5, P["v"][i],
                                                 scan_seq=SCAN_SEQ, colors_new=P["c"][i], sources_new=P["s"][i])
        out.append((n, ids))
    return out, nxt


@functools.lru_cache(maxsize=None)
def select_case_stats(case_id):
    """Per tile position of a case: the bitmap's bit offset, the keys besides the empty slots, the empty slots, the
    kernel that answers (sort_tiles' path refined per tile as k_pm_topk_sparse decides), and for hiword_ties the
    size of the k-th key's high-word group."""
    case = SELECT_BY_ID[case_id]
    tiles, order, _ = build_select_case(case)
    path = select_path(case.M, case.k)
    rows = []
    for pos, tid in enumerate(order):
        t = tiles.get(tid) or opm.create_empty_tile(case.M)
        keys, E = tile_keys(t, case.mode)
        other = int((keys != E).sum())
        empty = case.M - other
        kern = path
        if path == "tree+sparse":
            if other <= SP_MAX:
                kern = "sparse"
            elif case.mode == "evict" and empty >= min(case.k, case.M):
                kern = "dense_shortcut"
            else:
                kern = "tree"
        spec = case.tiles[pos]
        hw = None
        if spec is not None and spec.pattern == "hiword_ties" and spec.n_valid >= 2:
            o = np.argsort(keys, kind="stable")
            kth = keys[o[case.k - 1]]
            grp = keys[(keys >> np.uint64(32)) == (kth >> np.uint64(32))]
            inside = int((keys[o[:case.k]] >> np.uint64(32) == kth >> np.uint64(32)).sum())
            hw = dict(group=len(grp), distinct_low=len(np.unique(grp)), inside=inside)
        rows.append(dict(pos=pos, sh=(pos * case.M) & 31, other=other, empty=empty, kernel=kern, hiword=hw,
                         present=spec is not None))
    return dict(id=case.id, M=case.M, k=case.k, mode=case.mode, path=path, tiles=rows,
                G=-(-case.M // TOP_CHUNK), last_leaf=case.M - (-(-case.M // TOP_CHUNK) - 1) * TOP_CHUNK)


def select_table_guards():
    """Assertions on the inputs alone: the table reaches every branch the sweep is for.  Returns the report (what
    was reached) that the CPU test prints."""
    st = [select_case_stats(c.id) for c in SELECT_CASES]
    rep = dict(paths=sorted({s["path"] for s in st}), sh=set(), other=set(), dense_empty_minus_k=set(), leaves=set(),
               last_leaf=set(), kernels=set(), hiword=[], k_eq_M=set(), M=sorted({s["M"] for s in st}),
               k=sorted({s["k"] for s in st}))
    for s in st:
        assert 4 <= len(s["tiles"]) <= 6
        assert any(not r["present"] for r in s["tiles"][1:-1]), s["id"]        # an absent id in the middle
        assert any(r["present"] and r["other"] == 0 for r in s["tiles"]), s["id"]   # an empty tile
        if s["k"] == s["M"]:
            rep["k_eq_M"].add(s["M"])
        for r in s["tiles"]:
            rep["kernels"].add(r["kernel"])
            if r["kernel"] == "sparse" and r["other"] > 0:
                rep["sh"].add(r["sh"])
            if s["path"] in ("tree+sparse", "tree"):
                rep["other"].add(r["other"])
            if s["path"] == "tree+sparse" and s["mode"] == "evict" and r["other"] > SP_MAX:
                rep["dense_empty_minus_k"].add(r["empty"] - s["k"])
                assert (r["kernel"] == "dense_shortcut") == (r["empty"] >= s["k"])
            if r["kernel"] == "tree":
                rep["leaves"].add(s["G"])
                rep["last_leaf"].add(s["last_leaf"])
            if r["hiword"] is not None:
                h = r["hiword"]
                rep["hiword"].append((s["id"], r["pos"], h["group"], h["inside"]))
                # the k-th key shares its high word with another key whose low word differs
                assert h["group"] >= 2 and h["distinct_low"] >= 2, (s["id"], r)
                if s["M"] > s["k"] + 5 and r["kernel"] != "dense_shortcut" and r["empty"] < s["k"]:
                    assert 1 <= h["inside"] < h["group"], (s["id"], r)   # the group straddles rank k
    assert rep["paths"] == ["fullsort", "reg8", "tree", "tree+sparse"], rep["paths"]
    assert rep["sh"] >= set(range(1, 32)), sorted(set(range(1, 32)) - rep["sh"])
    assert {2047, 2048, 2049} <= rep["other"]
    assert {-1, 0, 1} <= rep["dense_empty_minus_k"]
    assert {3, 4, 16, 17} <= rep["leaves"] and {1, 17} <= rep["last_leaf"]
    assert {"sparse", "dense_shortcut", "tree", "reg8", "fullsort"} <= rep["kernels"]
    assert {1, 2, 1023, 1024} <= rep["k_eq_M"]
    assert {1, 2, 1023, 1024, 1025, 8191, 8192, 8193, 8209, 12289, 16384, 65535, 65536, 65537} <= set(rep["M"])
    assert any(r[0].startswith("view") for r in rep["hiword"]) and any(r[0].startswith("evict") for r in rep["hiword"])
    return rep


def _cpu(x):
    return x.detach().cpu().numpy()


def run_select_case(case, same_tile):
    """The case on the device against the oracle, exact (same_tile: test_gpu_primitive_map._same_tile)."""
    from gcslam import primitive_map as gpm
    tiles, order, P = build_select_case(case)
    am = gpm.AtlasMap(m_tile=case.M, max_tiles=8, n_lobes=NL, max_merge=0)
    try:
        for tid, t in tiles.items():
            am.write_tile(tid, t)
        if case.mode == "view":
            v = select_oracle(case, tiles, order, P)
            g = gpm.extract_atlas_map_view(am, order, case.k)
            for f in ("candidate_slots", "candidate_tile_ids", "valid_mask", "primitive_ids", "last_supported_scan_seq",
                      "weights"):
                a, b = _cpu(getattr(g, f)), v[f]
                assert np.array_equal(a, b), f"{case.id} {f}: first mismatch at {np.flatnonzero(a != b)[:8]}"
            np.testing.assert_allclose(_cpu(g.positions), v["positions"], rtol=1e-12, atol=1e-12, err_msg=case.id)
            return
        am.next_global_id = 1000
        res = gpm.primitive_map_insert_masked_tiles(am, order, P["L"], P["th"], P["e"], P["w"], 5.5, P["v"],
                                                    scan_seq=SCAN_SEQ, colors_new=P["c"], sources_new=P["s"])
        ref, nxt = select_oracle(case, tiles, order, P, 1000)
        for i, tid in enumerate(order):
            r, cert, eff = res[i]
            assert r.n_inserted == ref[i][0] == case.k, f"{case.id} tile {i}"
            assert np.array_equal(_cpu(r.new_ids), ref[i][1]), f"{case.id} tile {i} new_ids"
            same_tile(am.read_tile(tid), tiles[tid], what=f"{case.id} tile {i}")
            assert am.counts[tid] == int(tiles[tid]["valid_mask"].sum()), f"{case.id} tile {i} count"
        assert am.next_global_id == nxt
    finally:
        am.close()


def child_select_table():
    """Entry of the knob children (the knobs are read once per process): the whole select table against the oracle;
    the failing case's id goes to stderr and the exit status is non-zero."""
    from test_gpu_primitive_map import _same_tile
    for case in SELECT_CASES:
        try:
            run_select_case(case, _same_tile)
        except BaseException:
            sys.stderr.write(f"select case failed: {case.id}\n")
            raise


# --------------------------------------------------------------------------------------------------
# fuse cases (primitive_map_update: fuse_blocks' sort and k_pm_fuse_runs)
# --------------------------------------------------------------------------------------------------

M_FUSE = 1024
INACTIVE_ID = 777
MERGE_CAP = 512     # below M_FUSE: merge-reduce answers with its budget cap on both sides (not this sweep's subject)


@dataclass(frozen=True)
class FuseCase:
    id: str
    N: int
    B: int
    K: int
    n_active: int
    seed: int
    kind: str = "random"            # random | mono | layout | blocks
    layout: tuple = ()              # kind layout: run lengths in sorted-key order (one block); the rest is the tail
    tail: int = 0                   # kind layout: rows of the inactive tile (the nokey tail)
    refused: bool = False

    @property
    def nb(self):
        return -(-self.N // self.B)

    @property
    def rows(self):
        return self.nb * self.B * self.K


FUSE_ROW_CASES = (
    FuseCase("rows1023", 341, 341, 3, 4, 2001),
    FuseCase("rows1024", 128, 128, 8, 4, 2002),
    FuseCase("rows1025", 205, 205, 5, 4, 2003),
    FuseCase("rows16384", 2048, 256, 8, 3, 2004),
    FuseCase("rows16384-mono", 2048, 256, 8, 3, 2005, kind="mono"),
    FuseCase("rows16385", 565, 565, 29, 3, 2006),
    FuseCase("rows65536", 2048, 256, 32, 3, 2007),
    FuseCase("rows65536-mono", 2048, 256, 32, 3, 2008, kind="mono"),
    FuseCase("rows67584", 2048, 256, 33, 3, 2009),
    FuseCase("ragged", 300, 128, 8, 5, 2010),
    FuseCase("nb256", 256, 1, 4, 4, 2011),
)
FUSE_REFUSED = FuseCase("nb257", 257, 1, 4, 4, 2012, refused=True)


def _singles(n):
    return (1,) * n


FUSE_RUN_CASES = (
    # 545 rows in the seven lengths around 32 / 64 and 257, 217 single rows, then a run of 40 from position
    # 762 = 2 * 256 + 250 (it crosses a workgroup of k_pm_fuse_runs), singles, a run of 50 directly before the tail
    FuseCase("run-lengths", 256, 256, 8, 3, 2101, kind="layout",
             layout=(31, 32, 33, 63, 64, 65, 257) + _singles(217) + (40,) + _singles(300) + (50,), tail=896),
    # every row valid and in an active tile (no tail): the last run's 33 rows end on the array's last position
    FuseCase("run-end33", 128, 128, 8, 3, 2102, kind="layout", layout=_singles(400) + (70,) + _singles(521) + (33,)),
    # the same with 32 rows: the longest run that is not summed ahead, where pos + 32 == n
    FuseCase("run-end32", 128, 128, 8, 3, 2103, kind="layout", layout=_singles(400) + (70,) + _singles(522) + (32,)),
    # two association blocks, each with a long run on the same slots (the adds go block by block)
    FuseCase("run-two-blocks", 512, 256, 8, 3, 2104, kind="blocks"),
)
FUSE_CASES = FUSE_ROW_CASES + FUSE_RUN_CASES
FUSE_BY_ID = {c.id: c for c in FUSE_CASES + (FUSE_REFUSED,)}
Z_T = np.array([0.4, 0.2, -0.3, -0.03, 0.02, 0.9])
TS, SEQ, KINS, NEXT_ID = 7.0, 33, 64, 50_000


@functools.lru_cache(maxsize=None)
def build_fuse_case(case_id):
    """The inputs of one step 12b: dict(batch, assoc, active, tiles) -- `tiles` the map before the step (the first
    active tile populated).  Cached: callers copy what they change."""
    c = FUSE_BY_ID[case_id]
    rng = np.random.default_rng(c.seed)
    N, K, m = c.N, c.K, M_FUSE
    R, t = se3.so3_exp(Z_T[3:]), Z_T[:3]
    p_body = rng.uniform(-4, 4, size=(N, 3))
    A = rng.normal(size=(N, 3, 3)) * 0.2
    Lam = np.einsum("nij,nkj->nik", A, A) + np.eye(3)[None] * rng.uniform(1, 5, size=(N, 1, 1))
    exact = c.kind in ("mono", "layout", "blocks")       # the key array is laid out row by row: every row valid
    valid = np.ones(N, bool) if exact else rng.random(N) < 0.85
    batch = dict(Lambdas=Lam, thetas=np.einsum("nij,nj->ni", Lam, p_body), etas=rng.normal(size=(N, NL, 3)),
                 weights=rng.random(N), valid_mask=valid, colors=rng.random((N, 3)),
                 sources=rng.integers(0, 2, N).astype(np.int32))
    wtid = opm.tile_ids_from_xyz(p_body @ R.T + t[None], 2.0)
    uniq, cnts = np.unique(wtid, return_counts=True)
    active = [int(x) for x in uniq[np.argsort(-cnts, kind="stable")][:c.n_active]]
    assert len(active) == c.n_active and INACTIVE_ID not in active
    na, NK = len(active), N * K
    if c.kind == "random":
        tp = rng.integers(0, na + 1, NK)                  # na: the inactive tile
        slot = rng.integers(0, m, NK)
    elif c.kind == "mono":                                # keys ascend with the row: whole runs below a pair
        g = np.arange(NK, dtype=np.int64)
        flat = g * (na * m) // NK
        tp, slot = flat // m, flat % m
    elif c.kind == "layout":
        assert c.nb == 1 and sum(c.layout) + c.tail == NK and len(c.layout) <= na * m
        sk = np.repeat(np.arange(len(c.layout), dtype=np.int64), c.layout)   # sorted position -> (tile, slot) rank
        # spread the ranks over the active tiles' slots, order kept
        flat = np.sort(rng.permutation(na * m)[:len(c.layout)])[sk]
        tp_s = np.concatenate([flat // m, np.full(c.tail, na)])
        slot_s = np.concatenate([flat % m, rng.integers(0, m, c.tail)])
        perm = rng.permutation(NK)
        tp, slot = np.empty(NK, np.int64), np.empty(NK, np.int64)
        tp[perm], slot[perm] = tp_s, slot_s
    else:                                                 # blocks: runs of 40 / 70 / 33 rows per block on three slots
        tp, slot = rng.integers(0, na + 1, NK), rng.integers(0, m, NK)
        per = c.B * K
        for b in range(c.nb):
            rows = b * per + rng.permutation(per)
            o = 0
            for (tt, ss), ln in zip(((0, 5), (1, 900), (2, 17)), ((40, 70, 33), (70, 40, 65))[b % 2]):
                keep = (tp[b * per:(b + 1) * per] == tt) & (slot[b * per:(b + 1) * per] == ss)
                slot[b * per:(b + 1) * per][keep] = (ss + 1) % m          # no stray row on the crafted slots
                tp[rows[o:o + ln]], slot[rows[o:o + ln]] = tt, ss
                o += ln
    ctile = np.array(active + [INACTIVE_ID], dtype=np.int64)[tp].reshape(N, K)
    assoc = dict(responsibilities=rng.random((N, K)) / K, candidate_tile_ids=ctile,
                 candidate_slots=np.asarray(slot, np.int64).reshape(N, K), row_masses=rng.random(N) * 2.0 / N)
    t0 = rand_tile(rng, m=m, frac=0.5, seq_hi=30)
    t0["weights"][rng.random(m) < 0.05] = 1e-6            # below the cull threshold
    return dict(batch=batch, assoc=assoc, active=active, tiles={active[0]: t0})


def fuse_sorted_keys(case):
    """The key array fuse_blocks sorts, restated: ((tile position M + slot) nb + block) per padded row, kNoKey for
    rows that are padding, invalid or of no active tile; stable order (ties by row)."""
    d = build_fuse_case(case.id)
    N, K, B, nb = case.N, case.K, case.B, case.nb
    g = np.arange(case.rows)
    row, kk = g // K, g % K
    mi = np.minimum(row, N - 1)
    pos = {t: i for i, t in enumerate(d["active"])}
    tpos = np.array([pos.get(int(x), -1) for x in d["assoc"]["candidate_tile_ids"][mi, kk]])
    slot = d["assoc"]["candidate_slots"][mi, kk]
    ok = (row < N) & d["batch"]["valid_mask"][mi] & (tpos >= 0)
    assert len(d["active"]) * M_FUSE * nb < NOKEY
    key = np.where(ok, (tpos * M_FUSE + slot) * nb + row // B, NOKEY).astype(np.uint64)
    o = np.argsort(key, kind="stable")
    return key[o], o


def fuse_case_stats(case):
    """Of the sorted key array: padded rows, the sort fuse_blocks takes, runs (start, length) of one key, the tail,
    and k_ss_merge's last-step hits: (pair, other full run) with the whole run below the pair."""
    ks, order = fuse_sorted_keys(case)
    n = len(ks)
    starts = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
    lens = np.diff(np.r_[starts, n])
    real = ks[starts] != NOKEY
    tail = int((ks == NOKEY).sum())
    runs = [(int(s), int(ln)) for s, ln in zip(starts[real], lens[real])]
    sort = "lds1" if n <= SS_MAX else "lds4" if n <= SS_WIDE_MAX else "rocprim"
    hits = 0
    if sort != "rocprim":
        rank = np.empty(n, np.int64)
        rank[order] = np.arange(n)                                   # final position of input row g (run g // 1024)
        for r in range(n // SS_RUN):                                 # full runs only (padding is above every pair)
            top = rank[r * SS_RUN:(r + 1) * SS_RUN].max()            # the run's largest pair, by final position
            above = np.arange(n) > top                               # sorted positions above the whole run
            src = order[above]
            hits += int(((src // SS_RUN != r) & (ks[above] != NOKEY)).sum())
    # the same slot in two blocks, both long
    nb = case.nb
    long_keys = {int(ks[s]) for s, ln in runs if ln > FUSE_CHUNK}
    two = sum(1 for kx in long_keys if kx % nb + 1 < nb and kx + 1 in long_keys)
    return dict(id=case.id, rows=n, nrun=-(-n // SS_RUN), sort=sort, runs=runs, tail=tail, merge_last_step=hits,
                long=sorted({ln for _, ln in runs if ln > FUSE_CHUNK}), two_block_slots=two,
                max_run=max([ln for _, ln in runs], default=0))


def fuse_table_guards():
    """Assertions on the inputs alone; returns the report the CPU test prints."""
    rows_want = {"rows1023": 1023, "rows1024": 1024, "rows1025": 1025, "rows16384": 16384, "rows16384-mono": 16384,
                 "rows16385": 16385, "rows65536": 65536, "rows65536-mono": 65536, "rows67584": 67584}
    sort_want = {1023: "lds1", 1024: "lds1", 1025: "lds1", 16384: "lds1", 16385: "lds4", 65536: "lds4",
                 67584: "rocprim"}
    rep = {}
    for c in FUSE_CASES:
        s = fuse_case_stats(c)
        rep[c.id] = {k: s[k] for k in ("rows", "nrun", "sort", "tail", "merge_last_step", "long", "max_run",
                                       "two_block_slots")}
        assert s["rows"] == c.rows and 3 <= c.n_active <= 5
        if c.id in rows_want:
            assert s["rows"] == rows_want[c.id] and s["sort"] == sort_want[s["rows"]], s
    assert FUSE_BY_ID["ragged"].N % FUSE_BY_ID["ragged"].B != 0 and FUSE_BY_ID["nb256"].nb == MAX_FUSE_BLOCKS
    assert FUSE_REFUSED.nb == MAX_FUSE_BLOCKS + 1
    # whole foreign runs of valid pairs below a valid pair: the lo == 1023 step of k_ss_merge decides positions
    assert rep["rows16384-mono"]["merge_last_step"] >= 15 * SS_RUN
    assert rep["rows65536-mono"]["merge_last_step"] >= 63 * SS_RUN
    s = fuse_case_stats(FUSE_BY_ID["run-lengths"])
    lens = [ln for _, ln in s["runs"]]
    assert {31, 32, 33, 63, 64, 65, 257} <= set(lens)
    assert any(st % FUSE_THREADS == 250 and ln > FUSE_CHUNK and st // FUSE_THREADS != (st + ln - 1) // FUSE_THREADS
               for st, ln in s["runs"])                             # a long run across a workgroup
    st, ln = s["runs"][-1]
    assert ln > FUSE_CHUNK and s["tail"] > 0 and st + ln == s["rows"] - s["tail"]   # long run, then the tail
    for cid, last in (("run-end33", 33), ("run-end32", 32)):
        s = fuse_case_stats(FUSE_BY_ID[cid])
        st, ln = s["runs"][-1]
        assert s["tail"] == 0 and ln == last and st + ln == s["rows"]  # the run ends on the last position
        assert (st + FUSE_CHUNK < s["rows"]) == (last > FUSE_CHUNK)
    assert fuse_case_stats(FUSE_BY_ID["run-two-blocks"])["two_block_slots"] >= 3
    return rep


@functools.lru_cache(maxsize=None)
def fuse_oracle(case_id):
    """oracle step 12b of a case: (tiles after, next id, counters).  Computed once; callers leave it unchanged."""
    c = FUSE_BY_ID[case_id]
    d = build_fuse_case(case_id)
    tiles = {tid: opm.copy_tile(t) for tid, t in d["tiles"].items()}
    R, t = se3.so3_exp(Z_T[3:]), Z_T[:3]
    nxt, st = opm.map_update_step(tiles, NEXT_ID, d["batch"], d["assoc"], R, t, d["active"], M_FUSE, TS, SEQ,
                                  k_insert_tile=KINS, h_tile=2.0, block_size=c.B, merge_max_tile_size=MERGE_CAP)
    return tiles, nxt, st


def fuse_device(case, am=None):
    """The case's step 12b on a fresh (or the given) AtlasMap: (map, counters); the caller closes the map (a fresh
    one is closed here if the call raises)."""
    from types import SimpleNamespace
    from gcslam import primitive_map as gpm
    d = build_fuse_case(case.id)
    own = am is None
    if own:
        am = gpm.AtlasMap(m_tile=M_FUSE, max_tiles=8, n_lobes=NL, max_merge=0)
    for tid, tt in d["tiles"].items():
        am.write_tile(tid, tt)
    am.next_global_id = NEXT_ID
    cfg = gpm.PrimitiveMapUpdateConfig(k_insert_tile=KINS, block_size=case.B, primitive_merge_max_tile_size=MERGE_CAP)
    try:
        st = gpm.primitive_map_update(am, SimpleNamespace(**d["batch"]), SimpleNamespace(**d["assoc"]), Z_T,
                                      d["active"], TS, SEQ, cfg)
    except BaseException:
        if own:
            am.close()
        raise
    return am, st


def child_fuse_dump(path):
    """Entry of the sort-path children (GCSLAM_FUSE_SMALLSORT is read once per process): every fuse case on the
    device, every active tile's arrays into one .npz."""
    out = {}
    for c in FUSE_CASES:
        am, st = fuse_device(c)
        try:
            for tid in build_fuse_case(c.id)["active"]:
                for f, a in am.read_tile(tid).items():
                    out[f"{c.id}/{tid}/{f}"] = a
        finally:
            am.close()
    np.savez(path, **out)
