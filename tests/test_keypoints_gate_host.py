"""gcs_match_descriptors_gated_host and gcs_match_pairs_host (no device) against tests/keypoints_gate_ref.py's numpy
restatement of D8 and D9: every output as bytes on every fixture, the pairs without a gate against the
match_descriptors_host that was shipped before them, the refusals and that the next valid call still works, n = 0 on
either side, and the defaults.  The fixtures' own conditions (the hand-written candidate matrices of `edges`, the
end-to-end figures) are asserted where keypoints_gate_ref builds them."""

import ctypes as C
import os
import re

import numpy as np
import pytest

import keypoints_desc_ref as DR
import keypoints_gate_ref as G
from gcslam import _lib as L
from gcslam import descriptors as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gcs_match_gate_defaults", "gcs_match_filter_defaults", "gcs_match_descriptors_gated", "gcs_match_pairs",
               "gcs_match_descriptors_gated_host", "gcs_match_pairs_host")


def gate_args(gate):
    """keypoints_gate_ref's gate as the keyword arguments of gcslam.descriptors' gated entries."""
    if gate is None:
        return {}
    def kp(s):
        rows = (gate[s + "_u"], gate[s + "_v"])
        return rows if gate[s + "_level"] is None else rows + (None, gate[s + "_level"])

    kw = dict(kp_q=kp("q"), kp_t=kp("t"), gate=D.GateConfig(gate["radius"], gate["max_level_diff"]))
    if gate["q_pu"] is not None:
        kw["predicted"] = (gate["q_pu"], gate["q_pv"])
    return kw


def same(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.int32 and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, k, g, w)


def test_symbols_declared_listed_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "gcslam_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int64_t|const char\*)\s+(gcs_\w+)\s*\(", hdr, re.M))
    for name in NEW_SYMBOLS:
        assert name in declared and name in L.SYMBOLS and hasattr(lib, name), name
    for k in ("GateConfig", "match_pairs", "match_pairs_host", "nearest_gated_host"):
        assert hasattr(D, k), k
    assert hasattr(D.DescriptorMatcher, "queue_gated") and hasattr(D.DescriptorMatcher, "queue_pairs")
    assert "D8." in hdr and "D9." in hdr


def test_defaults(lib):
    g = L.GcsMatchGate(1, 2, 3, 4, 5, 6, 7, 8, -1.0, -1)
    assert lib.gcs_match_gate_defaults(C.byref(g)) == 0 and lib.gcs_match_gate_defaults(None) == -1
    assert (g.radius, g.max_level_diff) == (16.0, 1)
    assert [getattr(g, n) for n in ("q_u", "q_v", "q_level", "t_u", "t_v", "t_level", "q_pu", "q_pv")] == [None] * 8
    f = L.GcsMatchFilter()
    assert lib.gcs_match_filter_defaults(C.byref(f)) == 0 and lib.gcs_match_filter_defaults(None) == -1
    assert (f.max_distance, f.ratio_num, f.ratio_den, f.cross_check) == (64, 4, 5, 1)
    assert D.gate_defaults() == D.GateConfig() == D.GateConfig(16.0, 1)
    assert D.filter_defaults() == (64, (4, 5), True)


@pytest.mark.parametrize("name", G.GATED_NAMES)
def test_host_gated_search_equals_the_restatement(name):
    q, t, q_bin, t_bin, gate = G.gated_fixture(name)
    same(D.nearest_gated_host(q, t, q_bin=q_bin, t_bin=t_bin, **gate_args(gate)), G.gated_expected(name), name)


def test_the_gate_changes_nothing_where_every_row_is_inside():
    """A window that holds every row: D8's idx, dist, dist2 are D7's."""
    q, t, q_bin, t_bin = DR.match_fixture("invalid_rows")
    zq, zt = np.zeros(len(q), np.float32), np.zeros(len(t), np.float32)
    got = D.nearest_gated_host(q, t, (zq, zq), (zt, zt), gate=D.GateConfig(0.0, 0), q_bin=q_bin, t_bin=t_bin)
    same(got[:3], DR.match_expected("invalid_rows"), "invalid_rows")
    assert (got[3] == np.where(q_bin >= 0, (t_bin >= 0).sum(), 0)).all()


@pytest.mark.parametrize("name", G.PAIRS_NAMES)
def test_host_pairs_equal_the_restatement(name):
    q, t, q_bin, t_bin, gate = G.pairs_fixture(name)
    for gated, kw in G.pairs_cases(name):
        got = D.pairs_host(q, t, q_bin=q_bin, t_bin=t_bin, **kw, **(gate_args(gate) if gated else {}))
        same(got, G.pairs_expected(name, gated, kw), (name, gated, kw))


@pytest.mark.parametrize("name", ["predicted", "ties", "gate_257x513", "edges", "edges_predicted"])
def test_host_pairs_on_the_gated_fixtures(name):
    q, t, q_bin, t_bin, gate = G.gated_fixture(name)
    G.gated_expected(name)
    for kw in G.FILTERS:
        same(D.pairs_host(q, t, q_bin=q_bin, t_bin=t_bin, **kw, **gate_args(gate)), G.pairs(q, t, gate, q_bin, t_bin, **kw),
             (name, kw))


def test_pairs_without_a_gate_are_match_descriptors_hosts():
    """D9 is the behaviour already shipped: the four filter settings of
    test_match_descriptors_applies_the_filters_on_the_device."""
    a, b = DR.expected("ramp_96x64_l3_k48_c16"), DR.expected("blocks_61x97_l3_k200_c16")
    da, db = (D.Descriptors(r["desc"], r["angle"], r["angle_bin"]) for r in (a, b))
    for kw in (dict(), dict(cross_check=False), dict(ratio=(9, 10)), dict(max_distance=40, ratio=None)):
        want = D.match_descriptors_host(da, db, **kw)
        got = D.match_pairs_host(da, db, gate=None, **kw)
        assert len(want[0]) > 0
        same(got, want, kw)
    for name in ("self", "invalid_rows", "duplicates"):   # bare arrays and bins
        q, t, q_bin, t_bin = DR.match_fixture(name)
        sides = (D.Descriptors(q, None, q_bin), D.Descriptors(t, None, t_bin)) if q_bin is not None else (q, t)
        same(D.match_pairs_host(*sides), D.match_descriptors_host(*sides), name)


def _call(n_q=3, n_t=5):
    q, t = DR._rows(n_q, 93), DR._rows(n_t, 94)
    t[:n_q] = q   # every query row has its equal
    pos = np.zeros((6, 8), np.float32)
    out = np.zeros((4, n_q), np.int32)
    count = np.zeros(1, np.int32)
    i = L.GcsMatchInputs(n_q, n_t, q.ctypes.data, t.ctypes.data, None, None)
    g = L.GcsMatchGate(pos[0].ctypes.data, pos[1].ctypes.data, None, pos[2].ctypes.data, pos[3].ctypes.data, None, None, None,
                       8.0, 1)
    f = L.GcsMatchFilter(64, 4, 5, 1)
    o = L.GcsMatchGatedOutputs(*(out[k].ctypes.data for k in range(4)))
    p = L.GcsMatchPairOutputs(*(out[k].ctypes.data for k in range(3)), count.ctypes.data)
    return i, g, f, o, p, (q, t, pos, out, count)


BAD_GATE = [("radius", float("nan")), ("radius", -1.0), ("radius", float("inf")), ("max_level_diff", -1), ("q_u", None),
            ("q_v", None), ("t_u", None), ("t_v", None), ("q_pu", "set"), ("q_pv", "set"), ("n_query", 9), ("n_train", 9),
            ("n_query", -1), ("q", None), ("t", None)]
BAD_FILTER = [("ratio_num", 0), ("ratio_num", (1 << 20) + 1), ("ratio_den", -1), ("ratio_den", (1 << 20) + 1)]


@pytest.mark.parametrize("field,value", BAD_GATE + BAD_FILTER + [("idx", None), ("count", None), ("pair_b", None)])
def test_bad_gated_inputs_are_refused_and_the_next_call_works(lib, field, value):
    c = L.GcsMatchConfig(8, 8, 0)
    i, g, f, o, p, keep = _call()
    if value == "set":
        value = keep[2][4].ctypes.data
    target = next(s for s in (i, g, f, o, p) if hasattr(s, field))
    good = getattr(target, field)
    setattr(target, field, value)
    if target is not f and target is not p:
        assert lib.gcs_match_descriptors_gated_host(C.byref(c), C.byref(i), C.byref(g), C.byref(o)) == -1
    if target is not o:
        assert lib.gcs_match_pairs_host(C.byref(c), C.byref(i), C.byref(g), C.byref(f), C.byref(p)) == -1
    setattr(target, field, good)
    assert lib.gcs_match_descriptors_gated_host(C.byref(c), C.byref(i), C.byref(g), C.byref(o)) == 0
    assert lib.gcs_match_pairs_host(C.byref(c), C.byref(i), C.byref(g), C.byref(f), C.byref(p)) == 0
    assert keep[4][0] == 3 and keep[3][0].tolist() == [0, 1, 2]   # every row pairs with its equal


def test_null_structs_are_refused(lib):
    c = L.GcsMatchConfig(8, 8, 0)
    i, g, f, o, p, keep = _call()
    assert lib.gcs_match_descriptors_gated_host(C.byref(c), C.byref(i), None, C.byref(o)) == -1   # a gate is needed here
    assert lib.gcs_match_descriptors_gated_host(C.byref(c), None, C.byref(g), C.byref(o)) == -1
    assert lib.gcs_match_descriptors_gated_host(None, C.byref(i), C.byref(g), C.byref(o)) == -1
    assert lib.gcs_match_descriptors_gated_host(C.byref(c), C.byref(i), C.byref(g), None) == -1
    assert lib.gcs_match_pairs_host(C.byref(c), C.byref(i), C.byref(g), None, C.byref(p)) == -1
    assert lib.gcs_match_pairs_host(C.byref(c), C.byref(i), C.byref(g), C.byref(f), None) == -1
    assert lib.gcs_match_pairs_host(C.byref(c), C.byref(i), None, C.byref(f), C.byref(p)) == 0      # no gate
    assert lib.gcs_match_descriptors_gated(None, C.byref(i), C.byref(g), C.byref(o)) == -1
    assert lib.gcs_match_pairs(None, C.byref(i), C.byref(g), C.byref(f), C.byref(p)) == -1
    o.n_cand = None   # n_cand may be null
    assert lib.gcs_match_descriptors_gated_host(C.byref(c), C.byref(i), C.byref(g), C.byref(o)) == 0


def test_n_0_on_either_side(lib):
    e, q = np.zeros((0, 32), np.uint8), DR._rows(3, 91)
    z0, z3 = np.zeros(0, np.float32), np.zeros(3, np.float32)
    for got in (D.nearest_gated_host(e, q, (z0, z0), (z3, z3)), D.pairs_host(e, q, (z0, z0), (z3, z3))[:3]):
        assert all(x.shape == (0,) for x in got)
    assert D.pairs_host(e, q)[3].tolist() == [0] and D.pairs_host(e, q, (z0, z0), (z3, z3))[3].tolist() == [0]
    idx, dist, dist2, n_cand = D.nearest_gated_host(q, e, (z3, z3), (z0, z0))
    assert idx.tolist() == [-1] * 3 and dist.tolist() == [257] * 3 and dist2.tolist() == [257] * 3 and n_cand.tolist() == [0] * 3
    a, b, d, count = D.pairs_host(q, e, (z3, z3), (z0, z0))
    assert a.tolist() == [-1] * 3 and b.tolist() == [-1] * 3 and d.tolist() == [257] * 3 and count.tolist() == [0]
    c = L.GcsMatchConfig(8, 8, 0)   # n = 0 with null arrays throughout: only count is touched
    i = L.GcsMatchInputs(0, 0, None, None, None, None)
    g, f = L.GcsMatchGate(radius=1.0), L.GcsMatchFilter(64, 4, 5, 1)
    count = np.full(1, 9, np.int32)
    assert lib.gcs_match_descriptors_gated_host(C.byref(c), C.byref(i), C.byref(g), C.byref(L.GcsMatchGatedOutputs())) == 0
    assert lib.gcs_match_pairs_host(C.byref(c), C.byref(i), C.byref(g), C.byref(f),
                                    C.byref(L.GcsMatchPairOutputs(None, None, None, count.ctypes.data))) == 0
    assert count.tolist() == [0]


def test_python_entries_refuse_bad_arguments():
    q = DR._rows(3, 92)
    z = np.zeros(3, np.float32)
    with pytest.raises(ValueError):
        D.match_pairs_host(q, q, gate=D.GateConfig())                 # a gate without positions
    with pytest.raises(ValueError):
        D.match_pairs_host(q, q, kp_a=(z, z), gate=D.GateConfig())    # or with one side's only
    with pytest.raises(ValueError):
        D.match_pairs_host(q, q, (z, z), (z[:2], z[:2]))
    with pytest.raises(ValueError):
        D.match_pairs_host(q, q, (z, z), (z, z), gate=D.GateConfig(radius=-1.0))
    with pytest.raises(ValueError):
        D.match_pairs_host(q, q, (z, z), (z, z), predicted=(z[:2], z[:2]))
    with pytest.raises(ValueError):
        D.match_pairs_host(q, q, ratio=(0, 5))
    with pytest.raises(ValueError):
        D.nearest_gated_host(q, q, (z, z), (z, z), gate=D.GateConfig(max_level_diff=-1))
    a, b, d = D.match_pairs_host(q, q, (z, z), (z, z))
    assert a.tolist() == b.tolist() == [0, 1, 2] and d.tolist() == [0, 0, 0]


def test_the_restated_end_to_end_pair_meets_its_figures():
    """keypoints_gate_ref asserts them where it builds the pairs; the host twin returns the same pairs."""
    for build, want in ((G.vga_pyramid_gated, G.VGA_GATED_PYRAMID), (G.vga_grid_gated, G.VGA_GATED_GRID)):
        a, b, gate, ref = build()
        assert int(ref[3][0]) == want[0]
        got = D.pairs_host(a["desc"], b["desc"], q_bin=a["angle_bin"], t_bin=b["angle_bin"], **gate_args(gate))
        same(got, ref, want)
    assert G.VGA_GATED_PYRAMID[0] >= DR.VGA_PYRAMID_PAIRS
