"""CPU checks of map publishing and the splat export: tests/map_export_ref.py (the numpy restatement the GPU
tests compare with) is pinned with answers worked by hand, and the library exports gcs_pmap_export with
the ABI version and the struct layout the binding expects."""

import ctypes as C
import os
import re
import struct

import numpy as np

import map_export_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _three_row_tile():
    """Slots 0..3 of a 4-slot tile; slot 1 is invalid.  Lambda = diag, so the answers are quotients."""
    t = R.create_empty_tile(4)
    t["valid_mask"][:] = [True, False, True, True]
    t["weights"][:] = [0.5, 9.0, 2.0, 0.5]          # slots 0 and 3 tie at 0.5
    t["Lambdas"][:] = np.eye(3)[None] * np.array([1.0, 1.0, 2.0, 4.0])[:, None, None]
    t["thetas"][:] = [[1.0, 2.0, 3.0], [7.0, 7.0, 7.0], [2.0, 4.0, 6.0], [4.0, 8.0, 12.0]]
    t["etas"][:] = 0.0
    t["etas"][0, :, 2] = [1.0, 1.0, 1.0]            # sum (0, 0, 3): kappa 3, direction +z
    t["etas"][2, 0] = [3.0, 4.0, 0.0]               # kappa 5, direction (0.6, 0.8, 0)
    t["etas"][3, 1] = [0.0, -2.0, 0.0]              # kappa 2, direction -y
    t["primitive_ids"][:] = [40, 41, 42, 43]
    t["rgb"][:] = [[0.1, 0.2, 0.3], [0.9, 0.9, 0.9], [0.4, 0.5, 0.6], [0.7, 0.8, 0.9]]
    return t


def test_view_is_the_valid_slots_in_slot_order():
    v = R.extract_primitive_map_view(_three_row_tile(), 7, eps_lift=0.0, eps_mass=0.0)
    assert v["slot_indices"].tolist() == [0, 2, 3] and v["slot_indices"].dtype == np.int32
    assert v["tile_id"] == 7 and v["m_tile"] == 4
    assert np.array_equal(v["positions"], [[1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [1.0, 2.0, 3.0]])
    assert np.array_equal(v["covariances"], np.eye(3)[None] * np.array([1.0, 0.5, 0.25])[:, None, None])
    assert v["kappas"].tolist() == [3.0, 5.0, 2.0]
    assert np.array_equal(v["directions"], [[0.0, 0.0, 1.0], [0.6, 0.8, 0.0], [0.0, -1.0, 0.0]])
    assert v["weights"].tolist() == [0.5, 2.0, 0.5] and v["primitive_ids"].tolist() == [40, 42, 43]
    assert np.array_equal(v["colors"], [[0.1, 0.2, 0.3], [0.4, 0.5, 0.6], [0.7, 0.8, 0.9]])   # the tile's rgb
    # max_primitives == count: no downselection, still slot order
    assert R.extract_primitive_map_view(_three_row_tile(), 7, 3)["slot_indices"].tolist() == [0, 2, 3]


def test_view_downselects_by_weight_with_ties_to_the_lower_slot():
    v = R.extract_primitive_map_view(_three_row_tile(), 7, max_primitives=2)
    assert v["slot_indices"].tolist() == [2, 0]      # weight 2.0, then the 0.5 tie across the cut: slot 0, not 3
    assert v["weights"].tolist() == [2.0, 0.5] and v["primitive_ids"].tolist() == [42, 40]
    assert R.extract_primitive_map_view(_three_row_tile(), 7, max_primitives=1)["slot_indices"].tolist() == [2]
    t = _three_row_tile()
    t["weights"][:] = [-0.0, 9.0, 0.0, -0.0]         # -0.0 == 0.0: all tie, slot order decides
    assert R.extract_primitive_map_view(t, 7, max_primitives=2)["slot_indices"].tolist() == [0, 2]


def test_empty_and_absent_tiles():
    t = R.create_empty_tile(4)
    v = R.extract_primitive_map_view(t, 3)
    assert v["positions"].shape == (0, 3) and v["covariances"].shape == (0, 3, 3) and v["etas"].shape == (0, 3, 3)
    assert R.renderable_batch_from_view(v)["Lambda_world"] is None
    p = R.publish({3: t}, [3, 99])
    assert p["n"] == 0 and p["data"] == b"" and p["tile_rows"].tolist() == [0, 0] and p["Lambda_world"] is None
    assert R.export_splats({3: t}) is None


def test_lexsort_order_over_all_64_bits():
    big = (1 << 32) + 5
    rec = np.array([3, -2, big, 3, big, -2, 3], np.int64)
    ids = np.array([9, 1, 7, -4, 7, big, 9], np.int64)
    # newest first: recency 2^32+5 (ids 7, 7: positions 2 then 4), then 3 (ids -4, 9, 9: 3, 0, 6), then -2
    # (ids 1, 2^32+5: 1, 5)
    assert R.lexsort_order(ids, rec).tolist() == [2, 4, 3, 0, 6, 1, 5]


def test_pointcloud2_bytes_literal():
    up = 1.0 + 2.0 ** -24 + 2.0 ** -30               # above the midpoint of 1 and 1 + 2^-23: rounds up
    w = np.array([-1.0, 0.5, 1e6, 2e6, up])
    pos = np.array([[1.0, -2.0, 0.25], [0.0, 0.0, 0.0], [1.0 + 2.0 ** -24, 3.0, 4.0],   # a tie: to even, 1.0
                    [1e39, -1e39, 8.0], [up, 1.0, 1.0]])
    inf = 0x7f800000
    words = [0x3f800000, 0xc0000000, 0x3e800000, 0x00000000,         # intensity clip(-1) = 0
             0x00000000, 0x00000000, 0x00000000, 0x3f000000,         # 0.5
             0x3f800000, 0x40400000, 0x40800000, 0x49742400,         # 1e6
             inf, 0xff800000, 0x41000000, 0x49742400,                # +-inf out of range; clip(2e6) = 1e6
             0x3f800001, 0x3f800000, 0x3f800000, 0x3f800001]
    assert R.pointcloud2_bytes(pos, w) == struct.pack("<20I", *words)
    assert R.pointcloud2_bytes(np.zeros((0, 3)), np.zeros(0)) == b""
    nan = R.pointcloud2_bytes(np.zeros((1, 3)), np.array([np.nan]))
    assert np.isnan(np.frombuffer(nan, "<f4")[3])                    # np.clip propagates NaN


def test_publish_concatenates_skips_and_orders():
    a, b = _three_row_tile(), _three_row_tile()
    b["primitive_ids"][:] += 100
    a["last_supported_scan_seq"][:] = [5, 0, 1, 5]
    b["last_supported_scan_seq"][:] = [1, 0, 5, 9]
    p = R.publish({1: a, 2: b}, [2, 77, 1])
    assert p["tile_rows"].tolist() == [3, 0, 3] and p["n"] == 6
    # recency 9 (id 143), 5 (ids 40, 43, 142), 1 (ids 42, 140)
    assert p["primitive_ids"].tolist() == [143, 40, 43, 142, 42, 140]
    assert p["tile_ids"].tolist() == [2, 1, 1, 2, 1, 2] and p["slots"].tolist() == [3, 0, 3, 2, 2, 0]
    assert len(p["data"]) == 96 and p["cloud"]["row_step"] == 96 and p["cloud"]["width"] == 6
    c = R.publish({1: a, 2: b}, [2, 77, 1], order=False)
    assert c["primitive_ids"].tolist() == [140, 142, 143, 40, 42, 43]
    e = R.export_splats({2: b, 1: a})
    assert tuple(e) == R.SPLAT_KEYS and e["n"] == 6 and e["primitive_ids"].tolist() == [40, 42, 43, 140, 142, 143]
    assert np.array_equal(e["rgb"], e["colors"])


def test_library_exports_the_entry_point(lib):
    from gcslam import _lib as L
    hdr = open(os.path.join(ROOT, "include", "gcslam_hip.h")).read()
    assert re.search(r"^int gcs_pmap_export\(", hdr, re.M)
    assert "gcs_pmap_export" in L.SYMBOLS and hasattr(lib, "gcs_pmap_export")
    assert lib.gcs_abi_version() == 4 and L.ABI_VERSION == 4
    block = re.search(r"typedef struct \{([^}]*)\} gcs_pmap_export_out;", hdr).group(1)
    members = re.findall(r"^\s*(?:double|int64_t|int32_t|void)\*\s+(\w+);", block, re.M)
    assert members == [f[0] for f in L.GcsPmapExportOut._fields_]
    assert C.sizeof(L.GcsPmapExportOut) == C.sizeof(C.c_void_p) * len(members) == 152
    n = C.c_int32(-1)
    assert lib.gcs_pmap_export(None, None, None, 0, 0, 0, 1e-9, 1e-12, 0, None, C.byref(n), None) == -1
