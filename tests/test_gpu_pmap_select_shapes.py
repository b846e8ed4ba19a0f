"""The primitive map's per-tile top-k (sort_tiles of gcs_pmap.hip: k_pm_select_reg, k_pm_topk, k_pm_topk_sparse,
the rocPRIM full sort) at every path, tile size and k of tests/pmap_shape_util.py's select table, through
extract_atlas_map_view and primitive_map_insert_masked_tiles, each case against the numpy oracle
(oracle/primitive_map.py): slots, ids, masks, integer fields and weights equal, view positions at
rtol = atol = 1e-12, and after an insert every field of every tile bitwise.

The guards that show a case reaches its branch run without a GPU in tests/test_pmap_shapes.py.  The A/B knobs
(read once per process) each get one child process that runs the whole table the same way."""
import os
import subprocess
import sys

import pytest

torch = pytest.importorskip("torch")

import pmap_shape_util as U
from test_gpu_primitive_map import _same_tile

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", U.SELECT_CASES, ids=[c.id for c in U.SELECT_CASES])
def test_select_case_matches_oracle(case):
    U.run_select_case(case, _same_tile)


@pytest.mark.parametrize("env", [{"GCSLAM_PM_SELECT": "radix"}, {"GCSLAM_PM_FULLSORT": "1"},
                                 {"GCSLAM_PM_TOPK_SPARSE": "0"}], ids=["select_radix", "fullsort", "topk_tree_only"])
def test_select_table_knob_paths(env):
    """The one-workgroup radix select, the rocPRIM full sort and the tree for every tile on the whole table."""
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    code = ("import sys; sys.path[:0] = [%r, %r, %r]; import pmap_shape_util as U; U.child_select_table()"
            % (here, root, os.path.join(root, "gc-slam_amd")))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
