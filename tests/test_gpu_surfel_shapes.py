"""Surfel extraction (gcs_surfels.hip) at every occupancy form, grid size, sort path and capacity edge,
each case against the numpy oracle (oracle/surfels.py) at the bars of tests/test_gpu_surfels.py: buckets,
clipped counts and selected cell ids bit-exact; positions, weights and timestamps at rtol 1e-9; covariances
and the information form at 1e-7 of the matrix norm; normals at 1e-7 absolute and kappas at rtol 1e-6 on
every selected cell (the guards assert that every selected cell's smallest eigenvalue is separated).

The case table and the guards -- assertions on the oracle's output alone that show a case reaches its branch
-- live in tests/surfel_util.py; tests/test_surfels.py runs the same guards without a GPU.  A case with an
A/B knob (GCSLAM_SF_FOLD_CELLS, GCSLAM_SF_LDS_SORT) runs both settings: each against the oracle, and
bitwise equal to each other.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import surfel_util as SU
from oracle import surfels as OS

pytestmark = pytest.mark.gpu


def _check(case, got, ref, pts, w, ocfg):
    if case.mode == "flat":
        SU.compare_flat(got, ref)
        return
    checked = SU._compare(got, ref, ocfg, pts, w)
    assert checked == ref["n_valid"]            # normals and kappas on every selected row
    SU.compare_info(got, ref, ocfg)


@pytest.mark.parametrize("case", SU.CASES, ids=[c.id for c in SU.CASES])
def test_case_matches_oracle(case, monkeypatch):
    pts, t, w = case.scene()
    ocfg = case.ocfg()
    if case.knob:
        monkeypatch.setenv(case.knob, "1")
    got = SU.device_run(pts, t, w, ocfg, case.max_points)
    SU.check_center(got, pts, w, ocfg)
    ref = OS.extract_surfels_mahex3d(pts, t, w, ocfg, center=got["center"], only_occupied=True)
    SU.guards(case, ref)
    _check(case, got, ref, pts, w, ocfg)
    if case.mode == "empty":                    # padding rows as the reference's
        assert got["n_valid"] == 0 and np.all(got["cell_ids"] == -1) and not got["valid_mask"].any()
        assert np.all(got["covariances"] == np.eye(3)[None]) and not got["positions"].any()
    if case.knob:
        monkeypatch.setenv(case.knob, "0")
        alt = SU.device_run(pts, t, w, ocfg, case.max_points)
        _check(case, alt, ref, pts, w, ocfg)
        SU.assert_bitwise_equal(got, alt, case.knob)


@pytest.mark.parametrize("seq", SU.SEQUENCES, ids=[s.id for s in SU.SEQUENCES])
def test_one_context_many_calls(seq):
    """Calls of different sizes and sort paths on one context: every output and intermediate bitwise equal to
    the same call on a fresh context (stale run bounds, sorted values, moment and fit rows stay unread)."""
    from gcslam.surfels import SurfelExtractor
    ocfg = OS.SurfelExtractionConfig(**seq.cfg)
    cases = SU.sequence_cases(seq)
    scenes = [c.scene() for c in cases]
    fresh = [SU.device_run(p, t, w, ocfg, seq.max_points) for p, t, w in scenes]
    for c, (p, t, w), r in zip(cases, scenes, fresh):
        ref = OS.extract_surfels_mahex3d(p, t, w, ocfg, center=r["center"], only_occupied=True)
        SU.guards(c, ref)
        _check(c, r, ref, p, w, ocfg)
    ex = SurfelExtractor(SU._cfg(ocfg), max_points=seq.max_points)
    try:
        for i, (p, t, w) in enumerate(scenes):
            SU.assert_bitwise_equal(SU.snapshot(ex.extract(*SU.writable(p, t, w), want_intermediates=True)), fresh[i], f"call {i}")
    finally:
        ex.close()
    for (p, t, w), r in zip(scenes, fresh):
        if len(p) == 0:                         # all padding, counts 0
            assert r["n_valid"] == 0 and int(r["count"].sum()) == 0 and np.all(r["bucket"] == -1)
            assert np.all(r["cell_ids"] == -1) and np.all(r["covariances"] == np.eye(3)[None])
        else:
            assert r["n_valid"] > 0
