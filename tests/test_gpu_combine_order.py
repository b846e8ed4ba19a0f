"""gcs_scan_combine submits the scan's pushforward behind the combine's all-reduce and stage-out kernel
(GCS_DEBUG_PUSH_DEFER, default on); the two-call API (gcs_scan, then gcs_combine_allreduce) submits it
from the scan's tail.  Only the submission order differs, so over three scans at one small shape the
posterior, the scan outputs, the combined belief, the IW states and -- after a synchronize -- the map
agree bit for bit: with a world-1 RCCL communicator and with comm = NULL, with the context's own map
and with a single rank following itself (GCS_MAP_FOLLOW: the scan submits no pushforward, gcs_map_follow
replays the record the combine carried), and with the deferral switched off."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from gpu_util import device_scan
from gcslam.synthetic import scan_kwargs

pytestmark = pytest.mark.gpu

ORIGIN = (0.0, 0.0, 0.5)
B, CAP, N_SCANS = 5000, 4096, 3


@pytest.fixture(scope="module")
def scans():
    from gcslam import synthetic
    out = []
    for k in range(N_SCANS):
        sc = synthetic.make_scan(CAP, 60 + k)
        out.append((sc, device_scan(sc)))
    return out


def _run(scans, fused, comm, map_mode, defer=1):
    from gcslam import _lib as L
    from gcslam.context import HypothesisContext
    ctx = HypothesisContext(n_bins=B, n_points_cap=CAP, max_raw_points=CAP, mode="scale", lidar_origin=ORIGIN)
    try:
        ctx.set_debug(L.DEBUG_PUSH_DEFER, defer)
        ctx.set_map_mode(map_mode)
        res = []
        for k, (sc, (rec, t, w)) in enumerate(scans):
            prep = ctx.prepare_scan(rec, 16, t, w, CAP, **scan_kwargs(sc))
            out, comb = L.GcsScanOutputs(), L.GcsBelief()
            cert = np.zeros(4)
            if fused:
                ms = C.c_double()
                rc = ctx.lib.gcs_scan_combine(ctx.h, prep[1], C.byref(out), comm, 1.0, 1.0, k, C.addressof(comb),
                                              cert.ctypes.data, C.addressof(ms))
                ctx._chk(rc, "gcs_scan_combine")
            else:
                ctx.scan_prepared(prep, out)
                rc = ctx.lib.gcs_combine_allreduce(ctx.h, comm, 1.0, 1.0, k, C.addressof(comb), cert.ctypes.data)
                ctx._chk(rc, "gcs_combine_allreduce")
            if map_mode == "follow":
                ctx.map_follow(prep)
            ctx.synchronize()
            m, d = ctx.get_map()
            arrs = [np.array(getattr(out, f)[:]) for f in ("z_t", "cert", "L_evidence", "h_evidence", "R_mf", "t_wls",
                                                           "iw_process_dPsi", "iw_process_dnu")]
            arrs += [np.asarray(x) for x in L.struct_to_arrays(out.belief)]
            arrs += [np.asarray(x) for x in L.struct_to_arrays(comb)]
            arrs += [np.asarray(x) for x in ctx.get_belief()]
            arrs += [cert, *ctx.iw_state(), *ctx.meas_iw_state(), m, d, ctx.get_scan_stats()]
            res.append(arrs)
        split, (n_scans, n_calls) = ctx.host_split()
        return res, split, n_scans, n_calls
    finally:
        ctx.close()


def _same(tag, a, b):
    for k, (x, y) in enumerate(zip(a, b)):
        assert len(x) == len(y)
        for i, (u, v) in enumerate(zip(x, y)):
            u, v = (np.ascontiguousarray(np.atleast_1d(np.asarray(z, np.float64))) for z in (u, v))
            assert np.array_equal(u.view(np.uint8), v.view(np.uint8)), (tag, "scan", k, "item", i)


@pytest.mark.parametrize("map_mode", ["own", "follow"])
@pytest.mark.parametrize("with_comm", [True, False])
def test_fused_step_matches_two_calls_bitwise(scans, with_comm, map_mode):
    from gcslam.distributed import HypothesisComm
    comm = HypothesisComm(0, 1, 0) if with_comm else None
    try:
        h = comm.h if comm is not None else None
        two, _, _, _ = _run(scans, False, h, map_mode)
        fused, split, n_scans, n_calls = _run(scans, True, h, map_mode)
        _same((with_comm, map_mode, "deferred"), two, fused)
        held, _, _, _ = _run(scans, True, h, map_mode, defer=0)
        _same((with_comm, map_mode, "not deferred"), two, held)
    finally:
        if comm is not None:
            comm.close()
    # the host split still adds up: the call is the scan plus the combine (which now holds the
    # pushforward's launch calls); between them lie only clock reads and two flag stores (1 ms per
    # scan allows for a descheduled thread)
    assert n_scans == N_SCANS and n_calls == N_SCANS
    assert split["scan_combine_call"] >= split["gcs_scan"] + split["combine"] - 1e-9
    assert split["scan_combine_call"] - split["gcs_scan"] - split["combine"] < 1.0 * N_SCANS
