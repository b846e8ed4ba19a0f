"""gcs_scan_begin on a scale-mode context (the live primitive path's first half).  Its point stage is the
deskew-only kernel k_points<false, 0>: it reads no bin data and writes per-point outputs, so its budget
comes from a real k_budget in either mode and a scale-mode context must give what a dense one gives,
bit for bit -- on a fresh context, and after a gcs_scan whose k_pt has already done the next scan's
clears (where a self-budget scan would launch no k_budget at all).  Two stride cases at cap 2,048:
2,048 raw points (stride 1) and 5,000 (stride 3, 1,667 selected: a ragged last block)."""

import numpy as np
import pytest

from gpu_util import device_scan

pytestmark = pytest.mark.gpu

ORIGIN = (0.0, 0.0, 0.5)
B, CAP = 2000, 2048


def _ctx(mode):
    from gcslam.context import HypothesisContext
    return HypothesisContext(n_bins=B, n_points_cap=CAP, max_raw_points=8192, mode=mode, lidar_origin=ORIGIN)


def _begin(ctx, sc, n_raw, noise):
    """scan_begin into caller-owned buffers -> (points, weights, timestamps, n_selected, deskew_ess, cert)."""
    import torch
    from gcslam.synthetic import scan_kwargs
    rec, t, w = device_scan(sc)
    bufs = (torch.zeros(CAP, 3, dtype=torch.float64, device="cuda:0"),
            torch.zeros(CAP, dtype=torch.float64, device="cuda:0"),
            torch.zeros(CAP, dtype=torch.float64, device="cuda:0"))
    o = ctx.scan_begin(rec, 16, t, w, n_raw, **scan_kwargs(sc), **noise, buffers=bufs)
    p, tt, ww = (x.cpu().numpy() for x in bufs)
    return p, ww, tt, int(o.n_selected), float(o.deskew_ess), np.array(o.cert[:])


@pytest.mark.parametrize("n_raw,n_sel", [(2048, 2048), (5000, 1667)])
def test_scan_begin_scale_mode_matches_dense_bitwise(n_raw, n_sel):
    from gcslam import synthetic
    from gcslam.synthetic import scan_kwargs
    from oracle import ops
    noise = dict(Q=ops.process_noise_Q(*ops.datasheet_process_noise_state()),
                 Sigma_g=1e-5 * np.eye(3), Sigma_a=1e-3 * np.eye(3))
    n_gen = 16 * ((n_raw + 15) // 16)
    sc0, sc1, sc2 = (synthetic.make_scan(n_gen, 50 + k) for k in range(3))
    scale, dense = _ctx("scale"), _ctx("dense")
    # fresh contexts: every output of the begin, bit for bit
    got, ref = _begin(scale, sc0, n_raw, noise), _begin(dense, sc0, n_raw, noise)
    assert got[3] == ref[3] == n_sel
    for name, a, b in zip(("points", "weights", "timestamps", "n_selected", "deskew_ess", "cert"), got, ref):
        assert np.array_equal(a, b, equal_nan=True), f"fresh {name}"
    assert np.count_nonzero(got[1]) > n_sel // 2 and np.all(np.isfinite(got[0]))
    # after a gcs_scan: its k_pt has cleared the next scan's counts and flags
    rec, t, w = device_scan(sc1)
    o = scale.scan(rec, 16, t, w, n_raw, **scan_kwargs(sc1), **noise)
    assert np.all(np.isfinite(np.array(o.z_t[:])))
    dense.set_belief(*scale.get_belief())
    got, ref = _begin(scale, sc2, n_raw, noise), _begin(dense, sc2, n_raw, noise)
    assert got[3] == ref[3] == n_sel
    for name, a, b in zip(("points", "weights", "timestamps"), got, ref):
        assert np.array_equal(a, b, equal_nan=True), f"after a scan: {name}"
    assert np.count_nonzero(got[1]) > n_sel // 2 and np.all(np.isfinite(got[0]))
    # and a scan afterwards
    rec, t, w = device_scan(sc2)
    o = scale.scan(rec, 16, t, w, n_raw, **scan_kwargs(sc2), **noise)
    assert np.all(np.isfinite(np.array(o.z_t[:]))) and o.cert[57] == 0
    scale.close()
    dense.close()
