"""gcs_match_descriptors_gated and gcs_match_pairs on the MI355X against tests/keypoints_gate_ref.py's numpy
restatement of D8 and D9: all four gated outputs, the three pair arrays with their tails and the count, as bytes, on
every fixture; bitwise repeatability; a reused context after a larger call; the pairs without a gate against
match_descriptors; the raw C chain detector -> describer -> gcs_match_pairs on a side stream with prefilled buffers and
the padding rows; the end-to-end pair; the refusals.  The shapes are the smallest at which the kernels can go wrong:
one row, 63 / 64 / 65 query rows (one wave and one row more), 257 x 513 (a partial workgroup, five chunks of train rows
of which the last holds one row), duplicates 300 rows apart in different chunks, 256 and 257 query rows (one compaction
workgroup and one row into the second), 1100 x 1100 (nine chunks each way, five compaction workgroups);
ramp_vga_k512 is the only large frame."""

import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import keypoints_desc_ref as DR
import keypoints_gate_ref as G
import keypoints_grid_ref as GR
import test_keypoints_gate_host as TH
import test_keypoints_grid_host as TG
from gcslam import _lib as L
from gcslam import descriptors as D
from gcslam import keypoints as KP

pytestmark = pytest.mark.gpu


def numpy_of(tensors):
    torch.cuda.synchronize()
    assert all(x.is_cuda and x.dtype == torch.int32 for x in tensors)
    return tuple(x.cpu().numpy() for x in tensors)


def device_pairs(m, name, gated, kw):
    q, t, q_bin, t_bin, gate = G.pairs_fixture(name)
    return numpy_of(m.queue_pairs(q, t, q_bin=q_bin, t_bin=t_bin, **kw, **(TH.gate_args(gate) if gated else {})))


@pytest.mark.parametrize("name", G.GATED_NAMES)
def test_device_gated_search_equals_the_restatement(name):
    q, t, q_bin, t_bin, gate = G.gated_fixture(name)
    m = D._matcher_for(0, len(q), len(t))
    TH.same(numpy_of(m.queue_gated(q, t, q_bin=q_bin, t_bin=t_bin, **TH.gate_args(gate))), G.gated_expected(name), name)


@pytest.mark.parametrize("name", G.PAIRS_NAMES)
def test_device_pairs_equal_the_restatement(name):
    q, t = G.pairs_fixture(name)[:2]
    m = D._matcher_for(0, len(q), len(t))
    for gated, kw in G.pairs_cases(name):
        TH.same(device_pairs(m, name, gated, kw), G.pairs_expected(name, gated, kw), (name, gated, kw))


@pytest.mark.parametrize("name", ["predicted", "ties", "gate_257x513", "edges", "edges_predicted"])
def test_device_pairs_on_the_gated_fixtures(name):
    q, t, q_bin, t_bin, gate = G.gated_fixture(name)
    G.gated_expected(name)
    m = D._matcher_for(0, len(q), len(t))
    for kw in G.FILTERS:
        got = numpy_of(m.queue_pairs(q, t, q_bin=q_bin, t_bin=t_bin, **kw, **TH.gate_args(gate)))
        TH.same(got, G.pairs(q, t, gate, q_bin, t_bin, **kw), (name, kw))


def test_two_calls_are_byte_identical():
    q, t, q_bin, t_bin, gate = G.gated_fixture("gate_257x513")
    m = D.DescriptorMatcher(D.MatchConfig(1100, 1100))
    a, b = (numpy_of(m.queue_gated(q, t, **TH.gate_args(gate))) for _ in range(2))
    TH.same(a, b, "gated")
    a, b = (device_pairs(m, "pairs_1100x1100", True, {}) for _ in range(2))
    TH.same(a, b, "pairs")
    m.close()


def test_a_reused_context_keeps_nothing_of_a_larger_call():
    m = D.DescriptorMatcher(D.MatchConfig(1100, 1100))
    big = device_pairs(m, "pairs_1100x1100", True, {})
    TH.same(big, G.pairs_expected("pairs_1100x1100", True, {}), "1100 x 1100")
    small = device_pairs(m, "pairs_63x70", True, {})
    TH.same(small, G.pairs_expected("pairs_63x70", True, {}), "63 x 70 after 1100 x 1100")
    q, t, q_bin, t_bin, gate = G.pairs_fixture("pairs_63x70")
    TH.same(numpy_of(m.queue_gated(q, t, q_bin=q_bin, t_bin=t_bin, **TH.gate_args(gate))),
            G.match_gated(q, t, gate, q_bin, t_bin), "gated 63 x 70 after 1100 x 1100")
    m.close()
    fresh = D.DescriptorMatcher(D.MatchConfig(63, 70))
    TH.same(device_pairs(fresh, "pairs_63x70", True, {}), small, "a fresh context")
    fresh.close()


def test_match_pairs_without_a_gate_is_match_descriptors():
    a, b = DR.expected("ramp_96x64_l3_k48_c16"), DR.expected("blocks_61x97_l3_k200_c16")
    da, db = (D.Descriptors(*(torch.from_numpy(np.array(r[k])).cuda() for k in ("desc", "angle", "angle_bin"))) for r in (a, b))
    for kw in (dict(), dict(cross_check=False), dict(ratio=(9, 10)), dict(max_distance=40, ratio=None)):
        got, want = D.match_pairs(da, db, gate=None, **kw), D.match_descriptors(da, db, **kw)
        assert all(g.is_cuda and g.dtype == torch.int32 for g in got) and len(want[0]) > 0
        for g, w in zip(got, want):
            assert g.cpu().numpy().tobytes() == w.cpu().numpy().astype(np.int32).tobytes(), kw
    same = D.match_pairs(da, da)
    assert (same[0] == same[1]).all() and (same[2] == 0).all() and len(same[0]) > 40
    none = D.match_pairs(da, D.Descriptors(db.desc[:0], db.angle[:0], db.angle_bin[:0]))
    assert all(len(x) == 0 for x in none)
    with pytest.raises(ValueError):
        D.match_pairs(da, db, gate=D.GateConfig())


def test_c_route_chains_detector_describer_and_pairs_with_the_padding_and_no_wait(lib):
    """gcs_detect_keypoints_grid, gcs_describe_keypoints with n_keypoints = max_keypoints and the NaN / -1 padded arrays,
    then gcs_match_pairs of the set against itself -- the detector's positions and levels as the gate, the bins as
    q_bin and t_bin -- all queued on a side stream into prefilled buffers with nothing between them: every valid row
    pairs with itself at distance 0 and the padding rows produce nothing."""
    name, cap = "ramp_200x150_k512_c16", 512
    rgb = np.array(GR.image(name))
    H, W = rgb.shape[:2]
    ref = GR.expected(name)
    n = ref["counts"][0]
    assert n == 467 < cap
    gc = KP.grid_config_struct(TG.grid_config(name, max_width=256, max_height=256))
    dc = D.config_struct(D.DescriptorConfig(max_width=256, max_height=256, max_keypoints=cap))
    mc = D.match_config_struct(D.MatchConfig(cap, cap))
    gh, dh, mh = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert lib.gcs_keypoint_grid_ctx_create(C.byref(gc), C.byref(gh)) == 0
    assert lib.gcs_keypoint_desc_ctx_create(C.byref(dc), C.byref(dh)) == 0
    assert lib.gcs_match_ctx_create(C.byref(mc), C.byref(mh)) == 0
    side = torch.cuda.Stream()
    rgb_d = torch.from_numpy(rgb).cuda()
    kp = torch.full((3, cap), 7.0, dtype=torch.float32, device="cuda")
    level = torch.full((cap,), 99, dtype=torch.int32, device="cuda")
    words = torch.full((52,), -1, dtype=torch.int32, device="cuda")
    angle = torch.full((cap,), 7.0, dtype=torch.float32, device="cuda")
    bins = torch.full((cap,), 99, dtype=torch.int32, device="cuda")
    desc = torch.full((cap, 32), 0xAB, dtype=torch.uint8, device="cuda")
    out = torch.full((3, cap), 99, dtype=torch.int32, device="cuda")
    count = torch.full((1,), 99, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()   # the inputs above were made on the default stream
    ki = KP._inputs_struct(rgb_d.data_ptr(), 3, rgb_d.stride(0), W, H)
    ko = L.GcsKeypointGridOutputs(kp[0].data_ptr(), kp[1].data_ptr(), kp[2].data_ptr(), level.data_ptr(),
                                  words.data_ptr(), words[4:].data_ptr())
    dk = L.GcsKeypointDescKeypoints(cap, kp[0].data_ptr(), kp[1].data_ptr(), level.data_ptr())
    do = L.GcsKeypointDescOutputs(angle.data_ptr(), bins.data_ptr(), desc.data_ptr())
    mi = L.GcsMatchInputs(cap, cap, desc.data_ptr(), desc.data_ptr(), bins.data_ptr(), bins.data_ptr())
    mg = L.GcsMatchGate(kp[0].data_ptr(), kp[1].data_ptr(), level.data_ptr(), kp[0].data_ptr(), kp[1].data_ptr(),
                        level.data_ptr(), None, None, 8.0, 1)
    mf = L.GcsMatchFilter()
    assert lib.gcs_match_filter_defaults(C.byref(mf)) == 0
    mo = L.GcsMatchPairOutputs(out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), count.data_ptr())
    for h, setter in ((gh, lib.gcs_keypoint_grid_ctx_set_stream), (dh, lib.gcs_keypoint_desc_ctx_set_stream),
                      (mh, lib.gcs_match_ctx_set_stream)):
        assert setter(h, C.c_void_p(side.cuda_stream)) == 0
    assert lib.gcs_detect_keypoints_grid(gh, C.byref(ki), C.byref(ko)) == 0, lib.gcs_keypoint_grid_last_error(gh)
    assert lib.gcs_describe_keypoints(dh, C.byref(ki), C.byref(dk), C.byref(do)) == 0, lib.gcs_keypoint_desc_last_error(dh)
    assert lib.gcs_match_pairs(mh, C.byref(mi), C.byref(mg), C.byref(mf), C.byref(mo)) == 0, lib.gcs_match_last_error(mh)
    side.synchronize()
    assert words.cpu().tolist()[:4] == [n, n, ref["counts"][2], 8]
    b = bins.cpu().numpy()
    assert (b[:n] >= 0).all() and (b[n:] == -1).all()
    pa, pb, pd = (x.cpu().numpy() for x in out)
    want = G.pairs(desc.cpu().numpy()[:n], desc.cpu().numpy()[:n],
                   G.gate_of(ref["u"], ref["v"], ref["level"], ref["u"], ref["v"], ref["level"], radius=8.0))
    m = int(count.item())
    print(f"{m} of {n} valid rows pair with themselves")
    assert m == int(want[3][0]) and pa[:m].tobytes() == want[0][:m].tobytes() and pb[:m].tobytes() == want[1][:m].tobytes()
    assert (pa[:m] == pb[:m]).all() and (pd[:m] == 0).all() and (pa[:m] < n).all() and m > n // 2
    assert (pa[m:] == -1).all() and (pb[m:] == -1).all() and (pd[m:] == 257).all()
    # without the ratio test (a corner found on two levels is its own second nearest) every valid row is there
    mf.ratio_den = 0
    assert lib.gcs_match_pairs(mh, C.byref(mi), C.byref(mg), C.byref(mf), C.byref(mo)) == 0
    side.synchronize()
    pa, pb, pd = (x.cpu().numpy() for x in out)
    dup = np.array([(desc.cpu().numpy()[:i] == desc.cpu().numpy()[i]).all(1).any() for i in range(n)])
    assert int(count.item()) >= n - int(dup.sum())
    assert (pd[:int(count.item())] == 0).all() and (pa[int(count.item()):] == -1).all()
    assert lib.gcs_keypoint_grid_ctx_destroy(gh) == 0 and lib.gcs_keypoint_desc_ctx_destroy(dh) == 0
    assert lib.gcs_match_ctx_destroy(mh) == 0


def _end_to_end(detect, build, want):
    a_img, b_img = np.array(GR.image(DR.VGA)), DR.shifted_image()
    ka, kb = detect(a_img), detect(b_img)
    a, b, gate, ref = build()
    for k, u, lv in ((ka, gate["q_u"], gate["q_level"]), (kb, gate["t_u"], gate["t_level"])):
        assert k[0].cpu().numpy().tobytes() == u.tobytes() and k.level.cpu().numpy().tobytes() == lv.tobytes()
    ia, ib, dist = D.match_pairs(D.describe_keypoints(a_img, ka), D.describe_keypoints(b_img, kb), ka, kb,
                                 gate=D.GateConfig(**G.VGA_GATE))
    ia, ib, dist = numpy_of((ia, ib, dist))
    n = int(ref[3][0])
    print(f"pairs {len(ia)} of 512")
    assert ia.tobytes() == ref[0][:n].tobytes() and ib.tobytes() == ref[1][:n].tobytes() and dist.tobytes() == ref[2][:n].tobytes()
    ua, va, ub, vb = (x.cpu().numpy() for x in (ka[0], ka[1], kb[0], kb[1]))
    la, lb = ka.level.cpu().numpy(), kb.level.cpu().numpy()
    G._vga_check(ua, va, la, ub, vb, lb, (ia, ib, dist, np.array([len(ia)], np.int32)), want, 0)
    du, dv = ub[ib] - ua[ia], vb[ib] - va[ia]
    assert (np.abs(du) <= 8).all() and (np.abs(dv) <= 8).all() and 512 - len(ia) <= 512 - want[0]


def test_end_to_end_gated_with_the_pyramid_detector():
    """ramp_vga_k512 and the same frame moved by (5, 3): detect, describe, match_pairs with radius 8, level diff 1 and
    a null prediction.  The restatement's pairs byte for byte: 305 (the ungated matcher finds 290), 112 of them on level
    0, all 112 by exactly the shift; every pair on any level lies within the window."""
    cfg = KP.PyramidConfig(max_keypoints=512)
    _end_to_end(lambda img: KP.detect_keypoints_pyramid(img, cfg), G.vga_pyramid_gated, G.VGA_GATED_PYRAMID)
    assert G.VGA_GATED_PYRAMID == (305, 112, 112) and G.VGA_GATED_PYRAMID[0] >= DR.VGA_PYRAMID_PAIRS


def test_end_to_end_gated_with_the_grid_detector():
    """The same through GridDetector: 284 pairs (241 ungated), 82 on level 0, 78 of them by exactly the shift; the other
    four are keypoints whose partner the grid did not keep, and the window bounds their error to its radius."""
    cfg = KP.GridConfig(**dict(GR.config(DR.VGA), redistribute=True))
    _end_to_end(lambda img: KP.detect_keypoints_grid(img, cfg), G.vga_grid_gated, G.VGA_GATED_GRID)
    assert G.VGA_GATED_GRID == (284, 82, 78)


def test_device_entries_refuse_bad_inputs_and_stay_usable(lib):
    m = D.DescriptorMatcher(D.MatchConfig(8, 8))
    q = torch.from_numpy(DR._rows(8, 95)).cuda()
    pos = torch.zeros((5, 8), dtype=torch.float32, device="cuda")
    out = torch.full((4, 8), 99, dtype=torch.int32, device="cuda")
    count = torch.full((1,), 99, dtype=torch.int32, device="cuda")

    def call():
        i = L.GcsMatchInputs(3, 5, q.data_ptr(), q.data_ptr(), None, None)
        g = L.GcsMatchGate(pos[0].data_ptr(), pos[1].data_ptr(), None, pos[2].data_ptr(), pos[3].data_ptr(), None, None, None,
                           8.0, 1)
        f = L.GcsMatchFilter(64, 4, 5, 1)
        o = L.GcsMatchGatedOutputs(*(out[k].data_ptr() for k in range(4)))
        p = L.GcsMatchPairOutputs(*(out[k].data_ptr() for k in range(3)), count.data_ptr())
        return i, g, f, o, p

    for field, value in TH.BAD_GATE + TH.BAD_FILTER + [("count", None)]:
        i, g, f, o, p = call()
        target = next(s for s in (i, g, f, o, p) if hasattr(s, field))
        setattr(target, field, pos[4].data_ptr() if value == "set" else value)
        if target is not f and target is not p:
            assert lib.gcs_match_descriptors_gated(m.h, C.byref(i), C.byref(g), C.byref(o)) == -1, (field, value)
            assert lib.gcs_match_last_error(m.h)
        assert lib.gcs_match_pairs(m.h, C.byref(i), C.byref(g), C.byref(f), C.byref(p)) == -1, (field, value)
        assert lib.gcs_match_last_error(m.h)
    torch.cuda.synchronize()
    assert (out == 99).all() and count.item() == 99   # a refused call queues nothing
    i, g, f, o, p = call()
    assert lib.gcs_match_ctx_set_stream(m.h, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    assert lib.gcs_match_pairs(m.h, C.byref(i), C.byref(g), C.byref(f), C.byref(p)) == 0
    torch.cuda.synchronize()
    assert count.item() == 3 and out[0, :3].tolist() == [0, 1, 2] and out[2, :3].tolist() == [0, 0, 0]
    with pytest.raises(ValueError):
        m.queue_gated(q, q, (pos[0], pos[1]), (pos[0][:5], pos[1][:5]))
    with pytest.raises(ValueError):
        m.queue_pairs(q, q, kp_q=(pos[0], pos[1]))
    with pytest.raises(ValueError):
        m.queue_pairs(np.zeros((9, 32), np.uint8), q)
    got = numpy_of(m.queue_pairs(q, q, (pos[0], pos[1]), (pos[0], pos[1])))
    assert got[3].tolist() == [8] and got[0].tolist() == list(range(8))
    m.close()
