"""gcs_describe_keypoints and gcs_match_descriptors on the MI355X: the device results against
tests/keypoints_desc_ref.py's numpy restatement of D1-D7 on every fixture -- bins, descriptors and match outputs as
bytes, the informative angle within one float32 ulp (the comparisons of tests/test_keypoints_desc_host.py); the
quarter-turn property; bitwise repeatability; a context reused for a smaller image; row pitch; the raw C chain
detector -> describer -> matcher on a side stream with the NaN padding; and the end-to-end pair.  The shapes are the
smallest at which the kernels can go wrong: keypoints on the 16-pixel margin, counts of 1 and of no multiple of four
(four keypoints to a workgroup), n = 0, a 33 x 33 image that is one patch, 257 x 513 descriptors (two workgroups of
queries, two chunks of train rows, a partial tile); ramp_vga_k512 is the only large frame."""

import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import keypoints_desc_ref as DR
import keypoints_grid_ref as GR
import keypoints_ref as KR
import test_keypoints_desc_host as TH
import test_keypoints_grid_host as TG
from gcslam import _lib as L
from gcslam import descriptors as D
from gcslam import keypoints as KP

pytestmark = pytest.mark.gpu


def numpy_of(d):
    torch.cuda.synchronize()
    return D.Descriptors(d.desc.cpu().numpy(), d.angle.cpu().numpy(), d.angle_bin.cpu().numpy())


def device(name, image=None, describer=None, **over):
    img, cfg, u, v, level = DR.fixture(name)
    img = np.array(img) if image is None else image
    d = describer or D._describer_for(TH.desc_config(name, **over), 0, img.shape[0], img.shape[1], len(u))
    return numpy_of(d.queue(img, u, v, level))


def same_bytes(a, b):
    assert a.desc.tobytes() == b.desc.tobytes() and a.angle_bin.tobytes() == b.angle_bin.tobytes()
    assert a.angle.tobytes() == b.angle.tobytes()


@pytest.mark.parametrize("name", DR.NAMES)
def test_device_describer_equals_the_restatement(name):
    ref = DR.expected(name)
    TH.same_as_ref(device(name), ref, name)
    img = DR.fixture(name)[0]
    if img.ndim == 3:   # the fixture is rgb: its own grey image gives the same bytes
        TH.same_as_ref(device(name, KR.grey(img)), ref, (name, "gray"))
    elif img.size:      # the fixture is gray: the same value in three channels is that grey again
        TH.same_as_ref(device(name, np.repeat(np.array(img)[:, :, None], 3, 2)), ref, (name, "rgb"))


def test_describe_returns_device_tensors():
    name = "ramp_96x64_l3_k48_c16"
    ref = DR.expected(name)
    kp = KP.detect_keypoints_grid(np.array(GR.image(name)), TG.grid_config(name, edge_threshold=16))
    got = D.describe_keypoints(np.array(GR.image(name)), kp, TH.desc_config(name))
    assert got.desc.is_cuda and got.desc.shape == (48, 32) and got.desc.dtype == torch.uint8 and len(got) == 48
    assert got.angle.is_cuda and got.angle.dtype == torch.float32 and got.angle_bin.is_cuda and got.angle_bin.dtype == torch.int32
    TH.same_as_ref(numpy_of(got), ref, name)
    one = D.describe_keypoints(np.array(DR.fixture("quarter_64")[0]), KP.detect_keypoints(
        np.array(DR.fixture("quarter_64")[0]), KP.KeypointConfig(edge_threshold=16)), D.DescriptorConfig(n_levels=1))
    assert len(one) > 0 and (one.angle_bin >= 0).all()   # a single-level detector's result: level 0


def test_a_quarter_turn_moves_every_bin_by_8_and_keeps_the_descriptor():
    """As tests/test_keypoints_desc_host.py's: np.rot90 moves every bin by -8 mod 32 and keeps the 256 bits."""
    a, b = device("quarter_64"), device("quarter_64_turned")
    assert not DR.expected("quarter_64")["tie"].any()
    assert (a.angle_bin >= 0).all() and len(a) == 13
    assert (b.angle_bin == (a.angle_bin - 8) % 32).all(), (a.angle_bin, b.angle_bin)
    assert a.desc.tobytes() == b.desc.tobytes() and a.desc.any()


def test_two_calls_are_byte_identical():
    for name in (DR.VGA, "blocks_61x97_l3_k200_c16"):
        same_bytes(device(name), device(name))
    q, t, _, _ = DR.match_fixture("257x513")
    m = D.DescriptorMatcher(D.MatchConfig(257, 513))
    a, b = [x.cpu().numpy() for x in m.queue(q, t)], [x.cpu().numpy() for x in m.queue(q, t)]
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    m.close()


def test_a_reused_context_keeps_nothing_of_a_larger_frame():
    cfg = TH.desc_config("ramp_96x64_l3_k48_c16", max_width=640, max_height=480, max_keypoints=512)
    one = D.KeypointDescriber(cfg)
    big = device(DR.VGA, describer=one)   # (the describer has 3 levels: the rows of levels 3..7 come out invalid)
    assert (big.angle_bin >= 0).sum() == int((DR.fixture(DR.VGA)[4] < 3).sum()) > 200
    small = device("ramp_96x64_l3_k48_c16", describer=one)
    one.close()
    fresh = D.KeypointDescriber(cfg)
    same_bytes(small, device("ramp_96x64_l3_k48_c16", describer=fresh))
    fresh.close()
    TH.same_as_ref(small, DR.expected("ramp_96x64_l3_k48_c16"), "96 x 64 after vga")


@pytest.mark.parametrize("name", ["ramp_96x64_l3_k48_c16", "hand_40x40"])
def test_a_torch_view_keeps_its_row_pitch(name):
    src, cfg, u, v, level = DR.fixture(name)
    img = torch.from_numpy(np.array(src)).cuda()
    H, W = img.shape[0], img.shape[1]
    wide = torch.full((H, W + 7) + tuple(img.shape[2:]), 255, dtype=torch.uint8, device="cuda")
    wide[:, :W] = img
    view = wide[:, :W]
    assert not view.is_contiguous()
    d = D.KeypointDescriber(TH.desc_config(name, max_width=128, max_height=128))
    assert d._image(view)[0].data_ptr() == wide.data_ptr()   # passed as it is, rows (W + 7) pixels apart
    got = numpy_of(d.queue(view, u, v, level))
    same_bytes(got, numpy_of(d.queue(img, u, v, level)))
    TH.same_as_ref(got, DR.expected(name), name)
    d.close()


def test_device_entries_refuse_bad_inputs(lib):
    d = D.KeypointDescriber(D.DescriptorConfig(max_width=48, max_height=48, max_keypoints=8))
    img = torch.zeros((48, 144), dtype=torch.uint8, device="cuda")
    rows = torch.full((3, 8), 20.0, dtype=torch.float32, device="cuda")
    ints = torch.zeros((2, 8), dtype=torch.int32, device="cuda")
    desc = torch.zeros((8, 32), dtype=torch.uint8, device="cuda")
    for field, value in TH.BAD_INPUTS:
        i = KP._inputs_struct(img.data_ptr(), 1, 144, 40, 40)
        k = L.GcsKeypointDescKeypoints(4, rows[0].data_ptr(), rows[1].data_ptr(), ints[0].data_ptr())
        o = L.GcsKeypointDescOutputs(rows[2].data_ptr(), ints[1].data_ptr(), desc.data_ptr())
        setattr(next(s for s in (i, k, o) if hasattr(s, field)), field, value)
        assert lib.gcs_describe_keypoints(d.h, C.byref(i), C.byref(k), C.byref(o)) == -1, (field, value)
        assert lib.gcs_keypoint_desc_last_error(d.h)
    with pytest.raises(ValueError):
        d.queue(torch.zeros((49, 8), dtype=torch.uint8), rows[0], rows[1])
    d.close()
    m = D.DescriptorMatcher(D.MatchConfig(8, 8))
    with pytest.raises(ValueError):
        m.queue(np.zeros((9, 32), np.uint8), np.zeros((3, 32), np.uint8))
    with pytest.raises(ValueError):
        m.queue(np.zeros((3, 32), np.uint8), np.zeros((3, 32), np.uint8), np.zeros(2, np.int32))
    m.close()


# ---- the matcher

@pytest.mark.parametrize("name", DR.MATCH_NAMES)
def test_device_matcher_equals_the_restatement(name):
    q, t, q_bin, t_bin = DR.match_fixture(name)
    want = DR.match_expected(name)
    m = D._matcher_for(0, len(q), len(t))
    got = m.queue(q, t, q_bin, t_bin)
    torch.cuda.synchronize()
    for g, w, k in zip(got, want, ("idx", "dist", "dist2")):
        assert g.is_cuda and g.dtype == torch.int32 and g.cpu().numpy().tobytes() == w.tobytes(), (name, k)


def test_match_descriptors_applies_the_filters_on_the_device():
    a, b = DR.expected("ramp_96x64_l3_k48_c16"), DR.expected("blocks_61x97_l3_k200_c16")
    da, db = (D.Descriptors(*(torch.from_numpy(np.array(r[k])).cuda() for k in ("desc", "angle", "angle_bin"))) for r in (a, b))
    for kw in (dict(), dict(cross_check=False), dict(ratio=(9, 10)), dict(max_distance=40, ratio=None)):
        got = D.match_descriptors(da, db, **kw)
        want = D.match_descriptors_host(D.Descriptors(a["desc"], a["angle"], a["angle_bin"]),
                                        D.Descriptors(b["desc"], b["angle"], b["angle_bin"]), **kw)
        assert all(g.is_cuda for g in got)
        for g, w in zip(got, want):
            assert g.cpu().numpy().astype(np.int32).tobytes() == w.tobytes(), kw
    same = D.match_descriptors(da, da)
    assert (same[0] == same[1]).all() and (same[2] == 0).all() and len(same[0]) > 40
    none = D.match_descriptors(da, D.Descriptors(db.desc[:0], db.angle[:0], db.angle_bin[:0]))
    assert all(len(x) == 0 for x in none)


# ---- chaining

def test_c_route_chains_detector_describer_and_matcher_with_the_padding_and_no_wait(lib):
    """gcs_detect_keypoints_grid, gcs_describe_keypoints with n_keypoints = max_keypoints and the NaN / -1 padded
    arrays, then gcs_match_descriptors of the set against itself with the bins as q_bin and t_bin, all queued on a
    side stream with nothing between them: the padded rows come out invalid and the matcher ignores them."""
    name, cap = "ramp_200x150_k512_c16", 512
    rgb = np.array(GR.image(name))
    H, W = rgb.shape[:2]
    ref = GR.expected(name)
    n = ref["counts"][0]
    assert n == 467 < cap
    want = DR.describe(rgb, ref["u"], ref["v"], ref["level"])
    assert (want["angle_bin"] >= 0).all()
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
    torch.cuda.synchronize()   # the inputs above were made on the default stream
    ki = KP._inputs_struct(rgb_d.data_ptr(), 3, rgb_d.stride(0), W, H)
    ko = L.GcsKeypointGridOutputs(kp[0].data_ptr(), kp[1].data_ptr(), kp[2].data_ptr(), level.data_ptr(),
                                  words.data_ptr(), words[4:].data_ptr())
    dk = L.GcsKeypointDescKeypoints(cap, kp[0].data_ptr(), kp[1].data_ptr(), level.data_ptr())
    do = L.GcsKeypointDescOutputs(angle.data_ptr(), bins.data_ptr(), desc.data_ptr())
    mi = L.GcsMatchInputs(cap, cap, desc.data_ptr(), desc.data_ptr(), bins.data_ptr(), bins.data_ptr())
    mo = L.GcsMatchOutputs(out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr())
    for h, setter in ((gh, lib.gcs_keypoint_grid_ctx_set_stream), (dh, lib.gcs_keypoint_desc_ctx_set_stream),
                      (mh, lib.gcs_match_ctx_set_stream)):
        assert setter(h, C.c_void_p(side.cuda_stream)) == 0
    assert lib.gcs_detect_keypoints_grid(gh, C.byref(ki), C.byref(ko)) == 0, lib.gcs_keypoint_grid_last_error(gh)
    assert lib.gcs_describe_keypoints(dh, C.byref(ki), C.byref(dk), C.byref(do)) == 0, lib.gcs_keypoint_desc_last_error(dh)
    assert lib.gcs_match_descriptors(mh, C.byref(mi), C.byref(mo)) == 0, lib.gcs_match_last_error(mh)
    side.synchronize()
    assert words.cpu().tolist()[:4] == [n, n, ref["counts"][2], 8]
    b, a, d = bins.cpu().numpy(), angle.cpu().numpy(), desc.cpu().numpy()
    assert (b[n:] == -1).all() and np.isnan(a[n:]).all() and (d[n:] == 0).all()
    TH.same_as_ref(D.Descriptors(d[:n], a[:n], b[:n]), want, name)
    idx, dist, dist2 = (x.cpu().numpy() for x in out)
    assert (idx[n:] == -1).all() and (dist[n:] == 257).all() and (dist2[n:] == 257).all()
    wi, wd, wd2 = DR.match(want["desc"], want["desc"])
    assert idx[:n].tobytes() == wi.tobytes() and dist[:n].tobytes() == wd.tobytes() and dist2[:n].tobytes() == wd2.tobytes()
    assert (dist[:n] == 0).all() and (idx[:n] <= np.arange(n)).all()
    assert lib.gcs_keypoint_grid_ctx_destroy(gh) == 0 and lib.gcs_keypoint_desc_ctx_destroy(dh) == 0
    assert lib.gcs_match_ctx_destroy(mh) == 0


def test_end_to_end_a_shifted_frame_matches_by_its_shift():
    """ramp_vga_k512 and the same image moved by (5, 3) pixels: detect, describe, match_descriptors with its defaults;
    every returned pair whose two keypoints are on level 0 differs by exactly the shift, there is at least one, and
    no more keypoints stay without a partner than in the numpy restatement (keypoints_desc_ref.VGA_PYRAMID_UNMATCHED_CAP,
    computed there on the CPU).

    The detector is PyramidDetector (the fixture's fields it has: max_keypoints 512, 8 levels at 6 / 5).  The property
    is one of the describer and the matcher only if the detector keeps the same corners in both images, that is if
    its choice moves with the picture.  On level 0 the pyramid detector's does: the level is the image itself, the
    responses move with the pixels, and the quota's best by response are the same corners wherever they lie (the
    border of 31 pixels aside).  The grid detector's does not: G1 anchors its cells at (e, e) of the image, so a shift
    that is no multiple of the cell size changes which corners share a cell and which of them are kept; a keypoint
    whose partner was not kept can only be paired wrongly.  That case is the next test."""
    cfg = KP.PyramidConfig(max_keypoints=512)
    a_img, b_img = np.array(GR.image(DR.VGA)), DR.shifted_image()
    ka, kb = KP.detect_keypoints_pyramid(a_img, cfg), KP.detect_keypoints_pyramid(b_img, cfg)
    ra, rb, wa, wb, wd = DR.vga_pyramid_pair()
    for k, r in ((ka, ra), (kb, rb)):
        assert k[0].cpu().numpy().tobytes() == r["u"].tobytes() and k.level.cpu().numpy().tobytes() == r["level"].tobytes()
    ia, ib, dist = (x.cpu().numpy() for x in D.match_descriptors(D.describe_keypoints(a_img, ka), D.describe_keypoints(b_img, kb)))
    print(f"pairs {len(ia)} of 512")
    assert ia.astype(np.int32).tobytes() == wa.tobytes() and ib.tobytes() == wb.tobytes() and dist.tobytes() == wd.tobytes()
    assert 512 - len(ia) <= DR.VGA_PYRAMID_UNMATCHED_CAP
    la, lb = ka.level.cpu().numpy()[ia], kb.level.cpu().numpy()[ib]
    level0 = (la == 0) & (lb == 0)
    assert level0.sum() >= 1
    du = kb[0].cpu().numpy()[ib] - ka[0].cpu().numpy()[ia]
    dv = kb[1].cpu().numpy()[ib] - ka[1].cpu().numpy()[ia]
    assert (du[level0] == DR.SHIFT[0]).all() and (dv[level0] == DR.SHIFT[1]).all(), (du[level0], dv[level0])


def test_end_to_end_with_the_grid_detector_gives_the_restated_pairs():
    """The same two images through GridDetector (the fixture's own config).  The device returns exactly the pairs of
    the numpy restatement: 241, of which 81 have both keypoints on level 0, and 78 of those differ by exactly the
    shift.  The other three -- (173, 63) -> (226, 338) at distance 11, (191, 77) -> (164, 96) at 16, (127, 223) ->
    (130, 226) at 14 -- are keypoints whose partner the grid detector did not keep in the moved image (its cells do
    not move with the picture) and whose nearest row is another corner of the block pattern with the same brightness
    order; the ratio and cross checks cannot tell them from true pairs, a search window could."""
    cfg = KP.GridConfig(**dict(GR.config(DR.VGA), redistribute=True))
    a_img, b_img = np.array(GR.image(DR.VGA)), DR.shifted_image()
    ka, kb = KP.detect_keypoints_grid(a_img, cfg), KP.detect_keypoints_grid(b_img, cfg)
    fa, fb = DR.fixture(DR.VGA), DR.fixture("ramp_vga_k512_shifted")
    for k, f in ((ka, fa), (kb, fb)):
        assert k[0].cpu().numpy().tobytes() == f[2].tobytes() and k.level.cpu().numpy().tobytes() == f[4].tobytes()
    da, db = D.describe_keypoints(a_img, ka), D.describe_keypoints(b_img, kb)
    ia, ib, dist = (x.cpu().numpy() for x in D.match_descriptors(da, db))
    wa, wb, wd, both0, exact = DR.vga_pair_matches()
    assert ia.astype(np.int32).tobytes() == wa.tobytes() and ib.tobytes() == wb.tobytes() and dist.tobytes() == wd.tobytes()
    assert 512 - len(ia) <= DR.VGA_UNMATCHED_CAP
    level0 = (ka.level.cpu().numpy()[ia] == 0) & (kb.level.cpu().numpy()[ib] == 0)
    du = kb[0].cpu().numpy()[ib] - ka[0].cpu().numpy()[ia]
    dv = kb[1].cpu().numpy()[ib] - ka[1].cpu().numpy()[ia]
    hit = level0 & (du == DR.SHIFT[0]) & (dv == DR.SHIFT[1])
    assert (int(level0.sum()), int(hit.sum())) == (DR.VGA_PAIRS_LEVEL0, DR.VGA_PAIRS_EXACT)
