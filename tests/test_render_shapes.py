"""CPU tests of the renderer's edge fixtures (tests/golden/render_edges.npz, recorded from the reference by
tests/golden/make_render.py): tests/render_util.py's numpy restatements of binning, tile render and the
prepare stage against the recorded indices, tiles and per-row records, and the host build of the prepare
kernel's rows (gcs_render_prepare_host) against the same records, before test_gpu_render_shapes.py leans
on either.

Bars: indices and counts equal; tiles at rtol 1e-12; per-row records at rtol 1e-9, atol 0
(RU.assert_record), the project's bar for routes without an eigenvector.  The `hard` scene is built with
cond(Sigma') <= 1e6, where the recorded rows (slogdet, np.linalg.inv, eigvalsh) and the closed forms
agree far inside that bar.  Worst relative difference measured per family of the `hard` scene, over
means, Sigma^-1, radius, alpha and colour (host build / prepare_np):
  surfel 8.8e-15 / 7.1e-15     thin 1.7e-14 / 9.5e-15       needle 2.5e-11 / 3.4e-11   huge 7.4e-15 / 3.6e-15
  tiny 1.4e-14 / 9.0e-16       kappa0 1.1e-14 / 1.2e-15     kappa1e4 1.5e-14 / 4.7e-15
  antiparallel 3.8e-15 / 4.6e-16   zero_dir 2.8e-15 / 1.6e-16   colour_range 4.5e-15 / 3.8e-15
  ulp_asym 3.6e-15 / 1.1e-15
(the test prints them; the needles' cond(Sigma') runs from 1.2e5 to 8.8e5, and the difference grows like
cond * 2^-53).  The one-ulp asymmetric covariances meet the bar with the kernel's lower-triangle read of the
log-determinant: the reference's slogdet reads the whole matrix, and the difference stays at rounding
level.

The tile restatement forms the first product of d . Sigma^-1 . d with numpy's matmul, as the reference does.
On the needles that product cancels, so whether the BLAS build fuses it shows at 1e-11 in a weight: the
plain expression is 7.2e-12 from the recorded `hard` tiles, the matmul one 3.8e-14.  A numpy build whose 2 x 2
matmul rounds otherwise than the recording one's can therefore miss rtol 1e-12 on
test_render_restatement_matches_the_recorded_edges[hard] with nothing wrong in the project; the kernel itself
is held to the fixture at 1e-9 (test_gpu_render_shapes.py), which both expressions meet.

The `cfg` case (eps 1e-2) is the one that showed the prepare rows normalising the view direction and the lobe
with the config's eps, where vmf_shading_multi_lobe keeps its own 1e-12: shaded colours off by up to 40 %."""

import numpy as np
import pytest

import render_util as RU
from gcslam import rendering as R

TILE_CASES = tuple(c for c in RU.EDGE_CASES if c != "lattice")      # the lattice case records indices only
KEYS = ("means", "Sigmas_inv", "radii", "alphas", "colors")


def _inputs(case):
    return (case["positions"], case["covariances"], case["directions"], case["kappas"], case["colors"],
            case["valid_mask"], case["P_pix"], case["offsets"], case["view_dirs"])


def _worst(got, case, rows):
    """Largest relative difference over the record's fields on `rows` (0 where both are 0)."""
    s = case["fbm_modulate_scale"]
    mod = ((1.0 - s) + s * case["fbm"])[None, :, None] if s > 0 else 1.0
    want = dict(means=case["means"], Sigmas_inv=case["Sigmas_inv"], radii=case["radii"], alphas=case["alphas"],
                colors=case["shaded"] * mod)
    worst = 0.0
    for k in KEYS:
        g, w = (got[k][rows], want[k][rows]) if k == "alphas" else (got[k][:, rows], want[k][:, rows])
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.where(w == g, 0.0, np.abs(g - w) / np.abs(w))
        worst = max(worst, float(rel.max(initial=0.0)))
    return worst


@pytest.mark.parametrize("name", RU.EDGE_CASES)
def test_bin_restatement_matches_the_recorded_edges(name):
    """Indices and counts, tie order included: the lattice case's cap falls inside a group of exact ties."""
    case = RU.load_case(name)
    cfg = RU.splat_config(case)
    valid = case["valid_mask"].astype(bool)
    # the recorded radii come from eigvalsh; the closed form's lambda_min loses about cond * 2^-53 to the
    # subtraction (1e-10 at the needles' cond 1e6): the per-row bar, far inside the fixtures' margins
    np.testing.assert_allclose(RU.radii_from_inverse(case["Sigmas_inv"][:, valid], cfg.eps), case["radii"][:, valid],
                               rtol=1e-9, atol=0)
    idx, cnt = RU.bin_tiles_np(case["means"], case["radii"], case["width"], case["height"], cfg.tile_size,
                               cfg.max_splats_per_tile)
    assert np.array_equal(idx, case["tile_indices"]) and np.array_equal(cnt, case["tile_counts"])


@pytest.mark.parametrize("name", TILE_CASES)
def test_render_restatement_matches_the_recorded_edges(name):
    case = RU.load_case(name)
    cfg = RU.splat_config(case)
    tiles = RU.render_tiles_np(case["means"], case["Sigmas_inv"], case["alphas"], case["shaded"], case["tile_indices"],
                               case["tile_counts"], case["width"], case["height"], cfg.tile_size, cfg.ewa_log_clip)
    assert tiles.shape == case["tiles"].shape
    np.testing.assert_allclose(tiles, case["tiles"], rtol=1e-12, atol=0)


def test_render_restatement_takes_per_view_alphas():
    """alphas (V, N): every view equals that view rendered alone with its own (N,) alphas."""
    case = RU.load_case("tile5")
    cfg = RU.splat_config(case)
    rng = np.random.default_rng(31)
    V, n = case["n_views"], case["alphas"].shape[0]
    al = rng.uniform(0.05, 1.0, (V, n))
    args = lambda v: (case["means"][v], case["Sigmas_inv"][v], al[v], case["shaded"][v], case["tile_indices"][v],   # noqa: E731
                      case["tile_counts"][v])
    both = RU.render_tiles_np(*args(slice(None)), case["width"], case["height"], cfg.tile_size, cfg.ewa_log_clip)
    for v in range(V):
        one = RU.render_tiles_np(*(a[None] if i != 2 else a for i, a in enumerate(args(v))), case["width"],
                                 case["height"], cfg.tile_size, cfg.ewa_log_clip)
        assert np.array_equal(both[v], one[0])
    assert not np.array_equal(both[0], both[1])


@pytest.mark.parametrize("name", RU.EDGE_CASES + RU.CASES)
def test_prepare_restatement_and_host_rows_match_the_recorded_rows(name, capsys):
    """prepare_np (the reference's operations) and gcs_render_prepare_host (the kernel's closed forms) against
    the recorded per-row record, both at rtol 1e-9."""
    case = RU.load_case(name)
    cfg = RU.splat_config(case)
    kw = dict(fbm_modulate_scale=case["fbm_modulate_scale"], fbm_seed=case["fbm_seed"])
    host = R.prepare_splats_host(*_inputs(case), cfg=cfg, **kw)
    rest = RU.prepare_np(*_inputs(case), cfg, **kw)
    valid = case["valid_mask"].astype(bool)
    if name == "hard":
        with capsys.disabled():
            for f, fam in enumerate(case["family_names"]):
                rows = np.flatnonzero((case["family"] == f) & valid)
                print(f"\n  hard/{fam}: {rows.size} rows, worst relative difference host build "
                      f"{_worst(host, case, rows):.1e}, prepare_np {_worst(rest, case, rows):.1e}", end="")
    else:
        rows = np.flatnonzero(valid)
        print(f"{name}: worst relative difference host build {_worst(host, case, rows):.1e}, prepare_np "
              f"{_worst(rest, case, rows):.1e}")
    RU.assert_record(host, case)
    RU.assert_record(rest, case)


def test_prepare_restatement_with_intensity():
    """kappa modulated by intensity (below 0 and above intensity_max included) through prepare_np, against the
    reference's recorded one-lobe shading."""
    ops = RU._npz("render_ops")
    m = ops["vmf_mu"].shape[0]
    scale, imax, kmax = ops["vmf_int_args"]
    cfg = R.SplatRenderingConfig(vmf_intensity_scale=float(scale), vmf_intensity_max=float(imax), vmf_kappa_max=float(kmax))
    view = (np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), np.zeros((1, 2)), ops["vmf_v"][None])
    got = RU.prepare_np(np.zeros((m, 3)), np.broadcast_to(np.eye(3), (m, 3, 3)), ops["vmf_mu"][:, 0], ops["vmf_kappa"][:, 0],
                        np.full((m, 3), 0.5), None, *view, cfg, intensity=ops["vmf1_intensity"])
    np.testing.assert_allclose(got["colors"][0], np.clip(0.5 * ops["vmf1_out"], 0, 1)[:, None] * np.ones(3), rtol=1e-9,
                               atol=0)


def test_edge_fixture_has_the_cases_it_is_for():
    for name, tile, shape in (("tile5", 5, (2, 5, 7)), ("tile1", 1, (1, 5, 7)), ("tile31", 31, (1, 2, 3))):
        case = RU.load_case(name)
        cap = int(case["cfg"]["max_splats_per_tile"])
        assert int(case["cfg"]["tile_size"]) == tile and case["tile_counts"].shape == shape
        assert case["width"] % tile or tile == 1                       # partial tiles (none can be at tile 1)
        assert (case["tile_counts"] == cap).any() and (case["tile_counts"] < cap).any()

    cfg_case = RU.load_case("cfg")
    cfg, dflt = RU.splat_config(cfg_case), R.SplatRenderingConfig()
    for f in ("opacity_gamma", "alpha_min", "eps", "ewa_log_clip", "logdet0", "tile_size"):
        assert getattr(cfg, f) != getattr(dflt, f), f
    valid = cfg_case["valid_mask"].astype(bool)
    assert (cfg_case["radii"][:, valid] == 2.0 / np.sqrt(cfg.eps)).any()          # a radius at the floor
    listed = np.unique(cfg_case["tile_indices"][cfg_case["tile_indices"] >= 0])
    py, px = np.meshgrid(np.arange(cfg_case["height"]) + 0.5, np.arange(cfg_case["width"]) + 0.5, indexing="ij")
    d = np.stack([px, py], -1)[None] - cfg_case["means"][0, listed][:, None, None, :]
    q = np.einsum("nhwi,nij,nhwj->nhw", d, cfg_case["Sigmas_inv"][0, listed], d)
    assert np.mean(0.5 * q > cfg.ewa_log_clip) > 0.5                              # the clip is active on most pixels
    assert cfg_case["alphas"][valid].min() >= cfg.alpha_min and cfg_case["alphas"][valid].min() < cfg.alpha_min + 0.01

    hard = RU.load_case("hard")
    hcfg = RU.splat_config(hard)
    valid = hard["valid_mask"].astype(bool)
    rows = lambda fam: np.flatnonzero((hard["family"] == hard["family_names"].index(fam)) & valid)   # noqa: E731
    for fam in hard["family_names"]:
        assert rows(fam).size, fam
    cond = np.linalg.cond(hard["Sigmas_inv"][:, valid])
    assert cond.max() <= 1e6
    needle = np.linalg.cond(hard["Sigmas_inv"][:, rows("needle")])
    assert needle.min() >= 1e5 and needle.max() <= 1e6
    s3 = np.sqrt(np.linalg.eigvalsh(hard["covariances"][rows("thin")])[:, 0])
    assert np.all((s3 > 0.4e-6) & (s3 < 2.5e-6))
    assert np.all(hard["alphas"][rows("huge")] == hcfg.alpha_min)
    assert np.all(hard["radii"][:, rows("huge")] == 2.0 / np.sqrt(hcfg.eps))
    assert np.all(hard["alphas"][rows("tiny")] == 1.0)
    py, px = np.meshgrid(np.arange(hard["height"]) + 0.5, np.arange(hard["width"]) + 0.5, indexing="ij")
    for v in range(hard["n_views"]):
        d = np.stack([px, py], -1)[None] - hard["means"][v, rows("tiny")][:, None, None, :]
        q = np.einsum("nhwi,nij,nhwj->nhw", d, hard["Sigmas_inv"][v, rows("tiny")], d)
        assert np.all(0.5 * q > hcfg.ewa_log_clip)                                # clipped at every pixel
    assert not hard["kappas"][rows("kappa0")].any() and hard["shaded"][:, rows("kappa0")].any()
    assert np.all(hard["kappas"][rows("kappa1e4")] == 1e4) and not hard["shaded"][:, rows("kappa1e4")].any()
    dn = hard["directions"][rows("antiparallel")]
    assert np.all(((dn / np.linalg.norm(dn, axis=1, keepdims=True)) @ hard["view_dirs"].T).min(1) < -1.0 + 1e-12)
    assert not hard["directions"][rows("zero_dir")].any()
    col = hard["colors"][rows("colour_range")]
    assert (col < 0).any() and (col > 1).any()
    ua = hard["covariances"][rows("ulp_asym")]
    assert np.all(ua[:, 0, 1] != ua[:, 1, 0]) and np.all(np.abs(ua[:, 0, 1] - ua[:, 1, 0]) <= np.spacing(np.abs(ua[:, 1, 0])))
    for fam in ("thin", "needle", "tiny", "huge"):
        assert np.isin(rows(fam), hard["tile_indices"]).any(), fam

    lat = RU.load_case("lattice")
    cap = int(lat["cfg"]["max_splats_per_tile"])
    assert lat["tiles"] is None and lat["phi_center_deg"] == 0.0 and lat["means"].shape == (1, 300, 2)
    assert np.array_equal(lat["means"] * 4.0, np.round(lat["means"] * 4.0))       # on the 0.25 lattice, exactly
    assert np.all(lat["radii"] > 64.0)
    for tx in range(2):
        d2 = RU.sorted_keys(lat["means"][0], (16.0 + 32.0 * tx, 16.0))
        assert d2[cap - 1] == d2[cap]                                             # the cap falls inside a tie group
        listed = lat["tile_indices"][0, 0, tx]
        tied = listed[((lat["means"][0, listed] - (16.0 + 32.0 * tx, 16.0)) ** 2).sum(1) == d2[cap]]
        assert np.all(np.diff(tied) > 0)                                          # ties fall to the row
    assert not np.all(np.diff(lat["tile_indices"][0, 0, 0]) > 0) or not np.all(np.diff(lat["tile_indices"][0, 0, 1]) > 0)


def test_shape_scene_builders():
    """The builders of test_gpu_render_shapes.py give what they say: the lattice ties at every cap the GPU test
    uses, and the per-chunk occupancies."""
    rng = np.random.default_rng(41)
    means, radii = RU.lattice_scene(rng, 4097)
    for cap in (1, 2, 63, 64, 65, 1023, 1024):
        assert RU.tiles_tied_at_cap(means[0], 70, 40, 32, cap), cap
    _, group = np.unique(RU.sorted_keys(means[0], (16.0, 16.0)), return_counts=True)
    assert (group >= 4).sum() > 300                                               # hundreds of groups of exact ties
    assert RU.overlap_mask_np(means, radii, 70, 40, 32).all()
    means, radii = RU.occupancy_scene(rng, 4097, (1,), keep=(1500,))
    per_chunk = [int(c.sum()) for c in np.array_split(RU.overlap_mask_np(means, radii, 70, 40, 32)[0, 0, 0], [1024, 2048, 3072, 4096])]
    assert per_chunk == [1024, 1, 1024, 1024, 1]
    idx, cnt = RU.hand_lists(rng, 1, 2, 5, 129, 1100)
    assert cnt.ravel().tolist() == [0, 1, 63, 64, 65, 127, 128, 129, 129, 0]
    assert all(np.unique(idx[t][:cnt[t]]).size == cnt[t] for t in np.ndindex(1, 2, 5))


def test_thin_rows_log_det_mid_sigmoid():
    """The hard fixture records its thin rows (sigma_3 about 1e-6) with logdet0 = -16, where their alpha
    saturates to 1: at logdet0 = -37, mid-sigmoid, no f64 route meets the per-row bar, the reference's included.
    cond(Sigma) of these rows is 2e9 to 1e11, a backward-stable factorisation of a 3 x 3 moves the smallest
    eigenvalue by up to about 12 * cond * 2^-53 relative (Higham, Accuracy and Stability, Thm 10.3 with
    gamma_4 and |R^T||R| <= 3 |A| in norm), so log det is defined to that and alpha, whose slope in log det
    is at most gamma (1 - alpha_min) / 4, to a quarter of it.  Measured against the determinant in exact
    rational arithmetic: LDL^T (the host build) 1.3e-6, slogdet (prepare_np) 1.9e-6 in log det, the bound
    3e-6 to 2e-4 per row.  So here the LDL^T pivots are held to the exact value at the bound the format
    allows; a wrong pivot or a cofactor expansion's cancellation would miss it by orders of magnitude."""
    import dataclasses
    from fractions import Fraction
    case = RU.load_case("hard")
    cfg = dataclasses.replace(RU.splat_config(case), logdet0=-37.0)
    rows = np.flatnonzero((case["family"] == case["family_names"].index("thin")) & case["valid_mask"])
    host = R.prepare_splats_host(*_inputs(case), cfg=cfg)["alphas"][rows]
    rest = RU.prepare_np(*_inputs(case), cfg)["alphas"][rows]
    exact = np.zeros(rows.size)
    for j, i in enumerate(rows):
        a = [[Fraction(float(x)) for x in r] for r in case["covariances"][i]]
        det = (a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0]) +
               a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]))
        exact[j] = np.log(float(det))
    want = cfg.alpha_min + (1.0 - cfg.alpha_min) / (1.0 + np.exp(-cfg.opacity_gamma * (cfg.logdet0 - exact)))
    assert want.min() < 0.3 and want.max() > 0.6                          # mid-sigmoid
    bound = 0.25 * cfg.opacity_gamma * (1.0 - cfg.alpha_min) * 12.0 * np.linalg.cond(case["covariances"][rows]) * 2.0 ** -53
    print(f"thin rows at logdet0 -37: alpha {want.min():.3f} .. {want.max():.3f}, worst |alpha - exact| host build "
          f"{np.abs(host - want).max():.1e}, prepare_np {np.abs(rest - want).max():.1e}, bound {bound.min():.1e} .. {bound.max():.1e}")
    assert np.all(np.abs(host - want) <= bound) and np.all(np.abs(rest - want) <= bound)
