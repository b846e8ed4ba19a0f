"""Test helper: the reference's visual feature node after ORB, restated in numpy / plain Python from
fl_ws/src/fl_slam_poc/src/visual_feature_node.cpp (cited as :line) and _feature_batch_to_list
(FS/backend/backend_node.py:1589-1650), sequentially, one keypoint at a time.  A restatement, not a
recording: the node cannot be built where these tests run (no OpenCV, Eigen or rclcpp).  No file I/O: the
fixtures are built here from seeds.

What is declared where the node leaves it open: with more keypoints than max_features the
max_features largest responses are kept (ties to the lower index, NaN last), in input order; a non-finite
u / v or one beyond 1e9 is outside the image; a NaN response weighs 0.

check(got, case) holds the library's rows (host entry or device) against this restatement:
  * exact: count, kp_index, z_valid, n_depth, n_fit, has_mu, has_color, u, v, color, z_m, the zero rows
    beyond count and the invalid-depth rows;
  * rtol 1e-12 (absolute floor 1e-15 x the field's largest magnitude): what does not depend on the solve;
  * the solve by its backward error: |M beta - A^T b|_2 <= 256 * 2^-52 * (|M|_F |beta|_2 + |A^T b|_2);
  * everything after the solve from the library's own beta, at rtol 1e-12; K with an added absolute error
    of 4 * 2^-52 * (|H00 H11| + H01^2) / (1 + |grad z|^2)^2 where det H cancels, kappa_app within the spread
    of its formula over K +- that error.
"""

import math

import numpy as np

NODE_DEFAULTS = dict(   # :70-101
    max_features=512, depth_sample_mode="median3", pixel_sigma=1.0, depth_model="linear", depth_sigma0=0.01,
    depth_sigma_slope=0.01, min_depth_m=0.05, max_depth_m=80.0, depth_validity_slope=5.0, response_soft_scale=50.0,
    depth_scale=1.0, cov_reg_eps=1e-9, invalid_cov_inflate=1e6, hex_radius=2, quad_fit_radius=2,
    quad_fit_min_points=6, quad_fit_lstsq_eps=1e-8, student_t_nu=3.0, student_t_w_min=0.1, ma_tau=10.0,
    ma_delta_inflate=1e-4, kappa0=1.0, kappa_alpha=10.0, kappa_max=100.0, kappa_min=0.1)
K_EPS = 1e-12   # :34
W, H = 24, 16
INTRINSICS = (20.0, 21.0, 11.5, 7.75)   # fx, fy, cx, cy
NAN, INF = float("nan"), float("inf")
U = 2.0 ** -52


def cround(x):
    """static_cast<int>(std::round(x)): half away from zero (the fractional part x - trunc(x) is exact)."""
    t = math.trunc(x)
    f = x - t
    return t + (1 if f >= 0.5 else 0) - (1 if f <= -0.5 else 0)


def clamp(v, lo, hi):
    """:46-49 with std::min / std::max as the standard defines them (a NaN v gives hi)."""
    m = v if v < hi else hi
    return m if lo < m else lo


def cexp(x):
    """std::exp: overflows to inf."""
    try:
        return math.exp(x)
    except OverflowError:
        return INF


def safe_sigmoid(x):   # :37-44
    if x >= 0.0:
        return 1.0 / (1.0 + math.exp(-x))
    ex = math.exp(x)
    return ex / (1.0 + ex)


def _ok(z):
    return math.isfinite(z) and z > 0.0


class Ref:
    """One frame under one config: the node's member functions."""

    def __init__(self, depth, rgb, cfg, intrinsics):
        self.d, self.rgb, self.c = depth, rgb, dict(NODE_DEFAULTS, **cfg)
        self.fx, self.fy, self.cx, self.cy = intrinsics
        self.H, self.W = depth.shape

    def z_at(self, yy, xx):   # depth_to_meters(depth.at(yy, xx)), :179-182
        return float(self.d[yy, xx]) * self.c["depth_scale"]

    def depth_sigma(self, z_m):   # :216-226
        z = abs(z_m)
        return self.c["depth_sigma0"] + self.c["depth_sigma_slope"] * (z * z if self.c["depth_model"] == "quadratic" else z)

    def depth_sample(self, u, v):
        """:228-348 -> (valid, z_m, z_var, zs, n_depth).  Declared: u, v not finite or beyond 1e9 are outside."""
        out = (False, NAN, NAN, [], 0)
        if not (math.isfinite(u) and math.isfinite(v)) or abs(u) > 1e9 or abs(v) > 1e9:
            return out
        x, y = cround(u), cround(v)
        if x < 0 or y < 0 or x >= self.W or y >= self.H:   # :236
            return out
        mode = self.c["depth_sample_mode"]
        if mode == "nearest":   # :240-244: no variance, no zs
            z = self.z_at(y, x)
            return (True, z, NAN, [], 1) if _ok(z) else out
        if mode == "hex":   # :299-348
            r = max(1, self.c["hex_radius"])
            offs = [(0, 0)] + [(cround(r * math.cos(k * math.pi / 3.0)), cround(r * math.sin(k * math.pi / 3.0)))
                               for k in range(6)]
            zs = []
            for dx, dy in offs:
                xi, yi = x + dx, y + dy
                if 0 <= xi < self.W and 0 <= yi < self.H and _ok(self.z_at(yi, xi)):
                    zs.append(self.z_at(yi, xi))
            if len(zs) < 4:   # :327
                return (False, NAN, NAN, [], len(zs))
            z_hat = sorted(zs)[len(zs) // 2]
            mad = sorted(abs(z - z_hat) for z in zs)[len(zs) // 2]
            s = 1.4826 * mad
            return True, z_hat, s * s, zs, len(zs)
        r = {"median3": 1, "median5": 2}[mode]   # :250-257
        zs = []
        for yy in range(max(0, y - r), min(self.H - 1, y + r) + 1):
            for xx in range(max(0, x - r), min(self.W - 1, x + r) + 1):
                if _ok(self.z_at(yy, xx)):
                    zs.append(self.z_at(yy, xx))
        if not zs:
            return out
        z_med = sorted(zs)[len(zs) // 2]   # :279-280: the upper median
        z_var = NAN
        if len(zs) >= 4:   # :282-292
            mean = 0.0
            for z in zs:
                mean += z
            mean /= float(len(zs))
            var = 0.0
            for z in zs:
                var += (z - mean) * (z - mean)
            z_var = var / float(len(zs))
        return True, z_med, z_var, zs, len(zs)

    def student_t(self, z_hat, sigma_z2, zs):   # :350-369
        if len(zs) < 2 or not math.isfinite(sigma_z2) or sigma_z2 <= 0.0:
            return sigma_z2
        sigma2 = max(sigma_z2, K_EPS)
        q = 0.0
        for zi in zs:
            q += (zi - z_hat) * (zi - z_hat)
        q /= float(len(zs)) * sigma2 + K_EPS
        w = (self.c["student_t_nu"] + 1.0) / (self.c["student_t_nu"] + q)
        return sigma_z2 / max(w, self.c["student_t_w_min"])

    def fit_system(self, u, v):
        """:403-444 -> (n_pts, M = A^T A + eps I, A^T b) -- M, A^T b None below quad_fit_min_points."""
        x0, y0, r = cround(u), cround(v), max(1, self.c["quad_fit_radius"])
        rows, b = [], []
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                xi, yi = x0 + dx, y0 + dy
                if 0 <= xi < self.W and 0 <= yi < self.H and _ok(self.z_at(yi, xi)):
                    ut, vt = float(xi) - u, float(yi) - v
                    rows.append([ut * ut, ut * vt, vt * vt, ut, vt, 1.0])
                    b.append(self.z_at(yi, xi))
        if len(rows) < self.c["quad_fit_min_points"]:
            return len(rows), None, None
        A, b = np.array(rows), np.array(b)
        return len(rows), A.T @ A + self.c["quad_fit_lstsq_eps"] * np.eye(6), A.T @ b

    def post_solve(self, beta, z_hat, var_z_eff):
        """:447-490 and :582-600 on a given beta (numpy scalars: IEEE f64, one rounding per operation)."""
        f = np.float64
        a, b_, c, d, e = (f(x) for x in beta[:5])
        z = f(max(z_hat, 1e-6))
        sx, sy = f(self.fx) / z, f(self.fy) / z
        zu, zv = sx * d, sy * e
        h00, h01, h11 = sx * sx * (f(2.0) * a), sx * sy * b_, sy * sy * (f(2.0) * c)
        det = h00 * h11 - h01 * h01
        denom = f(1.0) + (zu * zu + zv * zv)
        K = det / (denom * denom) if denom > 0.0 else f(0.0)
        K_err = 4.0 * U * (abs(h00 * h11) + h01 * h01) / (denom * denom)
        hd = f(0.5) * (h00 - h11)
        lam_min = f(0.5) * (h00 + h11) - np.sqrt(hd * hd + h01 * h01)   # smallest eigenvalue, closed form
        w_ma = safe_sigmoid(float(self.c["ma_tau"] * lam_min))
        n = np.array([-zu, -zv, 1.0])
        nn = np.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2])
        n = n / nn if nn > 0.0 else n
        mu = n / (np.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]) + 1e-12)   # backend_node.py:1616-1620
        rel = math.sqrt(var_z_eff) / (z_hat + K_EPS) if math.isfinite(var_z_eff) else 1.0
        rho = 1.0 / (rel + K_EPS)

        def kappa(Kv):
            k = self.c["kappa0"] + self.c["kappa_alpha"] * math.sqrt(abs(Kv)) * rho
            return clamp(k, self.c["kappa_min"], self.c["kappa_max"]) * w_ma

        Ks = [float(K) - float(K_err), float(K), float(K) + float(K_err)]
        ks = [kappa(x) for x in Ks] + ([kappa(0.0)] if Ks[0] < 0.0 < Ks[2] else [])
        return dict(K=float(K), K_err=float(K_err), lam_min=float(lam_min), w_ma=w_ma, mu_app=mu, kappa_app=kappa(float(K)),
                    kappa_lo=min(ks), kappa_hi=max(ks))

    def keypoint(self, u, v, response):
        """on_rgbd's loop body (:548-634) up to the solve."""
        c = self.c
        valid, z_m, z_var, zs, n_depth = self.depth_sample(u, v)
        z_valid = valid and math.isfinite(z_m) and z_m > 0.0
        w_depth = 0.0
        if z_valid:   # :196-205
            a = c["depth_validity_slope"]
            w_depth = clamp(1.0 / (1.0 + cexp(-a * (z_m - c["min_depth_m"]))) *
                            (1.0 / (1.0 + cexp(+a * (z_m - c["max_depth_m"])))), 0.0, 1.0)
        w_resp = response / (response + c["response_soft_scale"]) if response > 0.0 else 0.0   # :207-214; NaN: 0
        weight = clamp(w_depth * w_resp, 0.0, 1.0)
        n_fit, M, Atb = self.fit_system(u, v) if z_valid else (0, None, None)
        var_z_eff = NAN   # :563-572
        if z_valid and math.isfinite(z_var):
            var_z_eff = self.student_t(z_m, max(z_var, self.depth_sigma(z_m) * self.depth_sigma(z_m)), zs)
        elif z_valid:
            var_z_eff = self.depth_sigma(z_m) * self.depth_sigma(z_m)
        if z_valid and not math.isfinite(var_z_eff):
            var_z_eff = self.depth_sigma(z_m) * self.depth_sigma(z_m)
        xyz, cov = np.zeros(3), np.eye(3) * c["invalid_cov_inflate"]
        if z_valid:   # :371-399, :577-580
            xyz = np.array([(u - self.cx) * z_m / self.fx, (v - self.cy) * z_m / self.fy, z_m])
            vz = max(max(var_z_eff, self.depth_sigma(z_m) * self.depth_sigma(z_m)), 0.0)
            du, dv, vu = u - self.cx, v - self.cy, max(c["pixel_sigma"] * c["pixel_sigma"], 0.0)
            cxy, cxz, cyz = (du * dv * vz) / (self.fx * self.fy), (du * vz) / self.fx, (dv * vz) / self.fy
            cov = np.array([[(z_m * z_m * vu + du * du * vz + vu * vz) / (self.fx * self.fx), cxy, cxz],
                            [cxy, (z_m * z_m * vu + dv * dv * vz + vu * vz) / (self.fy * self.fy), cyz],
                            [cxz, cyz, vz]])
        lam_c = th_c = 0.0   # :602-609
        if z_valid and math.isfinite(var_z_eff) and var_z_eff > 0.0:
            lam_c = 1.0 / var_z_eff
            th_c = lam_c * z_m
        color = np.zeros(3)
        if self.rgb is not None:   # :611-616
            ix = cround(clamp(u, 0.0, float(self.W - 1)))
            iy = cround(clamp(v, 0.0, float(self.H - 1)))
            color = self.rgb[iy, ix].astype(np.float64) / 255.0
        return dict(u=u, v=v, z_valid=z_valid, n_depth=n_depth, n_fit=n_fit, z_m=z_m if z_valid else NAN,
                    z_var=z_var if z_valid else NAN, var_z_eff=var_z_eff, xyz=xyz, cov_base=cov, weight=weight,
                    depth_Lambda_c=lam_c, depth_theta_c=th_c, color=color, M=M, Atb=Atb, has_mu=M is not None)


def select(responses, max_features):
    """Declared selection: the max_features largest responses (NaN last), ties to the lower index, input order."""
    n = len(responses)
    if n <= max_features:
        return list(range(n))
    key = [(-(r if r == r else -INF), i) for i, r in enumerate(float(x) for x in responses)]
    return sorted(i for _, i in sorted(key)[:max_features])


_refs = {}


def reference(case):
    """The restatement's rows of a case, computed once per case name."""
    if case["name"] not in _refs:
        r = Ref(case["depth"], case["rgb"], case["cfg"], case["intrinsics"])
        kp = case["keypoints"].astype(np.float32)
        idx = select(kp[:, 2], r.c["max_features"])
        _refs[case["name"]] = (r, idx, [r.keypoint(float(kp[i, 0]), float(kp[i, 1]), float(kp[i, 2])) for i in idx])
    return _refs[case["name"]]


def _close(name, got, want, tag):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    scale = np.abs(want[fin]).max() if fin.any() else 0.0
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-15 * scale, equal_nan=True, err_msg=f"{tag}: {name}")


def _same(name, got, want, tag):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (tag, name, got.shape, want.shape)
    assert np.array_equal(got, want, equal_nan=got.dtype.kind == "f"), \
        f"{tag}: {name} differs at {np.flatnonzero((got != want).reshape(len(got), -1).any(1))[:8]}"


def check(got, diag, count, case, tag=""):
    """got / diag: the library's feature and diagnostic arrays with all max_features rows (numpy); count: its count.
    Returns the measured figures (largest solve residual ratio, number of fitted rows)."""
    tag = f"{tag} {case['name']}"
    r, idx, rows = reference(case)
    m, cap = len(idx), r.c["max_features"]
    assert count == m == min(len(case["keypoints"]), cap), (tag, count, m)
    for name, x in list(got.items()) + list(diag.items()):
        assert x.shape[0] == cap, (tag, name, x.shape)
        if name == "kp_index":
            assert (x[m:] == -1).all(), tag
        else:
            assert not x[m:].any(), f"{tag}: {name} rows beyond count are not zero"
    if m == 0:
        return dict(residual=0.0, n_fit=0)

    def col(k):
        return np.array([row[k] for row in rows])

    _same("kp_index", diag["kp_index"][:m], np.array(idx, np.int32), tag)
    kp = case["keypoints"].astype(np.float32)
    _same("u", got["u"][:m], kp[idx, 0].astype(np.float64), tag)
    _same("v", got["v"][:m], kp[idx, 1].astype(np.float64), tag)
    for k in ("z_valid", "n_depth", "n_fit"):
        _same(k, diag[k][:m], col(k).astype(diag[k].dtype), tag)
    _same("has_mu", got["has_mu"][:m], col("has_mu").astype(np.uint8), tag)
    _same("has_color", got["has_color"][:m], np.full(m, case["rgb"] is not None, np.uint8), tag)
    _same("color", got["color"][:m], col("color"), tag)
    _same("z_m", diag["z_m"][:m], col("z_m"), tag)
    inv = ~col("z_valid")
    if inv.any():   # invalid-depth rows, exactly (:574-575, :554)
        assert not got["xyz"][:m][inv].any() and not got["weight"][:m][inv].any(), tag
        _same("cov (invalid depth)", got["cov"][:m][inv],
              np.tile((np.eye(3) * r.c["invalid_cov_inflate"]).reshape(9), (int(inv.sum()), 1)), tag)
        for k in ("depth_Lambda_c", "depth_theta_c", "kappa_app"):
            assert not got[k][:m][inv].any(), (tag, k)
        assert not got["has_mu"][:m][inv].any() and not got["mu_app"][:m][inv].any(), tag
    for k in ("z_var", "var_z_eff"):
        _close(k, diag[k][:m], col(k), tag)
    for k in ("xyz", "weight", "depth_Lambda_c", "depth_theta_c"):
        _close(k, got[k][:m], col(k), tag)
    fit = col("has_mu")
    _close("cov (no fit)", got["cov"][:m][~fit & ~inv], col("cov_base").reshape(m, 9)[~fit & ~inv], tag)
    for k in ("K", "lam_min", "w_ma"):
        assert np.isnan(diag[k][:m][~fit]).all(), (tag, k)
    assert np.isnan(diag["beta"][:m][~fit]).all() and not got["mu_app"][:m][~fit].any(), tag
    assert not got["kappa_app"][:m][~fit].any(), tag

    worst, post = 0.0, []
    for j in np.flatnonzero(fit):
        row, beta = rows[j], diag["beta"][j]
        assert np.isfinite(beta).all(), (tag, j, beta)
        res = np.linalg.norm(row["M"] @ beta - row["Atb"])
        bound = 256.0 * U * (np.linalg.norm(row["M"]) * np.linalg.norm(beta) + np.linalg.norm(row["Atb"]))
        worst = max(worst, res / bound)
        assert res <= bound, f"{tag}: row {j} solve residual {res:.3e} above {bound:.3e}"
        post.append(r.post_solve(beta, row["z_m"], row["var_z_eff"]))
    if post:
        f = np.flatnonzero(fit)

        def pcol(k):
            return np.array([p[k] for p in post])

        for k in ("lam_min", "w_ma"):
            _close(k, diag[k][f], pcol(k), tag)
        _close("mu_app", got["mu_app"][f], pcol("mu_app"), tag)
        K, Kw, Ke = diag["K"][f], pcol("K"), pcol("K_err")
        bad = np.abs(K - Kw) > 1e-12 * np.abs(Kw) + Ke
        assert not bad.any(), f"{tag}: K rows {f[bad][:8]}: {K[bad][:4]} vs {Kw[bad][:4]} (+- {Ke[bad][:4]})"
        ka, lo, hi = got["kappa_app"][f], pcol("kappa_lo"), pcol("kappa_hi")
        bad = (ka < lo - 1e-12 * np.abs(lo)) | (ka > hi + 1e-12 * np.abs(hi))
        assert not bad.any(), f"{tag}: kappa_app rows {f[bad][:8]}: {ka[bad][:4]} outside [{lo[bad][:4]}, {hi[bad][:4]}]"
        cov = col("cov_base")[f] + ((1.0 - pcol("w_ma")) * r.c["ma_delta_inflate"])[:, None, None] * np.eye(3)   # :582-583
        _close("cov (fit)", got["cov"][f], cov.reshape(-1, 9), tag)
    return dict(residual=worst, n_fit=int(fit.sum()))


# ------------------------------------------------------------------------------------------------ fixtures

def _surface(z0, a=0.0, b=0.0, c=0.0, d=0.0, e=0.0, noise=0.0, seed=0):
    """z = z0 + a x^2 + b x y + c y^2 + d x + e y around the image centre, as float32."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    x, y = x - 11.0, y - 7.0
    z = z0 + a * x * x + b * x * y + c * y * y + d * x + e * y
    return (z + noise * np.random.default_rng(seed).standard_normal(z.shape)).astype(np.float32)


def _rgb(seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


SLOT_X, SLOT_Y = (2, 7, 12, 17, 22), (2, 7, 12)   # centres of disjoint 5 x 5 windows (the last column's is clipped)

# geometry keypoints: sub-pixel interior points, the four corners and edges (clipped windows), halves
# (k + 0.5 rounds up, -0.5 rounds to -1: outside, -0.4 rounds to 0), W - 0.5 (rounds to W: outside) and
# coordinates outside, non-finite or huge
GEOMETRY = [(11.3, 7.6), (5.75, 9.2), (16.1, 4.45), (8.0, 8.0), (0.0, 0.0), (23.0, 0.0), (0.0, 15.0), (23.0, 15.0),
            (12.2, 0.3), (11.7, 15.2), (0.2, 8.4), (23.3, 6.6), (4.5, 6.5), (2.5, 3.5), (-0.5, 5.0), (5.0, -0.5),
            (-0.4, 5.0), (5.0, -0.4), (23.5, 5.0), (W - 0.5, 15.4), (10.0, 15.5), (-3.0, 4.0), (30.0, 4.0),
            (4.0, 40.0), (NAN, 4.0), (4.0, INF), (-INF, NAN), (2e9, 3.0), (3.0, -3e9), (22.5, 14.5), (1.5, 0.5)]
RESPONSES = [120.0, 3.5e-3, 1e4, 0.0, -1.0, 40.0, 75.5, NAN]


def _keypoints(points, seed=0):
    rs = np.random.default_rng(seed).permutation(len(points)) % len(RESPONSES)
    return np.array([(u, v, RESPONSES[k]) for (u, v), k in zip(points, rs)], np.float32)


def _slot_points():
    off = [(0.3, -0.2), (-0.4, 0.1), (0.0, 0.0), (0.45, 0.45), (-0.25, -0.45)]
    return [(x + off[(i + j) % 5][0], y + off[(i + j) % 5][1]) for j, y in enumerate(SLOT_Y) for i, x in enumerate(SLOT_X)]


def _holes_image(seed=3):
    """A tilted, noisy plane with every slot's 5 x 5 window knocked out (NaN, +inf, 0, negative in turn)
    except a per-slot pattern of survivors: (inner 3 x 3 survivors, whole-window survivors) =
    (0, 0), (1, 1), (3, 5), (4, 6), (5, 9), (8 without the centre, 8), (1, 7), (9, 25: untouched), then
    slots with duplicate values (all equal; two pairs) and with an even / odd count."""
    z = _surface(2.0, d=0.01, e=-0.02, noise=0.004, seed=seed).astype(np.float64)
    bad = [NAN, INF, 0.0, -1.5]
    ring = [(-2, -2), (2, -2), (-2, 2), (2, 2), (0, -2), (0, 2), (-2, 0), (2, 0), (1, -2), (-1, 2)]
    inner = [(0, 0), (1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1), (1, -1), (-1, 1)]
    keep = [[], inner[:1], inner[:3] + ring[:2], inner[:4] + ring[:2], inner[:5] + ring[:4], inner[1:], inner[:1] + ring[:6],
            None, "equal", "pairs", inner[:6], inner[:7] + ring[:1], inner[:2] + ring[:8], inner[:4], None]
    slots = [(x, y) for y in SLOT_Y for x in SLOT_X]
    k = 0
    for (sx, sy), pat in zip(slots, keep):
        if pat is None:
            continue
        if pat == "equal":
            z[sy - 2:sy + 3, max(sx - 2, 0):sx + 3] = 1.75
            continue
        if pat == "pairs":
            z[sy - 1:sy + 2, sx - 1:sx + 2] = np.array([[2.0, 2.5, 2.0], [2.25, 2.25, 2.5], [2.0, 2.25, 2.5]])
            continue
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                if (dx, dy) not in pat and 0 <= sx + dx < W:
                    z[sy + dy, sx + dx] = bad[k % 4]
                    k += 1
    return z.astype(np.float32)


def _case(name, depth, points, cfg=None, rgb_seed=None, seed=0, intrinsics=INTRINSICS):
    return dict(name=name, depth=depth, rgb=None if rgb_seed is None else _rgb(rgb_seed), cfg=dict(cfg or {}),
                keypoints=_keypoints(points, seed) if not isinstance(points, np.ndarray) else points,
                intrinsics=intrinsics)


def _random_points(n, seed):
    g = np.random.default_rng(seed)
    return np.stack([g.uniform(-1.0, W, n), g.uniform(-1.0, H, n), g.choice([0.0, 5.0, 5.0, 80.0, 900.0], n) +
                     g.integers(0, 3, n)], 1).astype(np.float32)


def build_cases():
    cases = []
    holes, pts = _holes_image(), _slot_points() + GEOMETRY
    for mode in ("nearest", "median3", "median5", "hex"):   # every sample mode on the knocked-out image
        cases.append(_case(f"holes_{mode}", holes, pts, dict(depth_sample_mode=mode), rgb_seed=1))
    for r in (1, 2, 3):   # hex radii (taps leave the image at the edges) and fit radii
        cases.append(_case(f"holes_hex_r{r}_fit_r{r}", holes, pts,
                           dict(depth_sample_mode="hex", hex_radius=r, quad_fit_radius=r), rgb_seed=None, seed=r))
        cases.append(_case(f"noisy_fit_r{r}", _surface(1.5, a=1e-3, c=2e-3, d=0.01, noise=0.01, seed=r), pts,
                           dict(quad_fit_radius=r, depth_sample_mode="median5"), rgb_seed=r))
    cases.append(_case("radius_below_1", holes, pts, dict(depth_sample_mode="hex", hex_radius=0, quad_fit_radius=-2)))
    shapes = dict(flat=dict(z0=1.25), tilted=dict(z0=2.0, d=0.03, e=-0.02), bowl=dict(z0=1.0, a=0.01, c=0.012, b=0.002),
                  saddle=dict(z0=1.5, a=0.01, c=-0.01), dome=dict(z0=3.0, a=-0.012, c=-0.015),
                  cylinder=dict(z0=1.5, a=0.005))
    for name, kw in shapes.items():   # exact surfaces: kappa_max on the bowl, w_ma -> 0 on the dome
        cases.append(_case(f"shape_{name}", _surface(**kw), pts, rgb_seed=None if name == "flat" else 2))
    cases.append(_case("kappa_min", _surface(1.25), pts, dict(kappa0=0.01, kappa_min=0.1)))
    cases.append(_case("quadratic_model", _surface(2.0, a=0.002, e=0.01, noise=0.02, seed=5), pts,
                       dict(depth_model="quadratic", depth_sigma_slope=0.002, student_t_nu=4.0, student_t_w_min=0.5,
                            pixel_sigma=0.7, ma_tau=3.0, response_soft_scale=10.0)))
    cases.append(_case("outliers_student_t", _outlier_image(), pts, dict(depth_sample_mode="median5")))
    rng_img = np.repeat(np.array([0.04, 0.05, 0.051, 0.06, 0.3, 1.0, 79.0, 79.9, 80.0, 80.4, 85.0, 300.0], np.float32), 2)
    cases.append(_case("depth_range", np.tile(rng_img, (H, 1)), [(x + 0.2, 6.3) for x in range(W)] + GEOMETRY[:8]))
    z16 = _holes_image().astype(np.float64)   # millimetres; what is not a positive finite depth is 0
    z16 = np.round(np.where(np.isfinite(z16) & (z16 > 0), z16, 0.0) * 1000.0).astype(np.uint16)
    cases.append(_case("uint16", z16, pts, dict(depth_scale=0.001), rgb_seed=4))
    col = np.full((H, W), NAN, np.float32)   # six collinear valid pixels: a degenerate fit (radius 3: 7 x 7 window)
    col[8, 5:11] = [1.5, 1.52, 1.49, 1.51, 1.5, 1.53]
    cases.append(_case("collinear_six", col, [(8.3, 8.2), (7.5, 7.6), (11.0, 8.0)], dict(quad_fit_radius=3)))
    surf = _surface(1.5, a=1e-3, c=2e-3, d=0.01, noise=0.01, seed=9)
    for n in (0, 1, 3, 4, 5, 63, 64, 65):   # wave and workgroup edges; 67 rows: the last workgroup is partial
        cases.append(_case(f"count_{n}", surf, _random_points(n, 20 + n), dict(max_features=67), rgb_seed=6))
    # the cut at max_features = 8, with responses tied across it: of 9, two are larger than the seven 5s (the
    # last 5 goes); of 20, six are larger and the 5s at 1 and 3 stay, those at 6, 8, 11, 13, 16 go
    tied = {8: None, 9: [5, 9, 5, 5, 7, 5, 5, 5, 5],
            20: [1, 5, 80, 5, NAN, 900, 5, 0, 5, 81, -1, 5, 82, 5, 2, 83, 5, 3, 84, 4]}
    for n, resp in tied.items():
        kp = _random_points(n, 40 + n)
        if resp is not None:
            kp[:, 2] = resp
        cases.append(_case(f"select_{n}", surf, kp, dict(max_features=8, max_keypoints=32), rgb_seed=7))
    for n in (300, 1100):   # more than one block of the rank count; more than one keypoint per thread of the scan
        cases.append(_case(f"select_{n}", surf, _random_points(n, 40 + n), dict(max_features=8, max_keypoints=2048)))
    return cases


def _outlier_image():
    z = _surface(2.0, d=0.005, noise=0.002, seed=8)
    g = np.random.default_rng(8)
    yy, xx = g.integers(0, H, 40), g.integers(0, W, 40)
    z[yy, xx] += g.choice([-0.8, 0.6, 1.5], 40).astype(np.float32)
    return z


CASES = build_cases()
CASE_NAMES = [c["name"] for c in CASES]
BY_NAME = {c["name"]: c for c in CASES}
