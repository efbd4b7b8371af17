"""numpy float64 restatement of the PSF fit: the contract the
GPU fit (siril_amd/csrc/psf_fit.hip) is compared against.  One star at a time,
Levenberg-Marquardt on the quadratic form (a, b, c) of a Gaussian or a Moffat
profile, Cholesky solves in double.  `reverse` sums the samples in the
opposite order: the difference between the two runs is the rounding floor of
the fit, which the GPU test turns into its tolerance."""
import math

import numpy as np

GAUSSIAN, MOFFAT = 0, 1
PROFILES = {"gaussian": GAUSSIAN, "moffat": MOFFAT}
FWHM_K = 2.3548200450309493
DEFAULTS = dict(radius=10, min_fwhm=1.0, roundness_min=0.5, sat=math.inf, max_iter=50)
PSF_DTYPE = np.dtype([("x", "f8"), ("y", "f8"), ("bkg", "f8"), ("amp", "f8"), ("fwhm_major", "f8"),
                      ("fwhm_minor", "f8"), ("roundness", "f8"), ("angle", "f8"), ("beta", "f8"), ("rmse", "f8"),
                      ("a", "f8"), ("b", "f8"), ("c", "f8"), ("nused", "i4"), ("iterations", "i4"), ("status", "i4"),
                      ("reserved", "i4")])
MU0, MU_MIN, MU_MAX, CONV = 1e-3, 1e-12, 1e10, 1e-12
BETA0, BETA_MIN, BETA_MAX = 2.5, 0.5, 10.0


def moffat_k(beta: float) -> float:
    return 2.0 * math.sqrt(math.pow(2.0, 1.0 / beta) - 1.0)


def half_size(ext, radius: int) -> int:
    return min(int(radius), max(int(e) for e in ext) + 2)


def evaluate(profile, p, beta, dx, dy, val):
    """(model values, residuals, Jacobian [n, len(p)]) at the point p; `beta`
    is used when p has 7 entries (Gaussian: ignored)."""
    B, A, x0, y0, a, b, c = (float(t) for t in p[:7])
    if len(p) == 8:
        beta = float(p[7])
    u = dx - x0
    v = dy - y0
    Q = a * u * u + 2.0 * b * u * v + c * v * v
    with np.errstate(all="ignore"):
        if profile == GAUSSIAN:
            E = np.exp(-Q / 2.0)
            g = -A * E / 2.0
        else:
            E = np.power(1.0 + Q, -beta)
            g = -beta * A * E / (1.0 + Q)
        f = B + A * E
        J = np.empty((len(dx), len(p)))
        J[:, 0] = 1.0
        J[:, 1] = E
        J[:, 2] = g * (-2.0 * a * u - 2.0 * b * v)
        J[:, 3] = g * (-2.0 * b * u - 2.0 * c * v)
        J[:, 4] = g * u * u
        J[:, 5] = 2.0 * g * u * v
        J[:, 6] = g * v * v
        if len(p) == 8:
            J[:, 7] = -A * E * np.log(1.0 + Q)
    return f, val - f, J


def valid(p, beta) -> bool:
    B, A, x0, y0, a, b, c = (float(t) for t in p[:7])
    if len(p) == 8:
        beta = float(p[7])
    return bool(A > 0.0 and a > 0.0 and c > 0.0 and a * c - b * b > 0.0 and BETA_MIN <= beta <= BETA_MAX)


def cholesky_solve(M, rhs):
    """Solution of M x = rhs for a symmetric M by Cholesky, or None at a
    non-positive (or non-finite) pivot."""
    n = len(rhs)
    L = [[0.0] * n for _ in range(n)]
    for j in range(n):
        d = float(M[j][j])
        for k in range(j):
            d -= L[j][k] * L[j][k]
        if not (d > 0.0) or not math.isfinite(d):
            return None
        L[j][j] = math.sqrt(d)
        for i in range(j + 1, n):
            s = float(M[i][j])
            for k in range(j):
                s -= L[i][k] * L[j][k]
            L[i][j] = s / L[j][j]
    y = [0.0] * n
    for i in range(n):
        s = float(rhs[i])
        for k in range(i):
            s -= L[i][k] * y[k]
        y[i] = s / L[i][i]
    x = [0.0] * n
    for i in range(n - 1, -1, -1):
        s = y[i]
        for k in range(i + 1, n):
            s -= L[k][i] * x[k]
        x[i] = s / L[i][i]
    return np.array(x)


def derived(profile, p, beta):
    """(fwhm_major, fwhm_minor, roundness, angle) of the quadratic form."""
    a, b, c = float(p[4]), float(p[5]), float(p[6])
    if len(p) == 8:
        beta = float(p[7])
    k = FWHM_K if profile == GAUSSIAN else moffat_k(beta)
    hd = (a - c) / 2.0
    q = math.sqrt(hd * hd + b * b)
    l1 = (a + c) / 2.0 + q
    l2 = (a + c) / 2.0 - q
    major = k / math.sqrt(l2) if l2 > 0.0 else 0.0
    minor = k / math.sqrt(l1) if l1 > 0.0 else 0.0
    t = 0.5 * math.atan2(2.0 * b, a - c) * (180.0 / math.pi)
    angle = t + 90.0 if t <= 0.0 else t - 90.0
    return major, minor, (minor / major if major > 0.0 else 0.0), angle


def start_point(star, bg, profile, beta):
    """(p, beta): the isotropic start; beta None or <= 0 frees it (Moffat)."""
    free = profile == MOFFAT and (beta is None or beta <= 0.0)
    bt = BETA0 if (beta is None or beta <= 0.0) else float(beta)
    f0 = math.sqrt(float(star["fwhm_major"]) * float(star["fwhm_minor"]))
    k = FWHM_K if profile == GAUSSIAN else moffat_k(bt)
    with np.errstate(all="ignore"):
        lam = (k / f0) ** 2 if f0 > 0.0 else math.nan
    p = [float(bg), float(star["amp"]), float(star["x"]) - int(star["px"]), float(star["y"]) - int(star["py"]),
         lam, 0.0, lam]
    if free:
        p.append(bt)
    return np.array(p), bt


def fit_star(frame, star, bg, profile="gaussian", beta=None, reverse=False, **params):
    """One PSF_DTYPE record (as a dict) for one find_stars record."""
    prm = dict(DEFAULTS, **params)
    prof = PROFILES[profile] if isinstance(profile, str) else int(profile)
    radius = int(prm["radius"])
    b = half_size(star["ext"], radius)
    px, py = int(star["px"]), int(star["py"])
    h_, w_ = frame.shape
    if px - b < 0 or py - b < 0 or px + b >= w_ or py + b >= h_:
        raise ValueError("the box leaves the frame")
    box = np.asarray(frame[py - b:py + b + 1, px - b:px + b + 1], np.float64)
    gy, gx = np.mgrid[-b:b + 1, -b:b + 1]
    p, bt = start_point(star, bg, prof, beta)
    np_ = len(p)
    rec = dict(nused=0, iterations=0, status=3, rmse=0.0, reserved=0)

    def fill(p, status):
        major, minor, rnd, ang = derived(prof, p, bt) if (p[4] > 0 and p[6] > 0) else (0.0, 0.0, 0.0, 0.0)
        rec.update(x=px + p[2], y=py + p[3], bkg=p[0], amp=p[1], fwhm_major=major, fwhm_minor=minor, roundness=rnd,
                   angle=ang, beta=(p[7] if np_ == 8 else (bt if prof == MOFFAT else 0.0)), a=p[4], b=p[5], c=p[6],
                   status=status)
        return rec

    if not np.isfinite(box).all():
        return fill(p, 3)
    use = (box < prm["sat"]).ravel()
    dx = gx.ravel()[use].astype(np.float64)
    dy = gy.ravel()[use].astype(np.float64)
    val = box.ravel()[use]
    if reverse:
        dx, dy, val = dx[::-1].copy(), dy[::-1].copy(), val[::-1].copy()
    n = len(val)
    rec["nused"] = n
    if n < np_ + 1 or not valid(p, bt) or not np.isfinite(p).all():
        return fill(p, 3)
    f, r, J = evaluate(prof, p, bt, dx, dy, val)
    if not np.isfinite(f).all():
        return fill(p, 3)
    chi2 = float((r * r).sum(0))
    mu = MU0
    it = 0
    status = None
    while status is None:
        JtJ = (J[:, :, None] * J[:, None, :]).sum(0)
        Jtr = (J * r[:, None]).sum(0)
        while True:
            M = JtJ + mu * np.diag(np.diag(JtJ))
            d = cholesky_solve(M, Jtr)
            ok = False
            if d is not None:
                pn = p + d
                if np.isfinite(pn).all() and valid(pn, bt):
                    fn, rn, Jn = evaluate(prof, pn, bt, dx, dy, val)
                    if np.isfinite(fn).all():
                        chi2n = float((rn * rn).sum(0))
                        ok = chi2n <= chi2
            if ok:
                mu = max(mu / 10.0, MU_MIN)
                break
            mu = 10.0 * mu
            if mu > MU_MAX:
                status = 2
                break
        if status is not None:
            break
        it += 1
        conv = chi2 - chi2n <= CONV * chi2
        p, r, J, chi2 = pn, rn, Jn, chi2n
        if conv:
            status = 0
        elif it >= prm["max_iter"]:
            status = 1
    rec["iterations"] = it
    rec["rmse"] = math.sqrt(chi2 / (n - np_))
    fill(p, status)
    if status == 0:
        if abs(p[2]) > b / 2.0 or abs(p[3]) > b / 2.0:
            rec["status"] = 4
        elif rec["fwhm_minor"] < prm["min_fwhm"] or rec["fwhm_major"] > 2 * radius + 1:
            rec["status"] = 5
        elif rec["roundness"] < prm["roundness_min"]:
            rec["status"] = 6
    return rec


def fit_stars(frame, stars, bg, profile="gaussian", beta=None, reverse=False, **params):
    """PSF_DTYPE array aligned with the find_stars array `stars` of one frame."""
    out = np.zeros(len(stars), PSF_DTYPE)
    for i, s in enumerate(stars):
        d = fit_star(frame, s, bg, profile, beta, reverse, **params)
        for k, v in d.items():
            out[i][k] = v
    return out
