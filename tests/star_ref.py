"""numpy restatement of the star finder and the star matcher:
the contract the GPU finder matches bit for bit and the C++ matcher matches
pair for pair.  Sums are sequential (python floats are IEEE doubles; numpy
float32 element-wise products and sums are single operations: no FMA, no
pairwise summation)."""
import itertools
import math

import numpy as np

DEFAULTS = dict(ksigma=1.0, radius=10, smooth_sigma=1.0, roundness_min=0.5, min_amp=5.0, cut=0.1, min_fwhm=1.0,
                sat=math.inf, max_stars=2000)
STAR_DTYPE = np.dtype([("x", "f8"), ("y", "f8"), ("flux", "f8"), ("amp", "f8"), ("fwhm_major", "f8"),
                       ("fwhm_minor", "f8"), ("roundness", "f8"), ("px", "i4"), ("py", "i4"), ("npix", "i4"),
                       ("ext", "i4", 4), ("reject", "i4")])
FWHM_K = 2.3548200450309493
SHIFT, SIMILARITY, AFFINE, HOMOGRAPHY = range(4)
MATCH_DEFAULTS = dict(nbright=20, tri_tol=0.002, match_radius=2.0, min_pairs=10, model=HOMOGRAPHY)


def smooth_table(sigma: float) -> np.ndarray:
    K = int(math.ceil(3.0 * sigma))
    if K == 0:
        return np.ones(1, np.float32)
    t = [math.exp(-float(k * k) / (2.0 * sigma * sigma)) for k in range(-K, K + 1)]
    s = 0.0
    for v in t:
        s += v
    return np.array([v / s for v in t], np.float64).astype(np.float32)


def smooth(frame: np.ndarray, tab: np.ndarray) -> np.ndarray:
    """Smoothed plane, float32, NaN where a tap would leave the frame (those
    values are undefined and never read)."""
    p = frame.astype(np.float32)
    h_, w_ = p.shape
    K = len(tab) // 2
    out = np.full((h_, w_), np.nan, np.float32)
    if w_ <= 2 * K or h_ <= 2 * K:
        return out
    wv = w_ - 2 * K
    h = tab[0] * p[:, 0:wv]
    for j in range(1, 2 * K + 1):
        h = h + tab[j] * p[:, j:j + wv]
    hv = h_ - 2 * K
    s = tab[0] * h[0:hv]
    for j in range(1, 2 * K + 1):
        s = s + tab[j] * h[j:j + hv]
    out[K:K + hv, K:K + wv] = s
    return out


def candidates(frame, bg, noise, ksigma=1.0, radius=10, smooth_sigma=1.0, **_):
    """[(x, y, (e0, e1, e2, e3))] in raster order."""
    r = radius
    tab = smooth_table(smooth_sigma)
    K = len(tab) // 2
    P = r + K
    h_, w_ = frame.shape
    thr = np.float32(bg + ksigma * noise)
    if w_ <= 2 * P or h_ <= 2 * P:
        return []
    with np.errstate(invalid="ignore"):
        s = smooth(frame, tab)
        above = s > thr
    out = []
    earlier = np.zeros((2 * r + 1, 2 * r + 1), bool)
    earlier[:r] = True
    earlier[r, :r] = True
    for y in range(P, h_ - P):
        for x in np.nonzero(above[y, P:w_ - P])[0] + P:
            x = int(x)
            v = s[y, x]
            win = s[y - r:y + r + 1, x - r:x + r + 1]
            with np.errstate(invalid="ignore"):
                if (win > v).any() or ((win == v) & earlier).any():
                    continue
            ext = []
            for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1)):
                k = 0
                while k < r:
                    cur = s[y + k * dy, x + k * dx]
                    nxt = s[y + (k + 1) * dy, x + (k + 1) * dx]
                    if nxt < cur and nxt > thr:
                        k += 1
                    else:
                        break
                ext.append(min(r, k + 1))
            out.append((x, y, tuple(ext)))
    return out


def measure(frame, x, y, ext, bg, noise, radius=10, roundness_min=0.5, min_amp=5.0, cut=0.1, min_fwhm=1.0,
            sat=math.inf, **_):
    """One record (STAR_DTYPE scalar as a dict) with its reject code."""
    p = frame.astype(np.float32)
    st = dict(x=0.0, y=0.0, flux=0.0, amp=0.0, fwhm_major=0.0, fwhm_minor=0.0, roundness=0.0, px=x, py=y, npix=0,
              ext=ext, reject=0)
    B = float(bg)
    peak = float(p[y, x])
    A = peak - B
    st["amp"] = A
    if not (A >= min_amp * float(noise)):
        st["reject"] = 1
        return st
    if peak >= sat:
        st["reject"] = 2
        return st
    lim = cut * A
    S0 = Sx = Sy = Sxx = Syy = Sxy = 0.0
    npix = 0
    for dy in range(-ext[2], ext[3] + 1):
        r0 = rx = ry = rxx = ryy = rxy = 0.0
        for dx in range(-ext[0], ext[1] + 1):
            v = float(p[y + dy, x + dx]) - B
            if v > lim:
                vx = v * float(dx)
                vy = v * float(dy)
                r0 += v
                rx += vx
                ry += vy
                rxx += vx * float(dx)
                ryy += vy * float(dy)
                rxy += vx * float(dy)
                npix += 1
        S0 += r0
        Sx += rx
        Sy += ry
        Sxx += rxx
        Syy += ryy
        Sxy += rxy
    st["flux"] = S0
    st["npix"] = npix
    if not (S0 > 0.0):
        st["reject"] = 3
        return st
    mx = Sx / S0
    my = Sy / S0
    a = Sxx / S0 - mx * mx
    c = Syy / S0 - my * my
    b = Sxy / S0 - mx * my
    hd = (a - c) / 2.0
    q = math.sqrt(hd * hd + b * b)
    l1 = (a + c) / 2.0 + q
    l2 = (a + c) / 2.0 - q
    st["x"] = float(x) + mx
    st["y"] = float(y) + my
    if not (l2 > 0.0):
        st["reject"] = 3
        return st
    st["fwhm_major"] = FWHM_K * math.sqrt(l1)
    st["fwhm_minor"] = FWHM_K * math.sqrt(l2)
    st["roundness"] = math.sqrt(l2 / l1)
    if not (st["fwhm_minor"] >= min_fwhm):
        st["reject"] = 4
    elif not (st["fwhm_major"] <= float(2 * radius + 1)):
        st["reject"] = 5
    elif not (st["roundness"] >= roundness_min):
        st["reject"] = 6
    return st


def _records(dicts):
    out = np.zeros(len(dicts), STAR_DTYPE)
    for i, d in enumerate(dicts):
        for k, v in d.items():
            out[i][k] = v
    return out


def find_stars(frame, bg, noise, **params):
    """(stars, every measured candidate in raster order), STAR_DTYPE arrays;
    stars sorted by flux descending, ties (row, column), cut at max_stars."""
    prm = dict(DEFAULTS, **params)
    cand = [measure(frame, x, y, e, bg, noise, **prm) for x, y, e in candidates(frame, bg, noise, **prm)]
    acc = [d for d in cand if d["reject"] == 0]
    acc.sort(key=lambda d: (-d["flux"], d["py"], d["px"]))
    return _records(acc[:prm["max_stars"]]), _records(cand)


# ------------------------------------------------------------------ matcher
def triangles(xy, n):
    out = []
    for tri in itertools.combinations(range(n), 3):
        ln = []
        for s in range(3):
            p, q = tri[(s + 1) % 3], tri[(s + 2) % 3]
            dx = xy[p][0] - xy[q][0]
            dy = xy[p][1] - xy[q][1]
            ln.append(math.sqrt(dx * dx + dy * dy))
        o = sorted(range(3), key=lambda s: -ln[s])        # stable: ties by the opposite vertex's index
        a, b, c = ln[o[0]], ln[o[1]], ln[o[2]]
        if not (a > 0.0):
            continue
        ba, ca = b / a, c / a
        if ca < 0.1 or ba > 0.95:
            continue
        v = [tri[s] for s in o]
        ax, ay = xy[v[0]]
        cr = (xy[v[1]][0] - ax) * (xy[v[2]][1] - ay) - (xy[v[1]][1] - ay) * (xy[v[2]][0] - ax)
        out.append((v, ba, ca, 1 if cr > 0.0 else (-1 if cr < 0.0 else 0)))
    return out


def _hartley(p):
    c = p.mean(0)
    d = np.sqrt(((p - c) ** 2).sum(1)).mean()
    s = math.sqrt(2.0) / d if d > 0 else 1.0
    return np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1.0]])


def _model_for(model, n):
    return min(model, HOMOGRAPHY if n >= 4 else AFFINE if n == 3 else SIMILARITY if n == 2 else SHIFT)


def normalised_system(model, src, dst):
    """(A, rhs, Ts, Td) of the Hartley-normalised least-squares system."""
    Ts, Td = _hartley(src), _hartley(dst)
    s = src * Ts[0, 0] + Ts[:2, 2]
    d = dst * Td[0, 0] + Td[:2, 2]
    m = len(src)
    n = {SIMILARITY: 4, AFFINE: 6, HOMOGRAPHY: 8}[model]
    A = np.zeros((2 * m, n))
    x, y, u, v = s[:, 0], s[:, 1], d[:, 0], d[:, 1]
    if model == SIMILARITY:
        A[0::2, 0], A[0::2, 1], A[0::2, 2] = x, -y, 1
        A[1::2, 0], A[1::2, 1], A[1::2, 3] = y, x, 1
    else:
        A[0::2, 0], A[0::2, 1], A[0::2, 2] = x, y, 1
        A[1::2, 3], A[1::2, 4], A[1::2, 5] = x, y, 1
        if model == HOMOGRAPHY:
            A[0::2, 6], A[0::2, 7] = -u * x, -u * y
            A[1::2, 6], A[1::2, 7] = -v * x, -v * y
    rhs = np.empty(2 * m)
    rhs[0::2], rhs[1::2] = u, v
    return A, rhs, Ts, Td


def fit(model, src, dst):
    """H mapping src to dst (numpy lstsq on the normalised system), h22 = 1."""
    src, dst = np.asarray(src, float), np.asarray(dst, float)
    model = _model_for(model, len(src))
    if model == SHIFT:
        t = (dst - src).mean(0)
        return np.array([[1, 0, t[0]], [0, 1, t[1]], [0, 0, 1.0]])
    A, rhs, Ts, Td = normalised_system(model, src, dst)
    h = np.linalg.lstsq(A, rhs, rcond=None)[0]
    if model == SIMILARITY:
        Hn = np.array([[h[0], -h[1], h[2]], [h[1], h[0], h[3]], [0, 0, 1.0]])
    else:
        Hn = np.append(np.append(h, np.zeros(8 - len(h))), 1.0).reshape(3, 3)
    H = np.linalg.inv(Td) @ Hn @ Ts
    return H / H[2, 2]


def apply_H(H, xy):
    xy = np.asarray(xy, float)
    w = H[2, 0] * xy[:, 0] + H[2, 1] * xy[:, 1] + H[2, 2]
    return np.stack([(H[0, 0] * xy[:, 0] + H[0, 1] * xy[:, 1] + H[0, 2]) / w,
                     (H[1, 0] * xy[:, 0] + H[1, 1] * xy[:, 1] + H[1, 2]) / w], 1)


def match_stars(ref_xy, img_xy, **params):
    """(registered, H, pairs [(img, ref)]); H zeros when not registered."""
    prm = dict(MATCH_DEFAULTS, **params)
    ref_xy, img_xy = np.asarray(ref_xy, float).reshape(-1, 2), np.asarray(img_xy, float).reshape(-1, 2)
    Z = np.zeros((3, 3))
    nr, ni = min(len(ref_xy), prm["nbright"]), min(len(img_xy), prm["nbright"])
    tr, ti = triangles(ref_xy.tolist(), nr), triangles(img_xy.tolist(), ni)
    votes = np.zeros((ni, nr), np.int64)
    if tr and ti:
        rb = np.array([[t[1], t[2], t[3]] for t in tr])
        rv = np.array([t[0] for t in tr])
        for v, ba, ca, sg in ti:
            ok = (rb[:, 2] == sg) & (np.abs(ba - rb[:, 0]) <= prm["tri_tol"]) & (np.abs(ca - rb[:, 1]) <= prm["tri_tol"])
            for s in range(3):
                np.add.at(votes[v[s]], rv[ok, s], 1)
    cand = sorted(((-votes[i, j], i, j) for i in range(ni) for j in range(nr) if votes[i, j] > 0))
    pairs, ui, uj = [], set(), set()
    for nv, i, j in cand:
        if 2 * -nv < -cand[0][0]:
            break
        if i in ui or j in uj:
            continue
        ui.add(i)
        uj.add(j)
        pairs.append((i, j))
    if len(pairs) < 3:
        return False, Z, []
    pairs.sort()
    rad2 = prm["match_radius"] ** 2
    for model in (SIMILARITY, AFFINE, prm["model"]):
        H = fit(model, img_xy[[i for i, _ in pairs]], ref_xy[[j for _, j in pairs]])
        m = apply_H(H, img_xy)
        d2 = ((m[:, None, :] - ref_xy[None, :, :]) ** 2).sum(2)
        bj = d2.argmin(1)
        bi = d2.argmin(0)
        pairs = [(i, int(bj[i])) for i in range(len(img_xy)) if d2[i, bj[i]] <= rad2 and bi[bj[i]] == i]
        if not pairs:
            return False, Z, []
    if len(pairs) < prm["min_pairs"]:
        return False, Z, pairs
    H = fit(prm["model"], img_xy[[i for i, _ in pairs]], ref_xy[[j for _, j in pairs]])
    return True, H, pairs
