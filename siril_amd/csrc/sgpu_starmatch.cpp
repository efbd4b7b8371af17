// sgpu_starmatch.cpp -- star-list matching and transform fit for star-based
// global registration: triangle voting on the brightest stars, greedy
// one-to-one initial pairs, three rounds of fit / mutual-nearest-neighbour
// re-pairing (similarity, affine, the requested model), final fit.  Host
// only, deterministic (no random sampling).  Modelled on Siril's matching/;
// the specification is DESIGN.md 6f, restated in tests/star_ref.py.  Parity
// with Siril is unpinned.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "sgpu_internal.h"

using sgpu_host::fail;

namespace {

struct Tri {
    int v[3];          // vertices opposite the sides a >= b >= c
    double ba, ca;
    int sign;
};

struct Pt {
    double x, y;
};

// all triangles of the first n stars
std::vector<Tri> triangles(const double *xy, int n) {
    std::vector<Tri> out;
    for (int i = 0; i < n; i++)
        for (int j = i + 1; j < n; j++)
            for (int k = j + 1; k < n; k++) {
                const int v[3] = {i, j, k};
                // side s is opposite vertex v[s]
                double len[3];
                for (int s = 0; s < 3; s++) {
                    const int p = v[(s + 1) % 3], q = v[(s + 2) % 3];
                    const double dx = xy[2 * p] - xy[2 * q], dy = xy[2 * p + 1] - xy[2 * q + 1];
                    len[s] = std::sqrt(dx * dx + dy * dy);
                }
                // descending length, ties by the opposite vertex's index (v is ascending: stable)
                int o[3] = {0, 1, 2};
                std::stable_sort(o, o + 3, [&](int a, int b) { return len[a] > len[b]; });
                const double a = len[o[0]], b = len[o[1]], c = len[o[2]];
                if (!(a > 0.0)) continue;
                Tri t;
                t.ba = b / a;
                t.ca = c / a;
                if (t.ca < 0.1 || t.ba > 0.95) continue;
                for (int s = 0; s < 3; s++) t.v[s] = v[o[s]];
                const double ax = xy[2 * t.v[0]], ay = xy[2 * t.v[0] + 1];
                const double cr = (xy[2 * t.v[1]] - ax) * (xy[2 * t.v[2] + 1] - ay) -
                                  (xy[2 * t.v[1] + 1] - ay) * (xy[2 * t.v[2]] - ax);
                t.sign = cr > 0.0 ? 1 : (cr < 0.0 ? -1 : 0);
                out.push_back(t);
            }
    return out;
}

// Gaussian elimination with partial pivoting on the n x n system M x = b (M row-major, destroyed)
bool solve(std::vector<double> &M, std::vector<double> &b, int n) {
    for (int c = 0; c < n; c++) {
        int piv = c;
        for (int r = c + 1; r < n; r++)
            if (std::fabs(M[r * n + c]) > std::fabs(M[piv * n + c])) piv = r;
        if (!(std::fabs(M[piv * n + c]) > 0.0)) return false;
        if (piv != c) {
            for (int k = 0; k < n; k++) std::swap(M[c * n + k], M[piv * n + k]);
            std::swap(b[c], b[piv]);
        }
        for (int r = c + 1; r < n; r++) {
            const double f = M[r * n + c] / M[c * n + c];
            for (int k = c; k < n; k++) M[r * n + k] -= f * M[c * n + k];
            b[r] -= f * b[c];
        }
    }
    for (int r = n - 1; r >= 0; r--) {
        double s = b[r];
        for (int k = r + 1; k < n; k++) s -= M[r * n + k] * b[k];
        b[r] = s / M[r * n + r];
    }
    return true;
}

// least squares through the normal equations: rows of A (m x n) and rhs
bool lstsq(const std::vector<double> &A, const std::vector<double> &rhs, int m, int n, std::vector<double> &x) {
    std::vector<double> N((size_t)n * n, 0.0);
    x.assign(n, 0.0);
    for (int r = 0; r < m; r++)
        for (int i = 0; i < n; i++) {
            const double ai = A[(size_t)r * n + i];
            if (ai == 0.0) continue;
            for (int j = 0; j < n; j++) N[i * n + j] += ai * A[(size_t)r * n + j];
            x[i] += ai * rhs[r];
        }
    return solve(N, x, n);
}

// Hartley normalisation: T = [[s, 0, -s cx], [0, s, -s cy], [0, 0, 1]], mean distance sqrt(2)
void hartley(const std::vector<Pt> &p, double &s, double &cx, double &cy) {
    const double n = (double)p.size();
    double sx = 0.0, sy = 0.0;
    for (const Pt &q : p) {
        sx += q.x;
        sy += q.y;
    }
    cx = sx / n;
    cy = sy / n;
    double d = 0.0;
    for (const Pt &q : p) d += std::sqrt((q.x - cx) * (q.x - cx) + (q.y - cy) * (q.y - cy));
    d /= n;
    s = d > 0.0 ? std::sqrt(2.0) / d : 1.0;
}

void mat3(const double *a, const double *b, double *o) {
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) o[3 * r + c] = (a[3 * r] * b[c] + a[3 * r + 1] * b[3 + c]) + a[3 * r + 2] * b[6 + c];
}

int model_for(int model, size_t npairs) {      // the highest model the pair count supports
    const int most = npairs >= 4 ? SGPU_MODEL_HOMOGRAPHY : npairs == 3 ? SGPU_MODEL_AFFINE
                     : npairs == 2 ? SGPU_MODEL_SIMILARITY : SGPU_MODEL_SHIFT;
    return std::min(model, most);
}

// H maps src to dst
bool fit(int model, const std::vector<Pt> &src, const std::vector<Pt> &dst, double *H) {
    const int m = (int)src.size();
    if (m < 1) return false;
    model = model_for(model, (size_t)m);
    if (model == SGPU_MODEL_SHIFT) {           // a shift does not survive two normalisations: plain mean
        double tx = 0.0, ty = 0.0;
        for (int i = 0; i < m; i++) {
            tx += dst[i].x - src[i].x;
            ty += dst[i].y - src[i].y;
        }
        const double I[9] = {1, 0, tx / m, 0, 1, ty / m, 0, 0, 1};
        std::memcpy(H, I, sizeof I);
        return true;
    }
    double ss, sx, sy, ds, dx, dy;
    hartley(src, ss, sx, sy);
    hartley(dst, ds, dx, dy);
    const int n = model == SGPU_MODEL_SIMILARITY ? 4 : model == SGPU_MODEL_AFFINE ? 6 : 8;
    std::vector<double> A((size_t)2 * m * n, 0.0), rhs((size_t)2 * m), h;
    for (int i = 0; i < m; i++) {
        const double x = ss * (src[i].x - sx), y = ss * (src[i].y - sy);
        const double u = ds * (dst[i].x - dx), v = ds * (dst[i].y - dy);
        double *r0 = &A[(size_t)(2 * i) * n], *r1 = r0 + n;
        if (model == SGPU_MODEL_SIMILARITY) {  // u = a x - b y + tx, v = b x + a y + ty
            r0[0] = x, r0[1] = -y, r0[2] = 1.0;
            r1[0] = y, r1[1] = x, r1[3] = 1.0;
        } else {
            r0[0] = x, r0[1] = y, r0[2] = 1.0;
            r1[3] = x, r1[4] = y, r1[5] = 1.0;
            if (model == SGPU_MODEL_HOMOGRAPHY) {
                r0[6] = -u * x, r0[7] = -u * y;
                r1[6] = -v * x, r1[7] = -v * y;
            }
        }
        rhs[2 * i] = u;
        rhs[2 * i + 1] = v;
    }
    if (!lstsq(A, rhs, 2 * m, n, h)) return false;
    double Hn[9] = {0, 0, 0, 0, 0, 0, 0, 0, 1};
    if (model == SGPU_MODEL_SIMILARITY) {
        Hn[0] = h[0], Hn[1] = -h[1], Hn[2] = h[2];
        Hn[3] = h[1], Hn[4] = h[0], Hn[5] = h[3];
    } else {
        for (int k = 0; k < n; k++) Hn[k] = h[k];
    }
    const double Ts[9] = {ss, 0, -ss * sx, 0, ss, -ss * sy, 0, 0, 1};
    const double Tdi[9] = {1.0 / ds, 0, dx, 0, 1.0 / ds, dy, 0, 0, 1};
    double t[9];
    mat3(Hn, Ts, t);
    mat3(Tdi, t, H);
    if (!(std::fabs(H[8]) > 0.0)) return false;
    const double w = H[8];
    for (int k = 0; k < 9; k++) {
        H[k] /= w;
        if (!std::isfinite(H[k])) return false;
    }
    return true;
}

}  // namespace

extern "C" void sgpu_match_default_params(sgpu_match_params *p) {
    if (!p) return;
    p->tri_tol = 0.002;
    p->match_radius = 2.0;
    p->nbright = 20;
    p->min_pairs = 10;
    p->model = SGPU_MODEL_HOMOGRAPHY;
    p->reserved = 0;
}

extern "C" int sgpu_match_stars(const double *ref_xy, int nref, const double *img_xy, int nimg, int width,
                                int height, const sgpu_match_params *p, double H[9], int *npairs, int *pairs) {
    if (!ref_xy || !img_xy || !p || !H || !npairs || !pairs || nref < 0 || nimg < 0 || width < 1 || height < 1)
        return fail(SGPU_BAD_ARGUMENT, "bad argument");
    if (p->nbright < 3 || p->nbright > 200 || !(p->tri_tol >= 0.0) || !(p->match_radius > 0.0) || p->min_pairs < 1 ||
        p->model < SGPU_MODEL_SHIFT || p->model > SGPU_MODEL_HOMOGRAPHY)
        return fail(SGPU_BAD_ARGUMENT, "match_stars: parameter out of range");
    for (int k = 0; k < 2 * nref; k++)
        if (!std::isfinite(ref_xy[k])) return fail(SGPU_BAD_ARGUMENT, "match_stars: non-finite coordinate");
    for (int k = 0; k < 2 * nimg; k++)
        if (!std::isfinite(img_xy[k])) return fail(SGPU_BAD_ARGUMENT, "match_stars: non-finite coordinate");
    for (int k = 0; k < 9; k++) H[k] = 0.0;
    *npairs = 0;

    // ---- triangle votes
    const int nr = std::min(nref, p->nbright), ni = std::min(nimg, p->nbright);
    const std::vector<Tri> tr = triangles(ref_xy, nr), ti = triangles(img_xy, ni);
    std::vector<int> votes((size_t)ni * nr, 0);
    for (const Tri &a : ti)
        for (const Tri &b : tr)
            if (a.sign == b.sign && std::fabs(a.ba - b.ba) <= p->tri_tol && std::fabs(a.ca - b.ca) <= p->tri_tol)
                for (int s = 0; s < 3; s++) votes[(size_t)a.v[s] * nr + b.v[s]]++;
    // ---- initial pairs: greedy, descending votes, ties by (img, ref)
    struct Cand {
        int votes, i, j;
    };
    std::vector<Cand> cand;
    for (int i = 0; i < ni; i++)
        for (int j = 0; j < nr; j++)
            if (votes[(size_t)i * nr + j] > 0) cand.push_back({votes[(size_t)i * nr + j], i, j});
    std::sort(cand.begin(), cand.end(), [](const Cand &a, const Cand &b) {
        if (a.votes != b.votes) return a.votes > b.votes;
        if (a.i != b.i) return a.i < b.i;
        return a.j < b.j;
    });
    std::vector<std::pair<int, int>> pr;
    {
        std::vector<char> ui((size_t)ni, 0), uj((size_t)nr, 0);
        for (const Cand &c : cand) {
            if (2 * c.votes < cand[0].votes) break;
            if (ui[c.i] || uj[c.j]) continue;
            ui[c.i] = uj[c.j] = 1;
            pr.push_back({c.i, c.j});
        }
    }
    if (pr.size() < 3) return SGPU_NOT_REGISTERED;
    std::sort(pr.begin(), pr.end());

    // ---- refinement
    auto points = [&](std::vector<Pt> &src, std::vector<Pt> &dst) {
        src.clear();
        dst.clear();
        for (const auto &q : pr) {
            src.push_back({img_xy[2 * q.first], img_xy[2 * q.first + 1]});
            dst.push_back({ref_xy[2 * q.second], ref_xy[2 * q.second + 1]});
        }
    };
    const int rounds[3] = {SGPU_MODEL_SIMILARITY, SGPU_MODEL_AFFINE, p->model};
    const double rad2 = p->match_radius * p->match_radius;
    std::vector<Pt> src, dst;
    double Hc[9];
    std::vector<int> best_j((size_t)nimg), best_i((size_t)nref);
    std::vector<double> mx((size_t)nimg), my((size_t)nimg);
    for (int round = 0; round < 3; round++) {
        points(src, dst);
        if (!fit(rounds[round], src, dst, Hc)) return SGPU_NOT_REGISTERED;
        for (int i = 0; i < nimg; i++) {
            const double x = img_xy[2 * i], y = img_xy[2 * i + 1];
            const double w = (Hc[6] * x + Hc[7] * y) + Hc[8];
            mx[i] = ((Hc[0] * x + Hc[1] * y) + Hc[2]) / w;
            my[i] = ((Hc[3] * x + Hc[4] * y) + Hc[5]) / w;
        }
        // mutual nearest neighbours within the radius (ties: the lowest index)
        std::vector<double> dj((size_t)nref, INFINITY);
        std::fill(best_i.begin(), best_i.end(), -1);
        for (int i = 0; i < nimg; i++) {
            double d = INFINITY;
            best_j[i] = -1;
            for (int j = 0; j < nref; j++) {
                const double ex = mx[i] - ref_xy[2 * j], ey = my[i] - ref_xy[2 * j + 1];
                const double d2 = ex * ex + ey * ey;
                if (d2 < d) {
                    d = d2;
                    best_j[i] = j;
                }
                if (d2 < dj[j]) {
                    dj[j] = d2;
                    best_i[j] = i;
                }
            }
            if (!(d <= rad2)) best_j[i] = -1;
        }
        pr.clear();
        for (int i = 0; i < nimg; i++)
            if (best_j[i] >= 0 && best_i[best_j[i]] == i) pr.push_back({i, best_j[i]});
        if (pr.empty()) return SGPU_NOT_REGISTERED;
    }
    *npairs = (int)pr.size();
    for (size_t k = 0; k < pr.size(); k++) {
        pairs[2 * k] = pr[k].first;
        pairs[2 * k + 1] = pr[k].second;
    }
    if ((int)pr.size() < p->min_pairs) return SGPU_NOT_REGISTERED;
    points(src, dst);
    if (!fit(p->model, src, dst, Hc)) return SGPU_NOT_REGISTERED;
    std::memcpy(H, Hc, sizeof Hc);
    return SGPU_OK;
}
