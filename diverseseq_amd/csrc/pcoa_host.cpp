// The dense symmetric eigensolver behind the Rayleigh-Ritz step of pcoa.hip (host only, no HIP): EISPACK's tred2 and
// tql2 (Householder tridiagonalisation with the transformations accumulated, then implicit QL), restated.  The basis
// of a principal-coordinates run has 512 columns at most, so the matrix is a few MB and the O(n^3) work a fraction of
// a second (DESIGN.md 4.16 has the figure).
#include "pcoa_host.h"

#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

namespace {

// V (row-major n x n, symmetric, lower triangle read) -> the orthogonal Q of Q^T V Q = tridiag(d, e), in V
void tred2(int n, double *V, double *d, double *e) {
    auto v = [&](int r, int c) -> double & { return V[size_t(r) * n + c]; };
    for (int j = 0; j < n; j++) d[j] = v(n - 1, j);
    for (int i = n - 1; i > 0; i--) {
        double scale = 0.0, h = 0.0;
        for (int k = 0; k < i; k++) scale += std::fabs(d[k]);
        if (scale == 0.0) {
            e[i] = d[i - 1];
            for (int j = 0; j < i; j++) {
                d[j] = v(i - 1, j);
                v(i, j) = 0.0;
                v(j, i) = 0.0;
            }
        } else {
            for (int k = 0; k < i; k++) {
                d[k] /= scale;
                h += d[k] * d[k];
            }
            double f = d[i - 1];
            double g = std::sqrt(h);
            if (f > 0) g = -g;
            e[i] = scale * g;
            h -= f * g;
            d[i - 1] = f - g;
            for (int j = 0; j < i; j++) e[j] = 0.0;
            for (int j = 0; j < i; j++) {
                f = d[j];
                v(j, i) = f;
                g = e[j] + v(j, j) * f;
                for (int k = j + 1; k <= i - 1; k++) {
                    g += v(k, j) * d[k];
                    e[k] += v(k, j) * f;
                }
                e[j] = g;
            }
            f = 0.0;
            for (int j = 0; j < i; j++) {
                e[j] /= h;
                f += e[j] * d[j];
            }
            const double hh = f / (h + h);
            for (int j = 0; j < i; j++) e[j] -= hh * d[j];
            for (int j = 0; j < i; j++) {
                f = d[j];
                g = e[j];
                for (int k = j; k <= i - 1; k++) v(k, j) -= f * e[k] + g * d[k];
                d[j] = v(i - 1, j);
                v(i, j) = 0.0;
            }
        }
        d[i] = h;
    }
    for (int i = 0; i < n - 1; i++) {
        v(n - 1, i) = v(i, i);
        v(i, i) = 1.0;
        const double h = d[i + 1];
        if (h != 0.0) {
            for (int k = 0; k <= i; k++) d[k] = v(k, i + 1) / h;
            for (int j = 0; j <= i; j++) {
                double g = 0.0;
                for (int k = 0; k <= i; k++) g += v(k, i + 1) * v(k, j);
                for (int k = 0; k <= i; k++) v(k, j) -= g * d[k];
            }
        }
        for (int k = 0; k <= i; k++) v(k, i + 1) = 0.0;
    }
    for (int j = 0; j < n; j++) {
        d[j] = v(n - 1, j);
        v(n - 1, j) = 0.0;
    }
    v(n - 1, n - 1) = 1.0;
    e[0] = 0.0;
}

// tridiag(d, e) -> eigenvalues in d; Z holds the accumulated transformations TRANSPOSED (row i = column i of tred2's
// Q), so that a rotation of columns i and i + 1 walks two contiguous rows
void tql2(int n, double *Z, double *d, double *e) {
    for (int i = 1; i < n; i++) e[i - 1] = e[i];
    e[n - 1] = 0.0;
    double f = 0.0, tst1 = 0.0;
    const double eps = std::ldexp(1.0, -52);
    for (int l = 0; l < n; l++) {
        tst1 = std::max(tst1, std::fabs(d[l]) + std::fabs(e[l]));
        int m = l;
        while (m < n - 1 && std::fabs(e[m]) > eps * tst1) m++;  // (e[n - 1] == 0 ends the search)
        if (m > l) {
            do {
                double g = d[l];
                double p = (d[l + 1] - g) / (2.0 * e[l]);
                double r = std::hypot(p, 1.0);
                if (p < 0) r = -r;
                d[l] = e[l] / (p + r);
                d[l + 1] = e[l] * (p + r);
                const double dl1 = d[l + 1];
                double h = g - d[l];
                for (int i = l + 2; i < n; i++) d[i] -= h;
                f += h;
                p = d[m];
                double c = 1.0, c2 = c, c3 = c;
                const double el1 = e[l + 1];
                double s = 0.0, s2 = 0.0;
                for (int i = m - 1; i >= l; i--) {
                    c3 = c2;
                    c2 = c;
                    s2 = s;
                    g = c * e[i];
                    h = c * p;
                    r = std::hypot(p, e[i]);
                    e[i + 1] = s * r;
                    s = e[i] / r;
                    c = p / r;
                    p = c * d[i] - s * g;
                    d[i + 1] = h + s * (c * g + s * d[i]);
                    double *zi = Z + size_t(i) * n, *zi1 = zi + n;
                    for (int k = 0; k < n; k++) {
                        h = zi1[k];
                        zi1[k] = s * zi[k] + c * h;
                        zi[k] = c * zi[k] - s * h;
                    }
                }
                p = -s * s2 * c3 * el1 * e[l] / dl1;
                e[l] = s * p;
                d[l] = c * p;
            } while (std::fabs(e[l]) > eps * tst1);
        }
        d[l] += f;
        e[l] = 0.0;
    }
}

}  // namespace

void dvs_symeig_desc(int n, double *a, double *w, double *z) {
    if (n <= 0) return;
    std::vector<double> d(n), e(n);
    tred2(n, a, d.data(), e.data());
    for (int i = 0; i < n; i++)  // the transpose, in place
        for (int j = i + 1; j < n; j++) std::swap(a[size_t(i) * n + j], a[size_t(j) * n + i]);
    tql2(n, a, d.data(), e.data());
    std::vector<int> order(n);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return d[x] > d[y]; });
    for (int j = 0; j < n; j++) {
        w[j] = d[order[j]];
        std::copy_n(a + size_t(order[j]) * n, n, z + size_t(j) * n);
    }
}
