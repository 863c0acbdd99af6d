// slsqp_box.hpp -- Kraft's SLSQP (D. Kraft, "A software package for sequential quadratic programming", DFVLR-FB 88-28,
// 1988) restricted to box bounds, as scipy.optimize.minimize(method="SLSQP") drives it: ftol 1e-6, at most 100 major
// iterations, the gradient by scipy's 2-point finite difference (absolute step sqrt(eps), flipped to a backward step when the
// forward one leaves the upper bound), the inexact L1 line search (alpha shrunk by a quadratic fit, never below 0.1, at most
// 10 trials), Powell's damped BFGS update kept as LDL' factors with Kraft's rank-one LDL routine.
//
// With no general constraints the QP subproblem is min 0.5 d'Bd + g'd over lb - x <= d <= ub - x.  For one variable it is
// a clip; for NV = 3 it is solved exactly by enumerating the 27 free / lower / upper active sets and keeping the feasible
// candidate of least QP objective (the optimum is one of them; B is positive definite, so it is unique).
//
// Everything is plain f64 straight-line code over compile-time sizes, callable from a kernel (one lane per problem) or from the
// host (the CPU checks run the same code).  Compile with -ffp-contract=off.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define SLSQP_HD __host__ __device__ inline
#else
#define SLSQP_HD inline
#endif

namespace slsqp {

constexpr double ACC = 1.0e-6;                    // ftol
constexpr double FD_STEP = 1.4901161193847656e-08;  // sqrt(DBL_EPSILON), scipy's default eps
constexpr int MAX_ITER = 100;

SLSQP_HD double clampd(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ascending sort of a register array (odd-even transposition network: compile-time indices keep it out of scratch); the
// objectives sum their pursuer terms in this order, as the reference does after dis_ep.sort()
template <int PM>
SLSQP_HD void sort_asc(double *d) {
#pragma unroll
    for (int r = 0; r < PM; r++)
#pragma unroll
        for (int i = r & 1; i + 1 < PM; i += 2) {
            const double lo = fmin(d[i], d[i + 1]), hi = fmax(d[i], d[i + 1]);
            d[i] = lo; d[i + 1] = hi;
        }
}

// 2-point forward difference at x (f0 = f(x)); backward where x + h passes the upper bound.  dx is recomputed as the
// representable step, as scipy's _dense_difference does.  The loop over i stays rolled (one inlined objective, not NV), so
// the arrays are only ever indexed by the unrolled j: they stay in registers.
template <int NV, class Fn>
SLSQP_HD void fd_grad(Fn &fn, const double *x, double f0, const double *ub, double *g) {
    for (int i = 0; i < NV; i++) {
        double xi[NV], dx = 0.0;
#pragma unroll
        for (int j = 0; j < NV; j++) {
            xi[j] = x[j];
            if (j == i) {
                xi[j] = x[j] + ((x[j] + FD_STEP > ub[j]) ? -FD_STEP : FD_STEP);
                dx = xi[j] - x[j];
            }
        }
        const double gi = (fn(xi) - f0) / dx;
#pragma unroll
        for (int j = 0; j < NV; j++)
            if (j == i) g[j] = gi;
    }
}

// Packed LDL' (column-major lower triangle, diagonal D in place of the unit diagonal of L), Kraft's layout.
template <int NV>
struct Ldl {
    static constexpr int N2 = NV * (NV + 1) / 2;
    double a[N2];
    SLSQP_HD void identity() {
        int j = 0;
#pragma unroll
        for (int k = 0; k < N2; k++) a[k] = 0.0;
#pragma unroll
        for (int i = 0; i < NV; i++) { a[j] = 1.0; j += NV - i; }
    }
    // v = L D L' s
    SLSQP_HD void mul(const double *s, double *v) const {
        int k = 0;
#pragma unroll
        for (int i = 0; i < NV; i++) {  // L' s
            double h = 0.0;
            k++;
#pragma unroll
            for (int j = i + 1; j < NV; j++) { h = h + a[k] * s[j]; k++; }
            v[i] = s[i] + h;
        }
        k = 0;
#pragma unroll
        for (int i = 0; i < NV; i++) { v[i] = a[k] * v[i]; k += NV - i; }  // D L' s
#pragma unroll
        for (int i = NV - 1; i >= 0; i--) {  // L D L' s
            double h = 0.0;
            int kk = i;
#pragma unroll
            for (int j = 0; j < i; j++) { h = h + a[kk] * v[j]; kk += NV - 1 - j; }
            v[i] = v[i] + h;
        }
    }
    // A := A + sigma z z' (Kraft's LDL, after Fletcher & Powell); z and w are overwritten
    SLSQP_HD void rank1(double *z, double sigma, double *w) {
        const double EPMACH = 2.22e-16;
        if (sigma == 0.0) return;
        int ij = 0;
        double t = 1.0 / sigma;
        if (sigma < 0.0) {
#pragma unroll
            for (int i = 0; i < NV; i++) w[i] = z[i];
#pragma unroll
            for (int i = 0; i < NV; i++) {
                const double v = w[i];
                t = t + v * v / a[ij];
#pragma unroll
                for (int j = i + 1; j < NV; j++) { ij++; w[j] = w[j] - v * a[ij]; }
                ij++;
            }
            if (t >= 0.0) t = EPMACH / sigma;
#pragma unroll
            for (int i = 0; i < NV; i++) {
                const int j = NV - 1 - i;
                ij -= i + 1;
                const double u = w[j];
                w[j] = t;
                t = t - u * u / a[ij];
            }
        }
#pragma unroll
        for (int i = 0; i < NV; i++) {
            const double v = z[i], delta = v / a[ij];
            const double tp = sigma < 0.0 ? w[i] : t + delta * v;
            const double alpha = tp / t;
            a[ij] = alpha * a[ij];
            if (i == NV - 1) break;
            const double beta = delta / tp;
            if (alpha > 4.0) {
                const double gamma = t / tp;
#pragma unroll
                for (int j = i + 1; j < NV; j++) {
                    ij++;
                    const double u = a[ij];
                    a[ij] = gamma * u + beta * z[j];
                    z[j] = z[j] - v * u;
                }
            } else {
#pragma unroll
                for (int j = i + 1; j < NV; j++) {
                    ij++;
                    z[j] = z[j] - v * a[ij];
                    a[ij] = a[ij] + beta * z[j];
                }
            }
            ij++;
            t = tp;
        }
    }
};

// QP step: argmin 0.5 d'Bd + g'd over lo <= d <= hi
SLSQP_HD void qp_box(const Ldl<1> &L, const double *g, const double *lo, const double *hi, double *d) {
    d[0] = clampd(-g[0] / L.a[0], lo[0], hi[0]);
}

SLSQP_HD void qp_box(const Ldl<3> &L, const double *g, const double *lo, const double *hi, double *d) {
    // B = L D L' from the packed factors: a = [d0, l10, l20, d1, l21, d2]
    const double d0 = L.a[0], l10 = L.a[1], l20 = L.a[2], d1 = L.a[3], l21 = L.a[4], d2 = L.a[5];
    const double b00 = d0, b01 = l10 * d0, b02 = l20 * d0;
    const double b11 = l10 * l10 * d0 + d1, b12 = l10 * l20 * d0 + l21 * d1;
    const double b22 = l20 * l20 * d0 + l21 * l21 * d1 + d2;
    double best = INFINITY;
    d[0] = clampd(0.0, lo[0], hi[0]); d[1] = clampd(0.0, lo[1], hi[1]); d[2] = clampd(0.0, lo[2], hi[2]);
    for (int code = 0; code < 27; code++) {
        const int s0 = code % 3, s1 = (code / 3) % 3, s2 = code / 9;  // 0 free, 1 at lower, 2 at upper
        // free rows keep the stationarity equation (B d + g)_i = 0, fixed rows pin d_i to its bound
        const double m00 = s0 ? 1.0 : b00, m01 = s0 ? 0.0 : b01, m02 = s0 ? 0.0 : b02, r0 = s0 ? (s0 == 1 ? lo[0] : hi[0]) : -g[0];
        const double m10 = s1 ? 0.0 : b01, m11 = s1 ? 1.0 : b11, m12 = s1 ? 0.0 : b12, r1 = s1 ? (s1 == 1 ? lo[1] : hi[1]) : -g[1];
        const double m20 = s2 ? 0.0 : b02, m21 = s2 ? 0.0 : b12, m22 = s2 ? 1.0 : b22, r2 = s2 ? (s2 == 1 ? lo[2] : hi[2]) : -g[2];
        const double c00 = m11 * m22 - m12 * m21, c01 = m12 * m20 - m10 * m22, c02 = m10 * m21 - m11 * m20;
        const double det = m00 * c00 + m01 * c01 + m02 * c02;
        if (!(det != 0.0)) continue;
        const double x0 = (r0 * c00 + m01 * (m12 * r2 - r1 * m22) + m02 * (r1 * m21 - m11 * r2)) / det;
        const double x1 = (m00 * (r1 * m22 - m12 * r2) + r0 * c01 + m02 * (m10 * r2 - r1 * m20)) / det;
        const double x2 = (m00 * (m11 * r2 - r1 * m21) + m01 * (r1 * m20 - m10 * r2) + r0 * c02) / det;
        const double y0 = s0 ? r0 : x0, y1 = s1 ? r1 : x1, y2 = s2 ? r2 : x2;
        if (!(y0 >= lo[0] && y0 <= hi[0] && y1 >= lo[1] && y1 <= hi[1] && y2 >= lo[2] && y2 <= hi[2])) continue;
        const double q = 0.5 * (y0 * (b00 * y0 + b01 * y1 + b02 * y2) + y1 * (b01 * y0 + b11 * y1 + b12 * y2) +
                                y2 * (b02 * y0 + b12 * y1 + b22 * y2)) + (g[0] * y0 + g[1] * y1 + g[2] * y2);
        if (q < best) { best = q; d[0] = y0; d[1] = y1; d[2] = y2; }
    }
}

// Minimises fn over lb <= x <= ub from x (clipped first), in place.  Returns the major iterations taken (scipy's nit).
template <int NV, class Fn>
SLSQP_HD int minimize(Fn &fn, double *x, const double *lb, const double *ub) {
#pragma unroll
    for (int i = 0; i < NV; i++) x[i] = clampd(x[i], lb[i], ub[i]);
    double f = fn(x), g[NV], s[NV], x0[NV], lo[NV], hi[NV], u[NV], v[NV];
    fd_grad<NV>(fn, x, f, ub, g);
    Ldl<NV> L;
    int ireset = 0, iter = 0;
    bool reset = true;
    for (;;) {
        if (reset) {
            if (++ireset > 5) return iter;  // B keeps giving ascent directions: stop where we are (Kraft's relaxed exit)
            L.identity();
            reset = false;
        }
        if (++iter > MAX_ITER) return MAX_ITER;
#pragma unroll
        for (int i = 0; i < NV; i++) { lo[i] = lb[i] - x[i]; hi[i] = ub[i] - x[i]; }
        qp_box(L, g, lo, hi, s);
        const double f0 = f;
        double gs = 0.0;
#pragma unroll
        for (int i = 0; i < NV; i++) { x0[i] = x[i]; gs = gs + g[i] * s[i]; }
        if (fabs(gs) < ACC) return iter;
        const double t0 = f;
        double h3 = gs;
        if (h3 >= 0.0) { reset = true; continue; }
        // inexact line search on the (here unconstrained) L1 merit function
        double alpha = 1.0;
        for (int line = 1;; line++) {
            h3 = alpha * h3;
#pragma unroll
            for (int i = 0; i < NV; i++) { s[i] = alpha * s[i]; x[i] = clampd(x0[i] + s[i], lb[i], ub[i]); }
            f = fn(x);
            const double h1 = f - t0;
            if (h1 <= h3 / 10.0 || line > 10) break;
            alpha = h3 / (2.0 * (h3 - h1));
            if (alpha < 0.1) alpha = 0.1;
        }
        double sn = 0.0;
#pragma unroll
        for (int i = 0; i < NV; i++) sn = sn + s[i] * s[i];
        if (fabs(f - f0) < ACC || sqrt(sn) < ACC) return iter;
        // gradient at the new point, then Powell's damped BFGS update of the LDL' factors
        double gn[NV];
        fd_grad<NV>(fn, x, f, ub, gn);
#pragma unroll
        for (int i = 0; i < NV; i++) u[i] = gn[i] - g[i];
        L.mul(s, v);
        double h1 = 0.0, h2 = 0.0;
#pragma unroll
        for (int i = 0; i < NV; i++) { h1 = h1 + s[i] * u[i]; h2 = h2 + s[i] * v[i]; }
        const double h3b = 0.2 * h2;
        if (h1 < h3b) {
            const double h4 = (h2 - h3b) / (h2 - h1);
            h1 = h3b;
#pragma unroll
            for (int i = 0; i < NV; i++) u[i] = h4 * u[i] + (1.0 - h4) * v[i];
        }
        if (h1 == 0.0 || h2 == 0.0) {
            reset = true;
        } else {
            L.rank1(u, 1.0 / h1, v);
            L.rank1(v, -1.0 / h2, u);
        }
#pragma unroll
        for (int i = 0; i < NV; i++) g[i] = gn[i];
    }
}

}  // namespace slsqp
