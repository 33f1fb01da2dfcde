// Model fits to empirical variograms (host code; nothing here touches the device): gss_variogram_fit,
// gss_variogram_fit_aniso and gss_variogram_fit_lmc.  The ordinates come from the pair pass of variography.hip; the
// conventions are the library's own (include/gss.h).
#include "gss_internal.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace gss {

namespace {

// f(x), x = h / range: the shapes of vg_shape (gss_internal.h), gamma = nugget + (sill - nugget) f
double fit_shape(int kind, double x, double nu) {
  const double pi = 3.14159265358979323846;
  switch (kind) {
    case GSS_VG_GAUSSIAN: return -std::expm1(-3.0 * x * x);
    case GSS_VG_EXPONENTIAL: return -std::expm1(-3.0 * x);
    case GSS_VG_SPHERICAL: return x < 1.0 ? 1.5 * x - 0.5 * x * x * x : 1.0;
    case GSS_VG_CUBIC: {
      const double x2 = x * x, x3 = x2 * x;
      return x < 1.0 ? 7.0 * x2 - 8.75 * x3 + 3.5 * x3 * x2 - 0.75 * x3 * x3 * x : 1.0;
    }
    case GSS_VG_PENTASPHERICAL: {
      const double x2 = x * x, x3 = x2 * x;
      return x < 1.0 ? 1.875 * x - 1.25 * x3 + 0.375 * x3 * x2 : 1.0;
    }
    case GSS_VG_SINEHOLE: {
      const double t = pi * x;
      return t > 0.0 ? 1.0 - std::sin(t) / t : 0.0;
    }
    default: {  // GSS_VG_MATERN
      const double d = std::sqrt(2.0 * nu) * 3.0 * x;
      if (!(d > 0.0)) return 0.0;
      if (d > 700.0) return 1.0;
      if (nu == 0.5) return -std::expm1(-d);
      if (nu == 1.5) return 1.0 - (1.0 + d) * std::exp(-d);
      if (nu == 2.5) return 1.0 - (1.0 + d + d * d / 3.0) * std::exp(-d);
      if (nu * std::log(2.0 / d) > 690.0) return 0.0;
      const double c = std::exp((1.0 - nu) * 0.6931471805599453 - std::lgamma(nu) + nu * std::log(d));
      return 1.0 - c * std::cyl_bessel_k(nu, d);
    }
  }
}

struct FitData {
  std::vector<double> h, g, w;
  double frac;   // nugget <= frac * sill
};

double fit_residual(const FitData& D, const std::vector<double>& f, double a, double b) {
  double s = 0.0;
  for (size_t k = 0; k < f.size(); ++k) {
    const double r = a + b * f[k] - D.g[k];
    s += D.w[k] * r * r;
  }
  return s;
}

// For a fixed range the objective is a quadratic in (a, b) = (nugget, sill - nugget) over the cone a >= 0, b >= 0,
// (1 - frac) a <= frac b.  Its minimum is the unconstrained one if feasible, else it lies on one of the three edges
// (each a one-variable least squares) or at their common vertex, the origin.  Returns the objective.
double fit_inner_f(const FitData& D, const std::vector<double>& f, double* a_out, double* b_out);

double fit_inner(const FitData& D, int kind, double nu, double range, double* a_out, double* b_out) {
  const size_t m = D.h.size();
  std::vector<double> f(m);
  for (size_t k = 0; k < m; ++k) f[k] = fit_shape(kind, D.h[k] / range, nu);
  return fit_inner_f(D, f, a_out, b_out);
}

// the cone solve for given shape values f_k (isotropic: f(h_k / range); anisotropic: f of the scaled lag)
double fit_inner_f(const FitData& D, const std::vector<double>& f, double* a_out, double* b_out) {
  const size_t m = D.h.size();
  double sw = 0.0, swf = 0.0, swg = 0.0;
  for (size_t k = 0; k < m; ++k) {
    sw += D.w[k];
    swf += D.w[k] * f[k];
    swg += D.w[k] * D.g[k];
  }
  const double fb = swf / sw, gb = swg / sw;
  double sff = 0.0, sfg = 0.0, swff = 0.0, swfg = 0.0;
  for (size_t k = 0; k < m; ++k) {
    sff += D.w[k] * (f[k] - fb) * (f[k] - fb);
    sfg += D.w[k] * (f[k] - fb) * (D.g[k] - gb);
    swff += D.w[k] * f[k] * f[k];
    swfg += D.w[k] * f[k] * D.g[k];
  }
  const double frac = D.frac;
  double best = fit_residual(D, f, 0.0, 0.0), ba = 0.0, bb = 0.0;   // the vertex
  auto feasible = [&](double a, double b) { return a >= 0.0 && b >= 0.0 && (1.0 - frac) * a <= frac * b; };
  auto offer = [&](double a, double b) {
    if (!(std::isfinite(a) && std::isfinite(b)) || !feasible(a, b)) return;
    const double o = fit_residual(D, f, a, b);
    if (o < best) {
      best = o;
      ba = a;
      bb = b;
    }
  };
  if (sff > 0.0) {
    const double b = sfg / sff;
    offer(gb - b * fb, b);                   // unconstrained
  }
  if (swff > 0.0) offer(0.0, swfg / swff);   // nugget = 0
  offer(gb, 0.0);                            // sill = nugget (feasible only when frac = 1)
  if (frac < 1.0) {                          // nugget = frac * sill: a = c b, gamma = b (c + f)
    const double c = frac / (1.0 - frac);
    double num = 0.0, den = 0.0;
    for (size_t k = 0; k < m; ++k) {
      num += D.w[k] * (c + f[k]) * D.g[k];
      den += D.w[k] * (c + f[k]) * (c + f[k]);
    }
    if (den > 0.0) offer(c * (num / den), num / den);
  }
  *a_out = ba;
  *b_out = bb;
  return best;
}

// smallest and largest lag of the usable bins: every range search runs over [hmin / 4, 4 hmax]
void fit_lag_span(const std::vector<double>& h, double* hmin, double* hmax) {
  *hmin = *hmax = h[0];
  for (double v : h) {
    *hmin = v < *hmin ? v : *hmin;
    *hmax = v > *hmax ? v : *hmax;
  }
}

constexpr int FIT_GRID = 256;

// The range search of the isotropic fits: log-spaced grid over [hmin / 4, 4 hmax], then golden section on the best
// bracket to 1e-8 relative width.  at(range) is the objective of the inner solve; the last call is at(*range), so
// whatever `at` leaves behind (nugget and sill, B0 and B1) belongs to the range returned.  Returns that objective.
template <class Objective>
double fit_range_search(const std::vector<double>& h, Objective at, double* range) {
  double hmin, hmax;
  fit_lag_span(h, &hmin, &hmax);
  const double r0 = 0.25 * hmin, r1 = 4.0 * hmax;
  std::vector<double> rg(FIT_GRID), og(FIT_GRID);
  int ib = 0;
  for (int i = 0; i < FIT_GRID; ++i) {
    rg[i] = r0 * std::pow(r1 / r0, (double)i / (double)(FIT_GRID - 1));
    og[i] = at(rg[i]);
    if (og[i] < og[ib]) ib = i;
  }
  double lo = rg[ib > 0 ? ib - 1 : 0], hi = rg[ib < FIT_GRID - 1 ? ib + 1 : FIT_GRID - 1];
  double rbest = rg[ib], obest = og[ib];
  const double gr = 0.6180339887498949;
  double x1 = hi - gr * (hi - lo), x2 = lo + gr * (hi - lo);
  double o1 = at(x1), o2 = at(x2);
  for (int it = 0; it < 200 && (hi - lo) > 1e-8 * 0.5 * (hi + lo); ++it) {
    if (o1 < obest) { obest = o1; rbest = x1; }
    if (o2 < obest) { obest = o2; rbest = x2; }
    if (o1 <= o2) {
      hi = x2;
      x2 = x1;
      o2 = o1;
      x1 = hi - gr * (hi - lo);
      o1 = at(x1);
    } else {
      lo = x1;
      x1 = x2;
      o1 = o2;
      x2 = lo + gr * (hi - lo);
      o2 = at(x2);
    }
  }
  if (o1 < obest) { obest = o1; rbest = x1; }
  if (o2 < obest) { obest = o2; rbest = x2; }
  *range = rbest;
  return at(rbest);
}

double fit_kind(const FitData& D, int kind, double nu, double* nugget, double* sill, double* range) {
  double a, b;
  const double obest = fit_range_search(D.h, [&](double r) { return fit_inner(D, kind, nu, r, &a, &b); }, range);
  *nugget = a;
  *sill = a + b;
  return obest;
}

// ---- linear model of coregionalisation (gss_variogram_fit_lmc) -------------------------------------------------------
// Gamma_k (nz x nz, symmetric) ~ B0 + B1 f_k with B0, B1 positive semidefinite.  Matrices are row-major nz x nz.
constexpr int LMC_MAX_NZ = 8;

// P+: the nearest positive semidefinite matrix in the Frobenius norm.  Cyclic Jacobi, rotations in the fixed order
// (0,1), (0,2), .., (nz-2,nz-1), until the off-diagonal part is below 1e-34 of the whole or 64 sweeps; negative
// eigenvalues are set to 0.  A matrix without a negative eigenvalue is returned as it came (no rounding added).
void lmc_project(int nz, double* M) {
  double A[LMC_MAX_NZ * LMC_MAX_NZ], V[LMC_MAX_NZ * LMC_MAX_NZ];
  for (int i = 0; i < nz; ++i) {
    for (int j = 0; j < nz; ++j) {
      A[i * nz + j] = 0.5 * (M[i * nz + j] + M[j * nz + i]);
      V[i * nz + j] = i == j ? 1.0 : 0.0;
    }
  }
  for (int sweep = 0; sweep < 64; ++sweep) {
    double off = 0.0, all = 0.0;
    for (int i = 0; i < nz; ++i) {
      for (int j = 0; j < nz; ++j) {
        all += A[i * nz + j] * A[i * nz + j];
        if (i != j) off += A[i * nz + j] * A[i * nz + j];
      }
    }
    if (off <= 1e-34 * all) break;
    for (int p = 0; p < nz - 1; ++p) {
      for (int q = p + 1; q < nz; ++q) {
        const double apq = A[p * nz + q];
        if (apq == 0.0) continue;
        const double theta = (A[q * nz + q] - A[p * nz + p]) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), sn = t * c;
        for (int k = 0; k < nz; ++k) {   // columns p, q
          const double akp = A[k * nz + p], akq = A[k * nz + q];
          A[k * nz + p] = c * akp - sn * akq;
          A[k * nz + q] = sn * akp + c * akq;
        }
        for (int k = 0; k < nz; ++k) {   // rows p, q
          const double apk = A[p * nz + k], aqk = A[q * nz + k];
          A[p * nz + k] = c * apk - sn * aqk;
          A[q * nz + k] = sn * apk + c * aqk;
        }
        A[p * nz + q] = A[q * nz + p] = 0.0;
        for (int k = 0; k < nz; ++k) {
          const double vkp = V[k * nz + p], vkq = V[k * nz + q];
          V[k * nz + p] = c * vkp - sn * vkq;
          V[k * nz + q] = sn * vkp + c * vkq;
        }
      }
    }
  }
  bool negative = false;
  for (int i = 0; i < nz; ++i) negative = negative || A[i * nz + i] < 0.0;
  if (!negative) return;
  for (int i = 0; i < nz; ++i) {
    for (int j = i; j < nz; ++j) {
      double v = 0.0;
      for (int k = 0; k < nz; ++k) {
        const double ev = A[k * nz + k];
        if (ev > 0.0) v += V[i * nz + k] * ev * V[j * nz + k];
      }
      M[i * nz + j] = M[j * nz + i] = v;
    }
  }
}

struct LmcData {
  int nz;
  std::vector<double> h, w;
  std::vector<double> G;   // per usable bin: the full nz x nz matrix
};

double lmc_objective(const LmcData& D, const std::vector<double>& f, const double* B0, const double* B1) {
  const int nn = D.nz * D.nz;
  double s = 0.0;
  for (size_t k = 0; k < f.size(); ++k) {
    double r2 = 0.0;
    for (int e = 0; e < nn; ++e) {
      const double r = D.G[k * nn + e] - B0[e] - B1[e] * f[k];
      r2 += r * r;
    }
    s += D.w[k] * r2;
  }
  return s;
}

// Goulard-Voltz sweeps for given shape values f_k, from the unconstrained least-squares solution of every entry.
double lmc_inner(const LmcData& D, const std::vector<double>& f, double* B0, double* B1) {
  const int nz = D.nz, nn = nz * nz;
  const size_t m = f.size();
  double sw = 0.0, swf = 0.0, swff = 0.0;
  for (size_t k = 0; k < m; ++k) {
    sw += D.w[k];
    swf += D.w[k] * f[k];
    swff += D.w[k] * f[k] * f[k];
  }
  const double fb = swf / sw;
  double sff = 0.0;
  for (size_t k = 0; k < m; ++k) sff += D.w[k] * (f[k] - fb) * (f[k] - fb);
  double SG[LMC_MAX_NZ * LMC_MAX_NZ], SFG[LMC_MAX_NZ * LMC_MAX_NZ];
  for (int e = 0; e < nn; ++e) {
    double sg = 0.0, sfg = 0.0;
    for (size_t k = 0; k < m; ++k) {
      sg += D.w[k] * D.G[k * nn + e];
      sfg += D.w[k] * f[k] * D.G[k * nn + e];
    }
    SG[e] = sg;
    SFG[e] = sfg;
    const double gb = sg / sw;
    double c = 0.0;
    for (size_t k = 0; k < m; ++k) c += D.w[k] * (f[k] - fb) * (D.G[k * nn + e] - gb);
    B1[e] = sff > 0.0 ? c / sff : 0.0;
    B0[e] = gb - B1[e] * fb;
  }
  for (int sweep = 0; sweep < 1000; ++sweep) {
    double N0[LMC_MAX_NZ * LMC_MAX_NZ], N1[LMC_MAX_NZ * LMC_MAX_NZ];
    for (int e = 0; e < nn; ++e) N0[e] = (SG[e] - B1[e] * swf) / sw;
    lmc_project(nz, N0);
    for (int e = 0; e < nn; ++e) N1[e] = swff > 0.0 ? (SFG[e] - N0[e] * swf) / swff : 0.0;
    lmc_project(nz, N1);
    double d0 = 0.0, d1 = 0.0, n0 = 0.0, n1 = 0.0;
    for (int e = 0; e < nn; ++e) {
      d0 += (N0[e] - B0[e]) * (N0[e] - B0[e]);
      d1 += (N1[e] - B1[e]) * (N1[e] - B1[e]);
      n0 += N0[e] * N0[e];
      n1 += N1[e] * N1[e];
      B0[e] = N0[e];
      B1[e] = N1[e];
    }
    const double tol = 1e-12 * (std::sqrt(n0) + std::sqrt(n1));
    if (std::sqrt(d0) <= tol && std::sqrt(d1) <= tol) break;
  }
  return lmc_objective(D, f, B0, B1);
}

double lmc_at(const LmcData& D, int kind, double nu, double range, double* B0, double* B1) {
  std::vector<double> f(D.h.size());
  for (size_t k = 0; k < f.size(); ++k) f[k] = fit_shape(kind, D.h[k] / range, nu);
  return lmc_inner(D, f, B0, B1);
}

// the range search with the sweeps as the inner solve
double lmc_kind(const LmcData& D, int kind, double nu, double* range, double* B0, double* B1) {
  return fit_range_search(D.h, [&](double r) { return lmc_at(D, kind, nu, r, B0, B1); }, range);
}

// ---- geometric anisotropy in the plane (gss_variogram_fit_aniso) -----------------------------------------------------
// Outer parameters u = (log r1, log(r2 / r1) <= 0, theta); for fixed u the scaled lag of bin k is
// h_k sqrt(cos^2(phi_k - theta) / r1^2 + sin^2(phi_k - theta) / r2^2) and the rest is the cone solve above.
struct AnisoFit {
  const FitData& D;
  const std::vector<double>& phi;
  int kind;
  double nu;
  double ulo, uhi;   // bounds of log r1
  mutable std::vector<double> f;

  double eval(const double* u, double* a, double* b) const {
    const double r1 = std::exp(u[0]), r2 = r1 * std::exp(u[1]);
    const size_t m = D.h.size();
    f.resize(m);
    for (size_t k = 0; k < m; ++k) {
      const double c = std::cos(phi[k] - u[2]) / r1, sn = std::sin(phi[k] - u[2]) / r2;
      f[k] = fit_shape(kind, D.h[k] * std::sqrt(c * c + sn * sn), nu);
    }
    return fit_inner_f(D, f, a, b);
  }
  double eval(const double* u) const {
    double a, b;
    return eval(u, &a, &b);
  }

  // golden section along u + t dir over t in [lo, hi] to a width of 1e-8 in the parameter that moves most (u holds
  // logarithms and an angle: a relative width for the radii); both ends are offered as well, so that a minimum on a
  // bound (ratio 1) is returned as the bound.  u and *o (the objective at u) are updated when something better is found.
  void line(double* u, const double* dir, double lo, double hi, double* o) const {
    const double gr = 0.6180339887498949;
    const double u0[3] = {u[0], u[1], u[2]};
    double scale = 0.0;
    for (int c = 0; c < 3; ++c) scale = std::fabs(dir[c]) > scale ? std::fabs(dir[c]) : scale;
    double best = *o, tbest = 0.0;
    auto at = [&](double t) {
      for (int c = 0; c < 3; ++c) u[c] = u0[c] + t * dir[c];
      if (u[1] > 0.0) u[1] = 0.0;   // (rounding at the bound)
      const double val = eval(u);
      if (val < best) {
        best = val;
        tbest = t;
      }
      return val;
    };
    at(lo);
    at(hi);
    double x1 = hi - gr * (hi - lo), x2 = lo + gr * (hi - lo);
    double o1 = at(x1), o2 = at(x2);
    for (int it = 0; it < 200 && (hi - lo) * scale > 1e-8; ++it) {
      if (o1 <= o2) {
        hi = x2;
        x2 = x1;
        o2 = o1;
        x1 = hi - gr * (hi - lo);
        o1 = at(x1);
      } else {
        lo = x1;
        x1 = x2;
        o1 = o2;
        x2 = lo + gr * (hi - lo);
        o2 = at(x2);
      }
    }
    for (int c = 0; c < 3; ++c) u[c] = u0[c] + tbest * dir[c];
    if (u[1] > 0.0) u[1] = 0.0;
    *o = best;
  }

  // the part [lo, hi] of t for which u + t dir stays inside the bounds of log r1 and of the log ratio
  void clip(const double* u, const double* dir, double* lo, double* hi) const {
    const double blo[2] = {ulo, -2.772588722239781}, bhi[2] = {uhi, 0.0};   // ratio in [1/16, 1]
    for (int c = 0; c < 2; ++c) {
      if (dir[c] == 0.0) continue;
      double t0 = (blo[c] - u[c]) / dir[c], t1 = (bhi[c] - u[c]) / dir[c];
      if (t0 > t1) {
        const double t = t0;
        t0 = t1;
        t1 = t;
      }
      *lo = *lo < t0 ? t0 : *lo;
      *hi = *hi > t1 ? t1 : *hi;
    }
  }

  // Cyclic line searches from u with brackets w that follow the steps taken (twice the last move, at least a quarter
  // of the last bracket), and after every cycle one search along the cycle's net move, which is what carries the point
  // along a valley that no axis follows; until a whole cycle moves nothing by more than 1e-10.
  double refine(double* u, const double* w0) const {
    double w[3] = {w0[0], w0[1], w0[2]};
    double o = eval(u);
    for (int cycle = 0; cycle < 400; ++cycle) {
      const double start[3] = {u[0], u[1], u[2]};
      for (int i = 0; i < 3; ++i) {
        double dir[3] = {0.0, 0.0, 0.0};
        dir[i] = 1.0;
        double lo = -w[i], hi = w[i];
        clip(u, dir, &lo, &hi);
        const double before = u[i];
        if (hi > lo) line(u, dir, lo, hi, &o);
        const double step = std::fabs(u[i] - before);
        const double shrunk = 0.25 * w[i], grown = 2.0 * step;
        w[i] = grown > shrunk ? grown : shrunk;
        if (w[i] < 1e-7) w[i] = 1e-7;
      }
      double net[3], moved = 0.0;
      for (int c = 0; c < 3; ++c) {
        net[c] = u[c] - start[c];
        moved = std::fabs(net[c]) > moved ? std::fabs(net[c]) : moved;
      }
      if (moved <= 1e-10) break;
      double lo = -1.0, hi = 8.0;
      clip(u, net, &lo, &hi);
      if (hi > lo) line(u, net, lo, hi, &o);
    }
    return o;
  }
};

constexpr int ANISO_NTHETA = 36, ANISO_NR1 = 32, ANISO_NRATIO = 16, ANISO_STARTS = 4;

// -> objective; u = (log r1, log ratio, theta in [0, pi))
double fit_kind_aniso(const FitData& D, const std::vector<double>& phi, int kind, double nu, double* nugget,
                      double* sill, double* u_out) {
  const double pi = 3.14159265358979323846;
  double hmin, hmax;
  fit_lag_span(D.h, &hmin, &hmax);
  AnisoFit F{D, phi, kind, nu, std::log(0.25 * hmin), std::log(4.0 * hmax), {}};
  const double w0[3] = {(F.uhi - F.ulo) / (ANISO_NR1 - 1), 2.772588722239781 / (ANISO_NRATIO - 1), pi / ANISO_NTHETA};
  // the grid; the ANISO_STARTS best points (ties: the first met) start a refinement each
  double so[ANISO_STARTS], su[ANISO_STARTS][3];
  int ns = 0;
  for (int it = 0; it < ANISO_NTHETA; ++it) {
    for (int ir = 0; ir < ANISO_NR1; ++ir) {
      for (int iq = 0; iq < ANISO_NRATIO; ++iq) {
        if (iq == ANISO_NRATIO - 1 && it > 0) continue;   // ratio 1: every angle is the same model
        const double u[3] = {F.ulo + w0[0] * ir, iq == ANISO_NRATIO - 1 ? 0.0 : -2.772588722239781 + w0[1] * iq,
                             w0[2] * it};
        const double o = F.eval(u);
        int pos = ns;
        while (pos > 0 && o < so[pos - 1]) --pos;
        if (pos >= ANISO_STARTS) continue;
        const int last = ns < ANISO_STARTS ? ns : ANISO_STARTS - 1;
        for (int q = last; q > pos; --q) {
          so[q] = so[q - 1];
          for (int c = 0; c < 3; ++c) su[q][c] = su[q - 1][c];
        }
        so[pos] = o;
        for (int c = 0; c < 3; ++c) su[pos][c] = u[c];
        if (ns < ANISO_STARTS) ++ns;
      }
    }
  }
  double obest = 0.0;
  for (int q = 0; q < ns; ++q) {
    const double o = F.refine(su[q], w0);
    if (q == 0 || o < obest) {
      obest = o;
      for (int c = 0; c < 3; ++c) u_out[c] = su[q][c];
    }
  }
  u_out[2] = u_out[2] - pi * std::floor(u_out[2] / pi);
  if (!(u_out[2] < pi)) u_out[2] = 0.0;
  double a, b;
  obest = F.eval(u_out, &a, &b);
  *nugget = a;
  *sill = a + b;
  return obest;
}

}  // namespace

}  // namespace gss

using namespace gss;

extern "C" int32_t gss_variogram_fit(const double* h, const double* gamma, const int64_t* count, int32_t nlags,
                                     const int32_t* kinds, int32_t nkinds, double nu, int32_t weighting,
                                     double max_nugget_frac, gss_variogram_t* best, double* objective) {
  GSS_ENTRY();
  GSS_REQUIRE(h != nullptr && gamma != nullptr && count != nullptr && kinds != nullptr && best != nullptr &&
                  objective != nullptr, "gss_variogram_fit: NULL argument");
  GSS_REQUIRE(nlags >= 1 && nlags <= 65536, "gss_variogram_fit: nlags %d outside 1..65536", nlags);
  GSS_REQUIRE(nkinds >= 1 && nkinds <= 64, "gss_variogram_fit: nkinds %d outside 1..64", nkinds);
  GSS_REQUIRE(weighting >= GSS_FIT_W_COUNT && weighting <= GSS_FIT_W_UNIFORM, "gss_variogram_fit: unknown weighting %d",
              weighting);
  GSS_REQUIRE(max_nugget_frac >= 0.0 && max_nugget_frac <= 1.0, "gss_variogram_fit: max_nugget_frac outside [0, 1]");
  bool matern = false;
  for (int i = 0; i < nkinds; ++i) {
    if (kinds[i] == GSS_VG_POWER) {
      set_error("gss_variogram_fit: the power model has no sill and no range to search; only the stationary kinds are "
                "fitted");
      return GSS_ERR_UNSUPPORTED;
    }
    GSS_REQUIRE(kinds[i] >= GSS_VG_GAUSSIAN && kinds[i] <= GSS_VG_SINEHOLE, "gss_variogram_fit: unknown kind %d",
                kinds[i]);
    matern = matern || kinds[i] == GSS_VG_MATERN;
  }
  if (matern) GSS_REQUIRE(nu > 0.0 && nu <= 50.0, "gss_variogram_fit: Matern order must lie in (0, 50]");
  FitData D;
  D.frac = max_nugget_frac;
  for (int k = 0; k < nlags; ++k) {
    if (count[k] <= 0) continue;
    GSS_REQUIRE(std::isfinite(h[k]) && h[k] > 0.0 && std::isfinite(gamma[k]), "gss_variogram_fit: bin %d has pairs but "
                "no finite positive lag / finite ordinate", k);
    const double c = (double)count[k];
    D.h.push_back(h[k]);
    D.g.push_back(gamma[k]);
    D.w.push_back(weighting == GSS_FIT_W_COUNT ? c : (weighting == GSS_FIT_W_COUNT_OVER_H2 ? c / (h[k] * h[k]) : 1.0));
  }
  GSS_REQUIRE(D.h.size() >= 2, "gss_variogram_fit: fewer than two bins hold pairs");
  int ibest = -1;
  double nbest = 0.0, sbest = 0.0, rbest = 0.0;
  for (int i = 0; i < nkinds; ++i) {
    double ng, sl, rg;
    objective[i] = fit_kind(D, kinds[i], nu, &ng, &sl, &rg);
    if (!(sl > 0.0)) {   // the ordinates admit no model of this kind with a positive sill
      objective[i] = std::nan("");
      continue;
    }
    if (ibest < 0 || objective[i] < objective[ibest]) {
      ibest = i;
      nbest = ng;
      sbest = sl;
      rbest = rg;
    }
  }
  GSS_REQUIRE(ibest >= 0, "gss_variogram_fit: no kind fits these ordinates with a positive sill");
  std::memset(best, 0, sizeof(*best));
  best->kind = kinds[ibest];
  best->dim = 0;   // left to the caller
  best->sill = sbest;
  best->nugget = nbest;
  best->range = rbest;
  best->nu = kinds[ibest] == GSS_VG_MATERN ? nu : 1.0;
  for (int a = 0; a < 3; ++a) {
    best->inv_radii[a] = 1.0;
    best->rotation[4 * a] = 1.0;
  }
  return GSS_OK;
}

extern "C" int32_t gss_variogram_fit_aniso(const double* h, const double* phi, const double* gamma, const int64_t* count,
                                           int32_t nbins, const int32_t* kinds, int32_t nkinds, double nu,
                                           int32_t weighting, double max_nugget_frac, gss_variogram_t* best,
                                           double* objective) {
  GSS_ENTRY();
  GSS_REQUIRE(h != nullptr && phi != nullptr && gamma != nullptr && count != nullptr && kinds != nullptr &&
                  best != nullptr && objective != nullptr, "gss_variogram_fit_aniso: NULL argument");
  GSS_REQUIRE(nbins >= 1 && nbins <= 65536, "gss_variogram_fit_aniso: nbins %d outside 1..65536", nbins);
  GSS_REQUIRE(nkinds >= 1 && nkinds <= 64, "gss_variogram_fit_aniso: nkinds %d outside 1..64", nkinds);
  GSS_REQUIRE(weighting >= GSS_FIT_W_COUNT && weighting <= GSS_FIT_W_UNIFORM,
              "gss_variogram_fit_aniso: unknown weighting %d", weighting);
  GSS_REQUIRE(max_nugget_frac >= 0.0 && max_nugget_frac <= 1.0,
              "gss_variogram_fit_aniso: max_nugget_frac outside [0, 1]");
  bool matern = false;
  for (int i = 0; i < nkinds; ++i) {
    if (kinds[i] == GSS_VG_POWER) {
      set_error("gss_variogram_fit_aniso: the power model has no sill and no range to search; only the stationary "
                "kinds are fitted");
      return GSS_ERR_UNSUPPORTED;
    }
    GSS_REQUIRE(kinds[i] >= GSS_VG_GAUSSIAN && kinds[i] <= GSS_VG_SINEHOLE, "gss_variogram_fit_aniso: unknown kind %d",
                kinds[i]);
    matern = matern || kinds[i] == GSS_VG_MATERN;
  }
  if (matern) GSS_REQUIRE(nu > 0.0 && nu <= 50.0, "gss_variogram_fit_aniso: Matern order must lie in (0, 50]");
  FitData D;
  std::vector<double> ph;
  D.frac = max_nugget_frac;
  for (int k = 0; k < nbins; ++k) {
    if (count[k] <= 0) continue;
    GSS_REQUIRE(std::isfinite(h[k]) && h[k] > 0.0 && std::isfinite(gamma[k]) && std::isfinite(phi[k]),
                "gss_variogram_fit_aniso: bin %d has pairs but no finite positive lag / finite ordinate / finite angle",
                k);
    const double c = (double)count[k];
    D.h.push_back(h[k]);
    D.g.push_back(gamma[k]);
    ph.push_back(phi[k]);
    D.w.push_back(weighting == GSS_FIT_W_COUNT ? c : (weighting == GSS_FIT_W_COUNT_OVER_H2 ? c / (h[k] * h[k]) : 1.0));
  }
  GSS_REQUIRE(D.h.size() >= 4, "gss_variogram_fit_aniso: fewer than four bins hold pairs");
  int ibest = -1;
  double nbest = 0.0, sbest = 0.0, ubest[3] = {0.0, 0.0, 0.0};
  for (int i = 0; i < nkinds; ++i) {
    double ng, sl, u[3];
    objective[i] = fit_kind_aniso(D, ph, kinds[i], nu, &ng, &sl, u);
    if (!(sl > 0.0)) {   // the ordinates admit no model of this kind with a positive sill
      objective[i] = std::nan("");
      continue;
    }
    if (ibest < 0 || objective[i] < objective[ibest]) {
      ibest = i;
      nbest = ng;
      sbest = sl;
      for (int c = 0; c < 3; ++c) ubest[c] = u[c];
    }
  }
  GSS_REQUIRE(ibest >= 0, "gss_variogram_fit_aniso: no kind fits these ordinates with a positive sill");
  std::memset(best, 0, sizeof(*best));
  best->kind = kinds[ibest];
  best->dim = 0;   // left to the caller
  best->sill = sbest;
  best->nugget = nbest;
  best->nu = kinds[ibest] == GSS_VG_MATERN ? nu : 1.0;
  for (int a = 0; a < 3; ++a) {
    best->inv_radii[a] = 1.0;
    best->rotation[4 * a] = 1.0;
  }
  const double r1 = std::exp(ubest[0]);
  if (ubest[1] == 0.0) {   // ratio 1: the isotropic form
    best->range = r1;
    return GSS_OK;
  }
  const double r2 = r1 * std::exp(ubest[1]), c = std::cos(ubest[2]), sn = std::sin(ubest[2]);
  best->aniso = 2;
  best->range = 1.0;
  best->inv_radii[0] = 1.0 / r1;
  best->inv_radii[1] = 1.0 / r2;
  best->rotation[0] = c;
  best->rotation[1] = -sn;
  best->rotation[3] = sn;
  best->rotation[4] = c;
  return GSS_OK;
}

extern "C" int32_t gss_variogram_fit_lmc(const double* h, const double* gamma, const int64_t* count, int32_t nlags,
                                         int32_t nz, const int32_t* kinds, int32_t nkinds, double nu,
                                         int32_t weighting, int32_t* kind, double* range, double* b0, double* b1,
                                         double* objective) {
  GSS_ENTRY();
  GSS_REQUIRE(h != nullptr && gamma != nullptr && count != nullptr && kinds != nullptr && kind != nullptr &&
                  range != nullptr && b0 != nullptr && b1 != nullptr && objective != nullptr,
              "gss_variogram_fit_lmc: NULL argument");
  GSS_REQUIRE(nz >= 1 && nz <= LMC_MAX_NZ, "gss_variogram_fit_lmc: nz %d outside 1..%d", nz, LMC_MAX_NZ);
  GSS_REQUIRE(nlags >= 1 && nlags <= 65536, "gss_variogram_fit_lmc: nlags %d outside 1..65536", nlags);
  GSS_REQUIRE(nkinds >= 1 && nkinds <= 64, "gss_variogram_fit_lmc: nkinds %d outside 1..64", nkinds);
  GSS_REQUIRE(weighting >= GSS_FIT_W_COUNT && weighting <= GSS_FIT_W_UNIFORM,
              "gss_variogram_fit_lmc: unknown weighting %d", weighting);
  bool matern = false;
  for (int i = 0; i < nkinds; ++i) {
    if (kinds[i] == GSS_VG_POWER) {
      set_error("gss_variogram_fit_lmc: the power model has no sill and no range to search; only the stationary kinds "
                "are fitted");
      return GSS_ERR_UNSUPPORTED;
    }
    GSS_REQUIRE(kinds[i] >= GSS_VG_GAUSSIAN && kinds[i] <= GSS_VG_SINEHOLE, "gss_variogram_fit_lmc: unknown kind %d",
                kinds[i]);
    matern = matern || kinds[i] == GSS_VG_MATERN;
  }
  if (matern) GSS_REQUIRE(nu > 0.0 && nu <= 50.0, "gss_variogram_fit_lmc: Matern order must lie in (0, 50]");
  const int nn = nz * nz;
  LmcData D;
  D.nz = nz;
  for (int k = 0; k < nlags; ++k) {
    if (count[k] <= 0) continue;
    GSS_REQUIRE(std::isfinite(h[k]) && h[k] > 0.0, "gss_variogram_fit_lmc: bin %d has pairs but no finite positive lag",
                k);
    const double c = (double)count[k];
    D.h.push_back(h[k]);
    D.w.push_back(weighting == GSS_FIT_W_COUNT ? c : (weighting == GSS_FIT_W_COUNT_OVER_H2 ? c / (h[k] * h[k]) : 1.0));
    const size_t at = D.G.size();
    D.G.resize(at + nn);
    for (int a = 0; a < nz; ++a) {
      for (int b = a; b < nz; ++b) {
        const double g = gamma[(size_t)(a * nz - a * (a - 1) / 2 + (b - a)) * nlags + k];
        GSS_REQUIRE(std::isfinite(g), "gss_variogram_fit_lmc: bin %d has pairs but no finite ordinate (%d, %d)", k, a, b);
        D.G[at + a * nz + b] = D.G[at + b * nz + a] = g;
      }
    }
  }
  GSS_REQUIRE(D.h.size() >= 2, "gss_variogram_fit_lmc: fewer than two bins hold pairs");
  int ibest = -1;
  double B0[LMC_MAX_NZ * LMC_MAX_NZ], B1[LMC_MAX_NZ * LMC_MAX_NZ];
  for (int i = 0; i < nkinds; ++i) {
    double rg = 0.0;
    bool positive = true;
    if (nz == 1) {   // one variable: the positive semidefinite cone is nugget >= 0, sill - nugget >= 0 -- the
      FitData F;     // closed form of gss_variogram_fit with max_nugget_frac = 1, and its very numbers
      F.h = D.h;
      F.g = D.G;
      F.w = D.w;
      F.frac = 1.0;
      double ng, sl;
      objective[i] = fit_kind(F, kinds[i], nu, &ng, &sl, &rg);
      B0[0] = ng;
      B1[0] = sl - ng;
      positive = sl > 0.0;
    } else {
      objective[i] = lmc_kind(D, kinds[i], nu, &rg, B0, B1);
      for (int a = 0; a < nz; ++a) positive = positive && B0[a * nz + a] + B1[a * nz + a] > 0.0;
    }
    if (!positive) {   // a variable without a positive sill: no model of this kind
      objective[i] = std::nan("");
      continue;
    }
    if (ibest < 0 || objective[i] < objective[ibest]) {
      ibest = i;
      *range = rg;
      for (int e = 0; e < nn; ++e) {
        b0[e] = B0[e];
        b1[e] = B1[e];
      }
    }
  }
  GSS_REQUIRE(ibest >= 0, "gss_variogram_fit_lmc: no kind fits these ordinates with a positive sill for every variable");
  *kind = kinds[ibest];
  return GSS_OK;
}
