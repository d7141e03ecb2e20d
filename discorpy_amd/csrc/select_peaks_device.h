// select_peaks_device.h -- the device code of select_good_peaks shared by select_peaks_kernel (select_peaks_kernels.hip: candidates from host
// tables) and extrema_fit_kernel (extrema_select_kernels.hip: candidates drawn from a worklist on the device): one wave fits one window.
//   fit_window              the window into LDS, the normalisation, the least-squares fit of a exp(-((x - c) / (2 b^2))^2) + d from
//                           (1, 1, 0, 0), the 80th percentile of |fit - y| and the decision
//   parabola_position       the sub-pixel position of a point of the peak search (peak_rows_kernel, extrema_compact_kernel)
// The fit is the Levenberg-Marquardt iteration of MINPACK's lmdif as scipy's curve_fit runs it for the reference ("Peak
// selection"): Jacobian by forward differences, columns scaled by the running maximum of their norms, a trust region on the scaled
// step, the tolerances 1.49012e-8 and the budget of 200 (4 + 1) evaluations -- on the normal equations J^T J, J^T r, whose fourteen sums
// and the cost are reduced across the wave in a fixed order.  Everything is float64.  Built with -ffp-contract=off: both kernels run
// the same sequence of IEEE operations on a window, so they decide alike bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include "dcp_device.h"

namespace dcp {

constexpr int kFitBlock = 256;                        // four waves: four candidates
constexpr int kFitWaves = kFitBlock / 64;
constexpr int kFitMaxWindow = 2 * kSelectMaxRadius + 1;
constexpr int kFitMaxEvals = 1000;                    // evaluations of the model per fit: curve_fit's maxfev = 200 (4 + 1); a Jacobian counts 4
constexpr double kFitTol = 1.49012e-8;                // curve_fit's ftol and xtol
constexpr double kFitStepEps = 1.4901161193847656e-08;   // sqrt(2^-52): the relative step of the forward differences
constexpr double kFitFactor = 100.0;                  // the first trust region: 100 |D x|
constexpr double kFitEps = 2.220446049250313e-16, kFitDwarf = 2.2250738585072014e-308;

// the sum over the wave in a fixed order: every lane ends with the same bits (a + b == b + a at every level of the butterfly)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmin(v, __shfl_xor(v, m, 64));
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m, 64));
  return v;
}

__device__ __forceinline__ double fit_model(double x, double a, double b, double c, double d) {
  const double t = (x - c) / (2.0 * (b * b));
  return a * exp(-(t * t)) + d;
}

// A symmetric 4 x 4 system in registers: the lower Cholesky factor of a (false where a is not positive definite), and the two
// triangular solves.
__device__ __forceinline__ bool chol4(const double (&a)[4][4], double (&l)[4][4]) {
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    double s = a[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) s -= l[j][k] * l[j][k];
    ok = ok && s > 0.0 && __builtin_isfinite(s);
    const double ljj = sqrt(s);
    l[j][j] = ljj;
#pragma unroll
    for (int i = j + 1; i < 4; ++i) {
      double u = a[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) u -= l[i][k] * l[j][k];
      l[i][j] = u / ljj;
    }
  }
  return ok;
}
__device__ __forceinline__ void forward4(const double (&l)[4][4], const double (&b)[4], double (&z)[4]) {   // l z = b
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    double s = b[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s -= l[i][k] * z[k];
    z[i] = s / l[i][i];
  }
}
__device__ __forceinline__ void backward4(const double (&l)[4][4], const double (&z)[4], double (&x)[4]) {   // l^T x = z
#pragma unroll
  for (int i = 3; i >= 0; --i) {
    double s = z[i];
#pragma unroll
    for (int k = i + 1; k < 4; ++k) s -= l[k][i] * x[k];
    x[i] = s / l[i][i];
  }
}
__device__ __forceinline__ double scaled_norm4(const double (&diag)[4], const double (&p)[4]) {
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j) s += (diag[j] * p[j]) * (diag[j] * p[j]);
  return sqrt(s);
}

// MINPACK's lmpar on the normal equations: the step p of (h + par D^2) p = -g whose scaled length |D p| lies within a tenth of
// delta, or the Gauss-Newton step (par = 0) where that one is short enough.  par: the previous parameter in, this step's out.
__device__ __forceinline__ void fit_step(const double (&h)[4][4], const double (&g)[4], const double (&diag)[4], double delta, double& par,
                                         double (&p)[4]) {
  double l[4][4], z[4], q[4];
  double parl = 0.0, dxnorm, fp;
  if (chol4(h, l)) {
    forward4(l, g, z);
    backward4(l, z, p);
#pragma unroll
    for (int j = 0; j < 4; ++j) p[j] = -p[j];
    dxnorm = scaled_norm4(diag, p);
    fp = dxnorm - delta;
    if (fp <= 0.1 * delta) {
      par = 0.0;
      return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) q[j] = diag[j] * (diag[j] * p[j]) / dxnorm;
    forward4(l, q, z);
    parl = fp / (delta * (z[0] * z[0] + z[1] * z[1] + z[2] * z[2] + z[3] * z[3]));
  } else {                                            // a rank-deficient Jacobian: no Gauss-Newton step, no lower bound
#pragma unroll
    for (int j = 0; j < 4; ++j) p[j] = 0.0;
    dxnorm = __builtin_inf();
    fp = __builtin_inf();
  }
  double gs = 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j) gs += (g[j] / diag[j]) * (g[j] / diag[j]);
  const double gnorm = sqrt(gs);
  double paru = gnorm / delta;
  if (paru == 0.0) paru = kFitDwarf / fmin(delta, 0.1);
  par = fmin(fmax(par, parl), paru);
  if (par == 0.0) par = gnorm / dxnorm;
  for (int it = 1; it <= 10; ++it) {
    if (par == 0.0) par = fmax(kFitDwarf, 0.001 * paru);
    double a[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) a[i][j] = i == j ? h[i][j] + par * (diag[j] * diag[j]) : h[i][j];
    if (!chol4(a, l)) {
      par = par * 10.0;
      continue;
    }
    forward4(l, g, z);
    backward4(l, z, p);
#pragma unroll
    for (int j = 0; j < 4; ++j) p[j] = -p[j];
    dxnorm = scaled_norm4(diag, p);
    const double before = fp;
    fp = dxnorm - delta;
    if (fabs(fp) <= 0.1 * delta || (parl == 0.0 && fp <= before && before < 0.0) || it == 10) break;
#pragma unroll
    for (int j = 0; j < 4; ++j) q[j] = diag[j] * (diag[j] * p[j]) / dxnorm;
    forward4(l, q, z);
    const double parc = fp / (delta * (z[0] * z[0] + z[1] * z[1] + z[2] * z[2] + z[3] * z[3]));
    if (fp > 0.0) parl = fmax(parl, par);
    if (fp < 0.0) paru = fmin(paru, par);
    par = fmax(parl, par + parc);
  }
}

// What one wave found out about its window: (a, b, c, d), the 80th percentile of |fit - y|, the FitStatus and the decision.  Valid in
// lane 0 of a wave whose `active` was true; NaN for what was not computed.
struct FitResult {
  double x[4];
  double num;
  int status;
  bool good;
};

// One wave, one window of n <= kFitMaxWindow samples, sample i = load(i) as a double.  EVERY thread of the workgroup calls this at the
// same point (there are two workgroup barriers inside); a wave without a candidate passes active = false.  y: the wave's kFitMaxWindow
// doubles of LDS, pick: its two.  y[i], i = lane, lane + 64, ...: every lane reads and writes its own samples only, up to the rank
// count behind the first barrier.
template <typename Load>
__device__ __forceinline__ FitResult fit_window(bool active, int n, int radius, double tol, int use_offset, double* __restrict__ y,
                                                double* __restrict__ pick, int lane, Load&& load) {
  const double nan = __builtin_nan("");
  FitResult res;
  int status = kFitShort;
  double x[4] = {nan, nan, nan, nan};                 // a, b, c, d
  if (!active) n = 0;
  DCP_BOUNDS(0u, (uint32_t)n * sizeof(double), kFitMaxWindow * sizeof(double), 43);
  for (int i = lane; i < n; i += 64) y[i] = load(i);
  if (active && n > 3) {
    double lo = __builtin_inf(), hi = -__builtin_inf(), sum = 0.0;
    bool finite = true;
    for (int i = lane; i < n; i += 64) {
      const double w = y[i];
      finite = finite && __builtin_isfinite(w);
      lo = fmin(lo, w);
      hi = fmax(hi, w);
      sum += w;
    }
    finite = __all(finite);
    lo = wave_min(lo);
    hi = wave_max(hi);
    if (!finite) {
      status = kFitNotFinite;
    } else if (lo == hi) {
      status = kFitConstant;
    } else {
      // y = (w - min) / std, std the population standard deviation about sum / n
      const double mean = wave_sum(sum) / (double)n;
      double dev = 0.0;
      for (int i = lane; i < n; i += 64) dev += (y[i] - mean) * (y[i] - mean);
      const double sd = sqrt(wave_sum(dev) / (double)n);
      for (int i = lane; i < n; i += 64) y[i] = (y[i] - lo) / sd;
      const int half = n / 2;                         // x_i = i - n // 2
      x[0] = 1.0, x[1] = 1.0, x[2] = 0.0, x[3] = 0.0;
      double cost = 0.0;
      for (int i = lane; i < n; i += 64) {
        const double r = fit_model((double)(i - half), x[0], x[1], x[2], x[3]) - y[i];
        cost += r * r;
      }
      double fnorm = sqrt(wave_sum(cost));
      int nfev = 1;
      double diag[4] = {1.0, 1.0, 1.0, 1.0};
      double par = 0.0, delta = 0.0, xnorm = 0.0;
      bool first = true;
      status = kFitBudget;
      while (status == kFitBudget && nfev < kFitMaxEvals) {
        // the Jacobian by forward differences and the sums of J^T J and J^T r, each lane over its samples in ascending order
        double step[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          step[j] = kFitStepEps * fabs(x[j]);
          if (step[j] == 0.0) step[j] = kFitStepEps;
        }
        double hs[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, gs[4] = {0.0, 0.0, 0.0, 0.0};
        for (int i = lane; i < n; i += 64) {
          const double xi = (double)(i - half);
          const double r = fit_model(xi, x[0], x[1], x[2], x[3]) - y[i];
          double jac[4];
          jac[0] = ((fit_model(xi, x[0] + step[0], x[1], x[2], x[3]) - y[i]) - r) / step[0];
          jac[1] = ((fit_model(xi, x[0], x[1] + step[1], x[2], x[3]) - y[i]) - r) / step[1];
          jac[2] = ((fit_model(xi, x[0], x[1], x[2] + step[2], x[3]) - y[i]) - r) / step[2];
          jac[3] = ((fit_model(xi, x[0], x[1], x[2], x[3] + step[3]) - y[i]) - r) / step[3];
          int k = 0;
#pragma unroll
          for (int a = 0; a < 4; ++a) {
#pragma unroll
            for (int b = 0; b <= a; ++b) hs[k++] += jac[a] * jac[b];
            gs[a] += jac[a] * r;
          }
        }
        nfev += 4;
        double h[4][4], g[4];
        {
          int k = 0;
#pragma unroll
          for (int a = 0; a < 4; ++a) {
#pragma unroll
            for (int b = 0; b <= a; ++b) {
              const double v = wave_sum(hs[k++]);
              h[a][b] = v;
              h[b][a] = v;
            }
            g[a] = wave_sum(gs[a]);
          }
        }
        bool sane = true;
        double colnorm[4], gmax = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          sane = sane && __builtin_isfinite(h[j][j]) && __builtin_isfinite(g[j]);
          colnorm[j] = sqrt(h[j][j]);
          gmax = fmax(gmax, fabs(g[j]));
        }
        if (!sane) {
          status = kFitDiverged;
          break;
        }
        if (first) {
#pragma unroll
          for (int j = 0; j < 4; ++j) diag[j] = colnorm[j] == 0.0 ? 1.0 : colnorm[j];
          xnorm = scaled_norm4(diag, x);
          delta = xnorm != 0.0 ? kFitFactor * xnorm : kFitFactor;
        }
        if (fnorm == 0.0 || gmax == 0.0) {            // nothing left to reduce, or the residuals stand at right angles to every column
          status = kFitOk;
          break;
        }
        double gnorm = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (colnorm[j] != 0.0) gnorm = fmax(gnorm, fabs(g[j] / (fnorm * colnorm[j])));
        if (gnorm <= kFitEps) {                       // MINPACK's info 8, which curve_fit raises on
          status = kFitGradient;
          break;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) diag[j] = fmax(diag[j], colnorm[j]);
        for (;;) {
          double p[4], xn[4];
          fit_step(h, g, diag, delta, par, p);
          bool okstep = true;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            okstep = okstep && __builtin_isfinite(p[j]);
            xn[j] = x[j] + p[j];
          }
          if (!okstep) {
            status = kFitDiverged;
            break;
          }
          const double pnorm = scaled_norm4(diag, p);
          if (first) {
            delta = fmin(delta, pnorm);
            first = false;
          }
          double c1 = 0.0;
          for (int i = lane; i < n; i += 64) {
            const double r = fit_model((double)(i - half), xn[0], xn[1], xn[2], xn[3]) - y[i];
            c1 += r * r;
          }
          ++nfev;
          double fnorm1 = sqrt(wave_sum(c1));
          if (!__builtin_isfinite(fnorm1)) fnorm1 = __builtin_inf();
          double actred = -1.0;
          if (0.1 * fnorm1 < fnorm) actred = 1.0 - (fnorm1 / fnorm) * (fnorm1 / fnorm);
          double php = 0.0;                           // |J p|^2 = p^T (J^T J) p
#pragma unroll
          for (int a = 0; a < 4; ++a) {
            double s = 0.0;
#pragma unroll
            for (int b = 0; b < 4; ++b) s += h[a][b] * p[b];
            php += p[a] * s;
          }
          const double temp1 = sqrt(fmax(php, 0.0)) / fnorm, temp2 = sqrt(par) * pnorm / fnorm;
          const double prered = temp1 * temp1 + temp2 * temp2 / 0.5, dirder = -(temp1 * temp1 + temp2 * temp2);
          const double ratio = prered != 0.0 ? actred / prered : 0.0;
          if (ratio <= 0.25) {
            double temp = actred >= 0.0 ? 0.5 : 0.5 * dirder / (dirder + 0.5 * actred);
            if (0.1 * fnorm1 >= fnorm || temp < 0.1) temp = 0.1;
            delta = temp * fmin(delta, pnorm / 0.1);
            par = par / temp;
          } else if (par == 0.0 || ratio >= 0.75) {
            delta = pnorm / 0.5;
            par = 0.5 * par;
          }
          if (ratio >= 1.0e-4) {
#pragma unroll
            for (int j = 0; j < 4; ++j) x[j] = xn[j];
            xnorm = scaled_norm4(diag, x);
            fnorm = fnorm1;
          }
          // the relative decrease of the cost, actual and predicted, or the trust region against the scaled parameters
          if (fabs(actred) <= kFitTol && prered <= kFitTol && 0.5 * ratio <= 1.0) status = kFitOk;
          if (delta <= kFitTol * xnorm) status = kFitOk;
          if (status == kFitOk || ratio >= 1.0e-4 || nfev >= kFitMaxEvals) break;
        }
      }
      if (status == kFitOk && !(__builtin_isfinite(x[0]) && __builtin_isfinite(x[1]) && __builtin_isfinite(x[2]) && __builtin_isfinite(x[3]) &&
                                __builtin_isfinite(fnorm)))
        status = kFitDiverged;
      if (status == kFitOk)
        for (int i = lane; i < n; i += 64) y[i] = fabs(fit_model((double)(i - half), x[0], x[1], x[2], x[3]) - y[i]);
    }
  }
  __syncthreads();
  // np.percentile(|fit - y|, 80): the sorted values at floor(0.8 (n - 1)) and behind it, by a rank count (ties by index)
  double frac = 0.0;
  if (status == kFitOk) {
    const double pos = 0.8 * (double)(n - 1);
    const int k0 = (int)pos, k1 = min(k0 + 1, n - 1);
    frac = pos - (double)k0;
    for (int e = lane; e < n; e += 64) {
      const double ve = y[e];
      int rank = 0;
      for (int j = 0; j < n; ++j) {
        const double vj = y[j];
        rank += (vj < ve || (vj == ve && j < e)) ? 1 : 0;
      }
      if (rank == k0) pick[0] = ve;
      if (rank == k1) pick[1] = ve;
    }
  }
  __syncthreads();
  double num = nan;
  bool good = false;
  if (status == kFitOk) {
    num = pick[0] + frac * (pick[1] - pick[0]);
    good = fabs(x[2]) < (double)(radius / 2) && num < tol && (!use_offset || fabs(x[3]) < tol);
  }
  res.x[0] = x[0], res.x[1] = x[1], res.x[2] = x[2], res.x[3] = x[3];
  res.num = num;
  res.status = status;
  res.good = good;
  return res;
}

// The sub-pixel position of the point at sample ip: the parabola through d0, d1, d2 = row[ip - 1 .. ip + 1] in float64, vertex
// -b / (2 a) where it lies in [0, 3), else the argmin of the three.
__device__ __forceinline__ double parabola_position(int ip, double d0, double d1, double d2) {
  const double a = (d0 - 2.0 * d1 + d2) / 2.0;
  const double b = (-3.0 * d0 + 4.0 * d1 - d2) / 2.0;
  double off = d1 < d0 ? (d2 < d1 ? 2.0 : 1.0) : (d2 < d0 ? 2.0 : 0.0);
  if (a != 0.0) {
    const double num = -b / (2.0 * a);
    if (num >= 0.0 && num < 3.0) off = num;
  }
  return (double)(ip - 1) + off;
}

}  // namespace dcp
