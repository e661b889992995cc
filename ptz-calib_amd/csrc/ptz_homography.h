// ptz_homography.h -- the pair homography estimator of host/homography.cc (FindHomographyRansac, the stand-in for
// cv::findHomography(src, dst, RANSAC, thresh) of LoadMatchesInfo, data_io.cc:340-355, 384-385 of the reference) as
// fixed-size FP64 building blocks.
//
// Every function performs the host's operations in the host's order, without contraction, so the device kernel
// (ptz_homography.hip) and the host instantiation of this header (tests/cpu_harness/homography_harness.cc) return the
// host estimator's bits: found flag, H (row-major, h33 = 1) and inlier mask.  What the kernel spreads over lanes --
// hypotheses of one batch, accumulator entries, points of an integer count -- is a set of independent computations
// here; no floating-point sum is ever split.  ptzh_find_homography_seq composes them in the host's sequence.
//
// Points are interleaved (u, v) float pairs: p[2 i], p[2 i + 1] = cv::Point2f x, y of correspondence i.  Matrices
// handed to the Jacobi SVD live in caller storage with element k at A[k * ld] (ld = 64 for a lane's slot in LDS).
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PTZ_HD __host__ __device__ __forceinline__
#else
#define PTZ_HD inline
#endif

#if !defined(__HIP_DEVICE_COMPILE__)
#include <algorithm>
#include <cmath>
#endif

#if defined(__clang__)
#pragma clang fp contract(off)  // the host library is built without FMA: every product and sum rounds on its own
#endif

namespace ptz {

constexpr uint64_t PTZH_SEED = 0x50545A48ull;  // Rng(0x50545A48u) of FindHomographyRansac
constexpr int PTZH_MAX_ITERS = 2000;           // adaptive bound starts here
constexpr int PTZH_MAX_TRIES = 100;            // degenerate samples redrawn up to this many times per iteration

// ---- SplitMix64 and the index draw ------------------------------------------------------------------------------------
PTZ_HD uint64_t ptzh_next(uint64_t& s)
{
  uint64_t z = (s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
PTZ_HD int ptzh_below(uint64_t& s, int n) { return static_cast<int>(ptzh_next(s) % static_cast<uint64_t>(n)); }

// ---- the forward transfer error ---------------------------------------------------------------------------------------
PTZ_HD double ptzh_err2(const double* H, const float* a, const float* b)
{
  const double ax = a[0], ay = a[1];
  const double w = H[6] * ax + H[7] * ay + H[8];
  const double iw = fabs(w) > 2.2e-16 ? 1.0 / w : 0.0;  // a point mapped to infinity counts as a gross error
  const double dx = (H[0] * ax + H[1] * ay + H[2]) * iw - static_cast<double>(b[0]);
  const double dy = (H[3] * ax + H[4] * ay + H[5]) * iw - static_cast<double>(b[1]);
  return dx * dx + dy * dy;
}

// ---- minimal samples ----------------------------------------------------------------------------------------------------
// three of the four sample points (nearly) on a line; the coordinate differences are float differences, as in the host
PTZ_HD bool ptzh_degenerate(const float* p, const int* s)
{
  for (int a = 0; a < 4; ++a)
    for (int b = a + 1; b < 4; ++b)
      for (int c = b + 1; c < 4; ++c) {
        const float fx1 = p[2 * s[b]] - p[2 * s[a]], fy1 = p[2 * s[b] + 1] - p[2 * s[a] + 1];
        const float fx2 = p[2 * s[c]] - p[2 * s[a]], fy2 = p[2 * s[c] + 1] - p[2 * s[a] + 1];
        const double x1 = fx1, y1 = fy1, x2 = fx2, y2 = fy2;
        if (fabs(x1 * y2 - x2 * y1) <= 1e-7 * (fabs(x1) + fabs(y1) + fabs(x2) + fabs(y2))) return true;
      }
  return false;
}

// One RANSAC iteration's sample: distinct indices, redrawn while degenerate (up to PTZH_MAX_TRIES); false = no valid sample,
// the iteration is consumed all the same.  n >= 5.
PTZ_HD bool ptzh_draw_sample(uint64_t& rng, int n, const float* src, const float* dst, int* s)
{
  bool ok = false;
  for (int tries = 0; tries < PTZH_MAX_TRIES && !ok; ++tries) {
    for (int k = 0; k < 4;) {
      s[k] = ptzh_below(rng, n);
      bool dup = false;
      for (int q = 0; q < k; ++q) dup |= (s[q] == s[k]);
      if (!dup) ++k;
    }
    ok = !ptzh_degenerate(src, s) && !ptzh_degenerate(dst, s);
  }
  return ok;
}

// ---- one-sided Jacobi SVD of an N x N matrix (small_linalg.cc JacobiSVD with m = n = N) --------------------------------
// A is overwritten with A V, W receives V before the sort; norm[j] = |column j of A V|, order = stable descending sort of
// the norms.  The sorted SVD is then s[j] = norm[order[j]], V(:, j) = W(:, order[j]), U(:, j) = (A V)(:, order[j]) / s[j].
template <int N>
PTZ_HD void ptzh_jacobi(double* A, double* W, int ld, double* norm, int* order)
{
  for (int k = 0; k < N * N; ++k) W[k * ld] = 0.0;
  for (int j = 0; j < N; ++j) W[(j * N + j) * ld] = 1.0;
  const double eps = 1e-15;
  for (int sweep = 0; sweep < 60; ++sweep) {
    bool rotated = false;
    for (int p = 0; p < N - 1; ++p)
      for (int q = p + 1; q < N; ++q) {
        double alpha = 0, beta = 0, gamma = 0;
        for (int i = 0; i < N; ++i) {
          const double ap = A[(i * N + p) * ld], aq = A[(i * N + q) * ld];
          alpha += ap * ap; beta += aq * aq; gamma += ap * aq;
        }
        if (fabs(gamma) <= eps * sqrt(alpha * beta) || gamma == 0.0) continue;
        rotated = true;
        const double zeta = (beta - alpha) / (2.0 * gamma);
        const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + t * t), sn = c * t;
        for (int i = 0; i < N; ++i) {
          const double x = A[(i * N + p) * ld], y = A[(i * N + q) * ld];
          A[(i * N + p) * ld] = c * x - sn * y;
          A[(i * N + q) * ld] = sn * x + c * y;
        }
        for (int i = 0; i < N; ++i) {
          const double x = W[(i * N + p) * ld], y = W[(i * N + q) * ld];
          W[(i * N + p) * ld] = c * x - sn * y;
          W[(i * N + q) * ld] = sn * x + c * y;
        }
      }
    if (!rotated) break;
  }
  for (int j = 0; j < N; ++j) {
    double a = 0;
    for (int i = 0; i < N; ++i) a += A[(i * N + j) * ld] * A[(i * N + j) * ld];
    norm[j] = sqrt(a);
  }
  // stable descending sort (insertion: equal norms keep their order, as std::stable_sort does)
  for (int j = 0; j < N; ++j) order[j] = j;
  for (int a = 1; a < N; ++a)
    for (int b = a; b > 0 && norm[order[b]] > norm[order[b - 1]]; --b) {
      const int t = order[b]; order[b] = order[b - 1]; order[b - 1] = t;
    }
}

// ---- normalised DLT (FitHomographyDLT) ------------------------------------------------------------------------------------
// Normalisation of the points idx[0..m): centroid and sqrt(2) / mean distance.  m >= 1.
PTZ_HD void ptzh_normalisation(const float* p, const int* idx, int m, double* cs)
{
  double cx = 0, cy = 0;
  for (int k = 0; k < m; ++k) { cx += p[2 * idx[k]]; cy += p[2 * idx[k] + 1]; }
  cx /= m; cy /= m;
  double d = 0;
  for (int k = 0; k < m; ++k) {
    const int i = idx[k];
    d += sqrt((p[2 * i] - cx) * (p[2 * i] - cx) + (p[2 * i + 1] - cy) * (p[2 * i + 1] - cy));
  }
  d /= m;
  cs[0] = cx; cs[1] = cy; cs[2] = d > 1e-12 ? sqrt(2.0) / d : 1.0;
}

// Entry a of the two DLT rows of one normalised correspondence: r0 = (x, y, 1, 0, 0, 0, -u x, -u y, -u),
// r1 = (0, 0, 0, x, y, 1, -v x, -v y, -v).
PTZ_HD double ptzh_dlt_r0(int a, double x, double y, double u)
{
  return a == 0 ? x : a == 1 ? y : a == 2 ? 1.0 : a < 6 ? 0.0 : a == 6 ? -u * x : a == 7 ? -u * y : -u;
}
PTZ_HD double ptzh_dlt_r1(int a, double x, double y, double v)
{
  return a < 3 ? 0.0 : a == 3 ? x : a == 4 ? y : a == 5 ? 1.0 : a == 6 ? -v * x : a == 7 ? -v * y : -v;
}

// AtA[9 a + b] of the normalised DLT over idx[0..m) (the host adds the points in index order).  cs = (cxa, cya, sa, cxb, cyb, sb).
// The products commute, so entry (b, a) has the bits of entry (a, b).
PTZ_HD double ptzh_ata_entry(int a, int b, const float* src, const float* dst, const int* idx, int m, const double* cs)
{
  double acc = 0.0;
  for (int k = 0; k < m; ++k) {
    const int i = idx[k];
    const double x = (src[2 * i] - cs[0]) * cs[2], y = (src[2 * i + 1] - cs[1]) * cs[2];
    const double u = (dst[2 * i] - cs[3]) * cs[5], v = (dst[2 * i + 1] - cs[4]) * cs[5];
    acc += ptzh_dlt_r0(a, x, y, u) * ptzh_dlt_r0(b, x, y, u) + ptzh_dlt_r1(a, x, y, v) * ptzh_dlt_r1(b, x, y, v);
  }
  return acc;
}

PTZ_HD void ptzh_mul33(const double* a, const double* b, double* c)
{
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) c[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}

// The DLT's second half: AtA (81 entries) sits in A (stride ld), W is the second 81-entry matrix of the same storage.
// Eigenvector of the smallest eigenvalue, normalisations undone, h33 = 1.  Returns false where the host's fit fails.
PTZ_HD bool ptzh_dlt_solve(double* A, double* W, int ld, const double* cs, double* H)
{
  double norm[9];
  int order[9];
  ptzh_jacobi<9>(A, W, ld, norm, order);
  double Hn[9];
  for (int k = 0; k < 9; ++k) Hn[k] = W[(k * 9 + order[8]) * ld];
  const double Ta[9] = {cs[2], 0, -cs[2] * cs[0], 0, cs[2], -cs[2] * cs[1], 0, 0, 1};
  const double Tbi[9] = {1.0 / cs[5], 0, cs[3], 0, 1.0 / cs[5], cs[4], 0, 0, 1};
  double T[9];
  ptzh_mul33(Tbi, Hn, T);
  ptzh_mul33(T, Ta, H);
  if (!(fabs(H[8]) > 1e-300)) return false;
  const double inv = 1.0 / H[8];
  for (int k = 0; k < 9; ++k) H[k] *= inv;
  for (int k = 0; k < 9; ++k)
    if (!isfinite(H[k])) return false;
  return true;
}

// FitHomographyDLT over idx[0..m), every step in one thread; ws holds 162 doubles at stride ld.
PTZ_HD bool ptzh_fit_dlt(const float* src, const float* dst, const int* idx, int m, double* ws, int ld, double* H)
{
  if (m < 4) return false;
  double cs[6];
  ptzh_normalisation(src, idx, m, cs);
  ptzh_normalisation(dst, idx, m, cs + 3);
  for (int a = 0; a < 9; ++a)
    for (int b = a; b < 9; ++b) {
      const double e = ptzh_ata_entry(a, b, src, dst, idx, m, cs);
      ws[(9 * a + b) * ld] = e;
      ws[(9 * b + a) * ld] = e;
    }
  return ptzh_dlt_solve(ws, ws + 81 * ld, ld, cs, H);
}

// The fit of one minimal sample s[0..4): the four correspondences are copied first (the same floats), so the fit reads
// registers rather than the pair's arrays.
PTZ_HD bool ptzh_fit_sample(const float* src, const float* dst, const int* s, double* ws, int ld, double* H)
{
  float a[8], b[8];
  for (int k = 0; k < 4; ++k) {
    a[2 * k] = src[2 * s[k]]; a[2 * k + 1] = src[2 * s[k] + 1];
    b[2 * k] = dst[2 * s[k]]; b[2 * k + 1] = dst[2 * s[k] + 1];
  }
  const int id[4] = {0, 1, 2, 3};
  return ptzh_fit_dlt(a, b, id, 4, ws, ld, H);
}

PTZ_HD int ptzh_count_inliers(const double* H, const float* src, const float* dst, int n, double thr2)
{
  int cnt = 0;
  for (int i = 0; i < n; ++i) cnt += ptzh_err2(H, src + 2 * i, dst + 2 * i) <= thr2;
  return cnt;
}

// The acceptance rule and the adaptive bound: bound = the host's static_cast<int>(ceil(need)) for this count (a table the
// host computes, ptzh_adaptive_bound).  Returns true if the hypothesis becomes the best one.
PTZ_HD bool ptzh_accept(int cnt, int it, int bound, int& best_inliers, int& max_iters)
{
  if (!(cnt > (best_inliers < 3 ? 3 : best_inliers))) return false;
  best_inliers = cnt;
  const int lo = it + 1 < bound ? bound : it + 1;  // std::max(it + 1, bound)
  max_iters = lo < max_iters ? lo : max_iters;     // std::min(max_iters, ...)
  return true;
}

// ---- Refine: Gauss-Newton / LM on the forward transfer error over h11..h32 ---------------------------------------------
PTZ_HD double ptzh_cost(const double* H, const float* src, const float* dst, const int* idx, int m)
{
  double c = 0;
  for (int k = 0; k < m; ++k) c += ptzh_err2(H, src + 2 * idx[k], dst + 2 * idx[k]);
  return c;
}

// ju[a], jv[a], ru, rv of correspondence i at H; a in [0, 8).
PTZ_HD void ptzh_refine_point(const double* H, const float* src, const float* dst, int i, int a, double& ja, double& va, double& ru,
                              double& rv)
{
  const double x = src[2 * i], y = src[2 * i + 1];
  const double w = H[6] * x + H[7] * y + H[8], iw = 1.0 / w;
  const double u = (H[0] * x + H[1] * y + H[2]) * iw, v = (H[3] * x + H[4] * y + H[5]) * iw;
  ja = a == 0 ? x * iw : a == 1 ? y * iw : a == 2 ? iw : a < 6 ? 0.0 : a == 6 ? -u * x * iw : -u * y * iw;
  va = a < 3 ? 0.0 : a == 3 ? x * iw : a == 4 ? y * iw : a == 5 ? iw : a == 6 ? -v * x * iw : -v * y * iw;
  ru = u - static_cast<double>(dst[2 * i]);
  rv = v - static_cast<double>(dst[2 * i + 1]);
}

// JtJ[8 a + b] (symmetric in a, b bit for bit) over idx[0..m)
PTZ_HD double ptzh_jtj_entry(int a, int b, const double* H, const float* src, const float* dst, const int* idx, int m)
{
  double acc = 0.0;
  for (int k = 0; k < m; ++k) {
    double ja, va, jb, vb, ru, rv;
    ptzh_refine_point(H, src, dst, idx[k], a, ja, va, ru, rv);
    ptzh_refine_point(H, src, dst, idx[k], b, jb, vb, ru, rv);
    acc += ja * jb + va * vb;
  }
  return acc;
}
PTZ_HD double ptzh_jtr_entry(int a, const double* H, const float* src, const float* dst, const int* idx, int m)
{
  double acc = 0.0;
  for (int k = 0; k < m; ++k) {
    double ja, va, ru, rv;
    ptzh_refine_point(H, src, dst, idx[k], a, ja, va, ru, rv);
    acc += ja * ru + va * rv;
  }
  return acc;
}

// SolveLeastSquares(8, 8, A, b) with rcond 1e-12: A (64 entries, stride ld) is overwritten, W is 64 more entries.
PTZ_HD void ptzh_solve8(double* A, double* W, int ld, const double* b, double* x)
{
  double norm[8];
  int order[8];
  ptzh_jacobi<8>(A, W, ld, norm, order);
  for (int i = 0; i < 8; ++i) x[i] = 0.0;
  const double s0 = norm[order[0]];
  for (int j = 0; j < 8; ++j) {
    const int o = order[j];
    const double sj = norm[o];
    if (!(sj > 1e-12 * s0)) continue;  // taken only with norm[o] > 0, where U(:, j) = (A V)(:, o) / norm[o]
    double ub = 0;
    for (int i = 0; i < 8; ++i) ub += (A[(i * 8 + o) * ld] / sj) * b[i];
    ub /= sj;
    for (int i = 0; i < 8; ++i) x[i] += W[(i * 8 + o) * ld] * ub;
  }
}

// The state of Refine between its parallel parts (JtJ / Jtr accumulation) and its serial parts (the damped solves).
struct PtzhRefine {
  double cur, lambda;
  int it;
};
PTZ_HD void ptzh_refine_begin(PtzhRefine& r, const double* H, const float* src, const float* dst, const int* idx, int m)
{
  r.cur = ptzh_cost(H, src, dst, idx, m);
  r.lambda = 1e-6;
  r.it = 0;
}
// One outer step after JtJ (64) and Jtr (8) are accumulated: up to six damping attempts.  Returns true if Refine goes on
// with another outer step.  ws: 128 doubles at stride ld.
PTZ_HD bool ptzh_refine_step(PtzhRefine& r, double* H, const double* JtJ, const double* Jtr, const float* src, const float* dst,
                             const int* idx, int m, double* ws, int ld)
{
  bool improved = false;
  for (int attempt = 0; attempt < 6 && !improved; ++attempt) {
    double b[8], d[8];
    for (int k = 0; k < 64; ++k) ws[k * ld] = JtJ[k];
    for (int a = 0; a < 8; ++a) { ws[(8 * a + a) * ld] *= 1.0 + r.lambda; b[a] = -Jtr[a]; }
    ptzh_solve8(ws, ws + 64 * ld, ld, b, d);
    double Hn[9];
    for (int k = 0; k < 9; ++k) Hn[k] = H[k];
    for (int a = 0; a < 8; ++a) Hn[a] += d[a];
    const double c = ptzh_cost(Hn, src, dst, idx, m);
    if (c < r.cur) {
      const bool tiny = r.cur - c <= 1e-12 * r.cur;
      for (int k = 0; k < 9; ++k) H[k] = Hn[k];
      r.cur = c;
      const double l = r.lambda * 0.1;
      r.lambda = l < 1e-12 ? 1e-12 : l;  // std::max(lambda * 0.1, 1e-12)
      improved = true;
      if (tiny) return false;
    }
    else r.lambda *= 10;
  }
  if (!improved) return false;
  return ++r.it < 10;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- host only --------------------------------------------------------------------------------------------------------
// The adaptive bound of FindHomographyRansac for `cnt` inliers of n: the same expression, evaluated with the host's libm.
// Where ceil(need) does not fit an int the host's static_cast gives x86's INT_MIN (max_iters then becomes it + 1): that
// conversion is written out here, defined, with the same result.
inline int32_t ptzh_adaptive_bound(int cnt, int n)
{
  const double confidence = 0.995;
  const double ep = 1.0 - static_cast<double>(cnt) / n;
  const double denom = std::log(std::max(1.0 - std::pow(1.0 - ep, 4), 1e-300));
  const double need = (denom >= 0 || ep <= 0) ? 0 : std::log(1.0 - confidence) / denom;
  const double c = std::ceil(need);
  return (c > -2147483649.0 && c < 2147483648.0) ? static_cast<int32_t>(c) : INT32_MIN;
}

// The whole estimator in the host's sequence (the harness instantiation).  bound[cnt] = ptzh_adaptive_bound(cnt, n) for
// cnt in [0, n]; inl: n ints of workspace.  Returns 1 and fills H (and mask[n] if non-NULL), or 0 with both untouched.
inline int ptzh_find_homography_seq(int n, const float* src, const float* dst, double thresh, const int32_t* bound, int* inl,
                                    double* H_out, uint8_t* mask)
{
  if (n < 4) return 0;
  const double thr2 = thresh * thresh;
  double ws[162];
  double best[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  int best_inliers = 0;
  if (n == 4) {
    const int all[4] = {0, 1, 2, 3};
    if (!ptzh_fit_dlt(src, dst, all, 4, ws, 1, best)) return 0;
    best_inliers = 4;
  }
  else {
    uint64_t rng = PTZH_SEED;
    int max_iters = PTZH_MAX_ITERS;
    for (int it = 0; it < max_iters; ++it) {
      int s[4];
      if (!ptzh_draw_sample(rng, n, src, dst, s)) continue;
      double Hs[9];
      if (!ptzh_fit_sample(src, dst, s, ws, 1, Hs)) continue;
      const int cnt = ptzh_count_inliers(Hs, src, dst, n, thr2);
      if (ptzh_accept(cnt, it, bound[cnt], best_inliers, max_iters))
        for (int k = 0; k < 9; ++k) best[k] = Hs[k];
    }
    if (best_inliers < 4) return 0;
  }
  int m = 0;
  for (int i = 0; i < n; ++i)
    if (ptzh_err2(best, src + 2 * i, dst + 2 * i) <= thr2) inl[m++] = i;
  if (m < 4) return 0;
  double H[9];
  if (ptzh_fit_dlt(src, dst, inl, m, ws, 1, H)) {
    PtzhRefine r;
    ptzh_refine_begin(r, H, src, dst, inl, m);
    for (;;) {
      double JtJ[64], Jtr[8];
      for (int a = 0; a < 8; ++a) {
        for (int b = a; b < 8; ++b) JtJ[8 * a + b] = JtJ[8 * b + a] = ptzh_jtj_entry(a, b, H, src, dst, inl, m);
        Jtr[a] = ptzh_jtr_entry(a, H, src, dst, inl, m);
      }
      if (!ptzh_refine_step(r, H, JtJ, Jtr, src, dst, inl, m, ws, 1)) break;
    }
  }
  else
    for (int k = 0; k < 9; ++k) H[k] = best[k];
  const double inv = 1.0 / H[8];
  for (int k = 0; k < 9; ++k) H[k] *= inv;
  if (mask)
    for (int i = 0; i < n; ++i) mask[i] = ptzh_err2(H, src + 2 * i, dst + 2 * i) <= thr2;
  for (int k = 0; k < 9; ++k) H_out[k] = H[k];
  return 1;
}
#endif

}  // namespace ptz
