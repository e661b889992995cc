// ptz_rotfocal.h -- the contract of the rotation-and-focal match gate (ptz_rotfocal_gate_run_device, ptz_rotfocal.hip): a fixed-count
// RANSAC over two-match samples for the model an ASSEMBLED relocalization query obeys.  uv_a of such a query is a pixel of a pinhole at
// the rig's shared centre (the anchor, or the virtual anchor [fa, fa, S, S] of the K > 1 and landmark assemblies), uv_b a query pixel, so
// the two are related by K_q R K_a^-1 with K_a known and the query's centre known: four unknowns, f and R, which two matches fix in
// closed form.  The query's distortion and fx != fy do not enter; the threshold absorbs them, as it does for the homography gate.
//
// One header for host and device, in the manner of ptz_homography.h and ptz_reloc_prior.h: doubles, + - * / sqrt only, every product
// and sum rounded on its own, no floating-point sum ever split over lanes.  A host build (tests/cpu_harness/rotfocal_harness.cc) gives
// the device's bits and numpy restates it (tests/rotfocal_util.py).
//
// One query: n matches, uv_a / uv_b interleaved float pairs, cam_a [fx, fy, cx, cy, ..] (only these four are read), (cxq, cyq).
//   lift        a = ((u_a - cx) / fx, (v_a - cy) / fy, 1), not normalised;  q = (u_b - cxq, v_b - cyq);  doubles from the floats
//   sample it   a generator of its own, state PTZH_SEED + (it + 1) * 0xD1342543DE82EF95 (wrapping): i = below(n), j = below(n - 1),
//               ++j if j >= i.  No redraw.  Depends on it and n only -- not on the query's place in a batch, not on the launch shape.
//   focal       A = |a_i|^2 |a_j|^2, X = |a_i x a_j|^2, n1 = |q_i|^2, n2 = |q_j|^2, e = |q_i - q_j|^2, k = (q_ix q_jy - q_iy q_jx)^2;
//               F = f^2 solves X F^2 + (X (n1 + n2) - A e) F + (X (n1 n2) - A k) = 0: sin^2 of the ray angle = sin^2 of the pixel-ray
//               angle, no coefficient of which cancels at small angles.  t = -0.5 (b + sign(b) sqrt(disc)), sign(0) = +1; root 0 = t / X,
//               root 1 = c / t.  No hypothesis unless X > 0, disc >= 0, t != 0.  A root is used iff finite, > 0 and
//               (q_i . q_j + F)(a_i . a_j) > 0.  Hypothesis number = 2 it + root.
//   rotation    triads: e1 = a_i / |a_i|, e3 = (a_i x a_j) / |a_i x a_j|, e2 = e3 x e1; g1, g2, g3 likewise of b = (q_x, q_y, f);
//               R = g1 e1^T + g2 e2^T + g3 e3^T, each entry summed left to right.  A non-finite entry drops the hypothesis.
//   inlier      m = R a, rows summed left to right; m_z > 0 and ((f m_x) / m_z - q_x)^2 + ((f m_y) / m_z - q_y)^2 <= thresh^2 (NaN: no).
//   selection   most inliers, ties to the lowest hypothesis number; found = (n >= 2 and best count >= 3); mask = the test under it.
//   model       [f, R row-major]; H = K_q R K_a^-1 with both matrices written out as in prior_homography (ptz_reloc_prior.h), divided by
//               its last entry; nine NaN where that entry's magnitude is not above 1e-300.
#pragma once

#include <math.h>
#include <stdint.h>

#include "ptz_homography.h"  // PTZ_HD, PTZH_SEED, ptzh_next / ptzh_below

#if defined(__clang__)
#pragma clang fp contract(off)  // every product and sum rounds on its own
#endif

namespace ptz {

constexpr int PTZRF_MAX_ITERS = 4096;       // iters of a run: 1 .. this
constexpr int PTZRF_DEFAULT_ITERS = 128;
constexpr int PTZRF_MIN_COUNT = 3;          // a model needs one inlier besides its two sample matches

PTZ_HD bool ptzrf_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }  // false for NaN and the infinities

// the two matches of iteration `it`; n >= 2
PTZ_HD void ptzrf_sample(int it, int n, int& i, int& j)
{
  uint64_t s = PTZH_SEED + (static_cast<uint64_t>(it) + 1ull) * 0xD1342543DE82EF95ull;
  i = ptzh_below(s, n);
  j = ptzh_below(s, n - 1);
  if (j >= i) ++j;
}

// one match lifted: l = (a_x, a_y, q_x, q_y); a_z = 1
PTZ_HD void ptzrf_lift(const double* cam_a, double cxq, double cyq, const float* ua, const float* ub, double* l)
{
  l[0] = (static_cast<double>(ua[0]) - cam_a[2]) / cam_a[0];
  l[1] = (static_cast<double>(ua[1]) - cam_a[3]) / cam_a[1];
  l[2] = static_cast<double>(ub[0]) - cxq;
  l[3] = static_cast<double>(ub[1]) - cyq;
}

// rows e1, e2, e3 of the triad of (v, w): E[0..2] = v / |v|, E[6..8] = (v x w) / |v x w|, E[3..5] = e3 x e1
PTZ_HD void ptzrf_triad(const double* v, const double* w, double* E)
{
  const double nv = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  E[0] = v[0] / nv; E[1] = v[1] / nv; E[2] = v[2] / nv;
  const double c0 = v[1] * w[2] - v[2] * w[1], c1 = v[2] * w[0] - v[0] * w[2], c2 = v[0] * w[1] - v[1] * w[0];
  const double nc = sqrt(c0 * c0 + c1 * c1 + c2 * c2);
  E[6] = c0 / nc; E[7] = c1 / nc; E[8] = c2 / nc;
  E[3] = E[7] * E[2] - E[8] * E[1];
  E[4] = E[8] * E[0] - E[6] * E[2];
  E[5] = E[6] * E[1] - E[7] * E[0];
}

// hypothesis `root` (0, 1) of the sample (li, lj) of lifted matches: model = [f, R]; false = no hypothesis
PTZ_HD bool ptzrf_hypothesis(const double* li, const double* lj, int root, double* model)
{
  const double ai[3] = {li[0], li[1], 1.0}, aj[3] = {lj[0], lj[1], 1.0};
  const double nai = ai[0] * ai[0] + ai[1] * ai[1] + ai[2] * ai[2], naj = aj[0] * aj[0] + aj[1] * aj[1] + aj[2] * aj[2];
  const double A = nai * naj;
  const double c0 = ai[1] * aj[2] - ai[2] * aj[1], c1 = ai[2] * aj[0] - ai[0] * aj[2], c2 = ai[0] * aj[1] - ai[1] * aj[0];
  const double X = c0 * c0 + c1 * c1 + c2 * c2;
  const double n1 = li[2] * li[2] + li[3] * li[3], n2 = lj[2] * lj[2] + lj[3] * lj[3];
  const double dx = li[2] - lj[2], dy = li[3] - lj[3];
  const double e = dx * dx + dy * dy;
  const double kk = li[2] * lj[3] - li[3] * lj[2];
  const double k = kk * kk;
  const double b = X * (n1 + n2) - A * e;
  const double c = X * (n1 * n2) - A * k;
  const double disc = b * b - (4.0 * X) * c;
  if (!(X > 0.0) || !(disc >= 0.0)) return false;
  const double sq = sqrt(disc);
  const double t = -0.5 * (b + (b >= 0.0 ? sq : -sq));
  if (!(t != 0.0)) return false;
  const double F = root == 0 ? t / X : c / t;
  const double dq = li[2] * lj[2] + li[3] * lj[3];
  const double da = ai[0] * aj[0] + ai[1] * aj[1] + ai[2] * aj[2];
  if (!ptzrf_finite(F) || !(F > 0.0) || !((dq + F) * da > 0.0)) return false;
  const double f = sqrt(F);
  const double bi[3] = {li[2], li[3], f}, bj[3] = {lj[2], lj[3], f};
  double E[9], G[9];
  ptzrf_triad(ai, aj, E);
  ptzrf_triad(bi, bj, G);
  model[0] = f;
  bool ok = ptzrf_finite(f);
  for (int r = 0; r < 3; ++r)
    for (int cc = 0; cc < 3; ++cc) {
      const double v = G[r] * E[cc] + G[3 + r] * E[3 + cc] + G[6 + r] * E[6 + cc];
      model[1 + 3 * r + cc] = v;
      ok = ok && ptzrf_finite(v);
    }
  return ok;
}

// the inlier test of a lifted match under model = [f, R]
PTZ_HD bool ptzrf_inlier(const double* model, double ax, double ay, double qx, double qy, double thr2)
{
  const double mx = model[1] * ax + model[2] * ay + model[3];
  const double my = model[4] * ax + model[5] * ay + model[6];
  const double mz = model[7] * ax + model[8] * ay + model[9];
  const double ex = (model[0] * mx) / mz - qx;
  const double ey = (model[0] * my) / mz - qy;
  return mz > 0.0 && ex * ex + ey * ey <= thr2;
}

// H = K_q R K_a^-1 / (its last entry), K_q = [f, f, cxq, cyq]
PTZ_HD void ptzrf_homography(const double* model, const double* cam_a, double cxq, double cyq, double* H)
{
  const double f = model[0];
  const double* R = model + 1;
  double N[9];
  for (int i = 0; i < 3; ++i) {
    N[3 * i] = R[3 * i] / cam_a[0];
    N[3 * i + 1] = R[3 * i + 1] / cam_a[1];
    N[3 * i + 2] = (R[3 * i + 2] - N[3 * i] * cam_a[2]) - N[3 * i + 1] * cam_a[3];
  }
  double G[9];
  for (int j = 0; j < 3; ++j) {
    G[j] = f * N[j] + cxq * N[6 + j];
    G[3 + j] = f * N[3 + j] + cyq * N[6 + j];
    G[6 + j] = N[6 + j];
  }
  const bool ok = fabs(G[8]) > 1e-300;
  for (int k = 0; k < 9; ++k) H[k] = ok ? G[k] / G[8] : NAN;
}

// hypothesis number h of a query: the sample of iteration h / 2, lifted, root h % 2
PTZ_HD bool ptzrf_hypothesis_of(int h, int n, const float* uv_a, const float* uv_b, const double* cam_a, double cxq, double cyq, double* model)
{
  int i, j;
  ptzrf_sample(h >> 1, n, i, j);
  double li[4], lj[4];
  ptzrf_lift(cam_a, cxq, cyq, uv_a + 2 * (int64_t)i, uv_b + 2 * (int64_t)i, li);
  ptzrf_lift(cam_a, cxq, cyq, uv_a + 2 * (int64_t)j, uv_b + 2 * (int64_t)j, lj);
  return ptzrf_hypothesis(li, lj, h & 1, model);
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The whole estimator in sequence (host only).  model [10], H [9] (nullable) and mask [n] (nullable) are written only when the
// return value -- found -- is 1; *best_count (nullable) is the winner's inlier count, -1 when no sample gave a hypothesis.
inline int32_t ptzrf_find_seq(int n, const float* uv_a, const float* uv_b, const double* cam_a, double cxq, double cyq, double thresh, int iters,
                              double* model, double* H, uint8_t* mask, int32_t* best_count)
{
  if (best_count) *best_count = -1;
  if (n < 2) return 0;
  const double thr2 = thresh * thresh;
  int best = -1, best_h = -1;
  double m[10], l[4];
  for (int h = 0; h < 2 * iters; ++h) {
    if (!ptzrf_hypothesis_of(h, n, uv_a, uv_b, cam_a, cxq, cyq, m)) continue;
    int c = 0;
    for (int i = 0; i < n; ++i) {
      ptzrf_lift(cam_a, cxq, cyq, uv_a + 2 * (int64_t)i, uv_b + 2 * (int64_t)i, l);
      c += ptzrf_inlier(m, l[0], l[1], l[2], l[3], thr2) ? 1 : 0;
    }
    if (c > best) { best = c; best_h = h; }
  }
  if (best_count) *best_count = best;
  if (best < PTZRF_MIN_COUNT) return 0;
  (void)ptzrf_hypothesis_of(best_h, n, uv_a, uv_b, cam_a, cxq, cyq, m);
  for (int k = 0; k < 10; ++k) model[k] = m[k];
  if (H) ptzrf_homography(m, cam_a, cxq, cyq, H);
  if (mask)
    for (int i = 0; i < n; ++i) {
      ptzrf_lift(cam_a, cxq, cyq, uv_a + 2 * (int64_t)i, uv_b + 2 * (int64_t)i, l);
      mask[i] = ptzrf_inlier(m, l[0], l[1], l[2], l[3], thr2) ? 1 : 0;
    }
  return 1;
}
#endif

}  // namespace ptz
