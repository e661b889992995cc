// rotfocal_harness.cc -- TEST INFRASTRUCTURE.  Host instantiation of ptz-calib_amd/csrc/ptz_rotfocal.h: the estimator in sequence, one
// query or a CSR of queries with the outputs ptz_rotfocal_gate_run leaves, so that it can be held to the numpy restatement
// (tests/rotfocal_util.py) without a GPU and the device to it.  Never part of the product library.
// Build: g++ -O2 -ffp-contract=off -shared -fPIC -o librotfocal_harness.so rotfocal_harness.cc
// Stand-alone, for the sanitizers: g++ -O1 -g -ffp-contract=off -fsanitize=address,undefined -DROTFOCAL_HARNESS_MAIN -o rotfocal_harness_main rotfocal_harness.cc
#include <stdint.h>

#include "../../ptz-calib_amd/csrc/ptz_rotfocal.h"

using namespace ptz;

extern "C" {

void h_rotfocal_sample(int32_t it, int32_t n, int32_t* ij) { int i, j; ptzrf_sample(it, n, i, j); ij[0] = i; ij[1] = j; }

int32_t h_rotfocal_hypothesis(int32_t h, int32_t n, const float* uv_a, const float* uv_b, const double* cam_a, double cxq, double cyq, double* model)
{
  return ptzrf_hypothesis_of(h, n, uv_a, uv_b, cam_a, cxq, cyq, model) ? 1 : 0;
}

int32_t h_rotfocal_find(int32_t n, const float* uv_a, const float* uv_b, const double* cam_a, double cxq, double cyq, double thresh, int32_t iters,
                        double* model, double* H, uint8_t* mask, int32_t* best_count)
{
  return ptzrf_find_seq(n, uv_a, uv_b, cam_a, cxq, cyq, thresh, iters, model, H, mask, best_count);
}

// the inlier test of n matches under a GIVEN model [f, R]: mask [n]
void h_rotfocal_inliers(const double* model, int32_t n, const float* uv_a, const float* uv_b, const double* cam_a, double cxq, double cyq, double thresh,
                        uint8_t* mask)
{
  const double thr2 = thresh * thresh;
  for (int64_t i = 0; i < n; ++i) {
    double l[4];
    ptzrf_lift(cam_a, cxq, cyq, uv_a + 2 * i, uv_b + 2 * i, l);
    mask[i] = ptzrf_inlier(model, l[0], l[1], l[2], l[3], thr2) ? 1 : 0;
  }
}

// a batch: query p owns the matches [match_ptr[p], match_ptr[p + 1]), cam_ref / cam_cur are [n_pair, 15]
void h_rotfocal_batch(int32_t n_pair, const int64_t* match_ptr, const float* uv_a, const float* uv_b, const double* cam_ref, const double* cam_cur,
                      double thresh, int32_t iters, double* model, double* H, int32_t* found, uint8_t* mask, int32_t* best_count)
{
  for (int64_t p = 0; p < n_pair; ++p) {
    const int64_t a = match_ptr[p];
    found[p] = ptzrf_find_seq(static_cast<int>(match_ptr[p + 1] - a), uv_a + 2 * a, uv_b + 2 * a, cam_ref + 15 * p, cam_cur[15 * p + 2],
                              cam_cur[15 * p + 3], thresh, iters, model + 10 * p, H + 9 * p, mask + a, best_count + p);
  }
}
}

#if defined(ROTFOCAL_HARNESS_MAIN)
#include <cstdio>
#include <vector>

namespace {

uint64_t g_rng = 0x1234567ull;
double uni() { return static_cast<double>(ptzh_next(g_rng) >> 11) * (1.0 / 9007199254740992.0); }

int g_bad = 0, g_runs = 0, g_found = 0;

// every output of a query flagged valid is finite (H may be nine NaN as a whole: the documented "no admissible candidate")
void run(const std::vector<float>& a, const std::vector<float>& b, const double* cam, double cxq, double cyq, int iters)
{
  const int n = static_cast<int>(a.size() / 2);
  std::vector<uint8_t> mask(n + 1, 7);
  double model[10], H[9];
  int32_t best = 0;
  const int32_t found = ptzrf_find_seq(n, a.data(), b.data(), cam, cxq, cyq, 4.0, iters, model, H, mask.data(), &best);
  ++g_runs;
  if (mask[n] != 7) ++g_bad;
  if (!found) return;
  ++g_found;
  int ones = 0, nan_h = 0;
  for (int k = 0; k < 10; ++k) g_bad += ptzrf_finite(model[k]) ? 0 : 1;
  for (int k = 0; k < 9; ++k) nan_h += ptzrf_finite(H[k]) ? 0 : 1;
  if (nan_h != 0 && nan_h != 9) ++g_bad;
  for (int i = 0; i < n; ++i) { if (mask[i] > 1) ++g_bad; ones += mask[i]; }
  if (ones != best || best < 3) ++g_bad;
}

// n matches of a rotation (pan, tilt) and focal 2500 between the anchor cam and a 1920 x 1080 query, a share of them wrong
void synth(int n, const double* cam, double wrong, std::vector<float>& a, std::vector<float>& b)
{
  a.resize(2 * n); b.resize(2 * n);
  const double f = 2500.0, c = 0.9950041652780258, s = 0.09983341664682815;  // a pan of 0.1 rad
  for (int i = 0; i < n; ++i) {
    const double u = uni() * 1920.0, v = uni() * 1080.0;
    const double x = (u - 960.0) / f, y = (v - 540.0) / f;
    const double rx = c * x + s, rz = -s * x + c;  // the query pixel's ray in the anchor's frame
    a[2 * i] = static_cast<float>(cam[0] * rx / rz + cam[2]);
    a[2 * i + 1] = static_cast<float>(cam[1] * y / rz + cam[3]);
    const bool w = uni() < wrong;
    b[2 * i] = static_cast<float>(w ? uni() * 1920.0 : u);
    b[2 * i + 1] = static_cast<float>(w ? uni() * 1080.0 : v);
  }
}

}  // namespace

int main()
{
  const double virt[15] = {1500.0, 1500.0, 8192.0, 8192.0}, real[15] = {2200.0, 2210.0, 960.0, 540.0};
  const int sizes[] = {0, 1, 2, 3, 4, 5, 63, 64, 65, 257, 2049, 5000}, its[] = {1, 2, 128, 129};
  std::vector<float> a, b;
  for (const double* cam : {virt, real})
    for (int n : sizes)
      for (int it : its) {
        synth(n, cam, 0.3, a, b);
        run(a, b, cam, 960.0, 540.0, it);
      }
  // the degenerate inputs
  for (const double* cam : {virt, real}) {
    synth(64, cam, 0.0, a, b);
    std::vector<float> a1 = a, b1 = b;
    for (int i = 0; i < 64; ++i) { a1[2 * i] = a[0]; a1[2 * i + 1] = a[1]; b1[2 * i] = b[0]; b1[2 * i + 1] = b[1]; }
    run(a1, b1, cam, 960.0, 540.0, 128);  // all matches the same pixel
    run(std::vector<float>(a1.begin(), a1.begin() + 4), std::vector<float>(b1.begin(), b1.begin() + 4), cam, 960.0, 540.0, 128);  // two identical
    a1 = a; b1 = b;
    for (int i = 0; i < 64; ++i) { b1[2 * i] = b[0]; b1[2 * i + 1] = b[1]; }
    run(a1, b1, cam, 960.0, 540.0, 128);  // q_i = q_j
    a1 = a; b1 = b;
    for (int i = 0; i < 64; ++i) { a1[2 * i] = a[0]; a1[2 * i + 1] = a[1]; }
    run(a1, b1, cam, 960.0, 540.0, 128);  // parallel rays
    a1 = a; b1 = b;
    a1[6] = NAN; b1[21] = INFINITY; a1[40] = -INFINITY;
    run(a1, b1, cam, 960.0, 540.0, 128);  // NaN and infinite pixels
    a1 = a; b1 = b;
    for (int i = 0; i < 64; ++i) { a1[2 * i] = static_cast<float>(cam[2] + 1e7 * (uni() - 0.5)); }
    run(a1, b1, cam, 960.0, 540.0, 128);  // rays near the anchor's image plane: m_z <= 0 for many
  }
  printf("%d runs, %d found, %d mismatches\n", g_runs, g_found, g_bad);
  return g_bad == 0 && g_found > 0 ? 0 : 1;
}
#endif
