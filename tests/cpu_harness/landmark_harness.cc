// landmark_harness.cc -- TEST INFRASTRUCTURE.  Host instantiation of ptz-calib_amd/csrc/ptz_landmark.h in the order the kernels of
// ptz_landmark.hip use it: per track the views in CSR order (validity, ray, the sum left to right), the byte sums, the home search;
// per query the integer votes, the arg-max on (count, -index), the transfer and keep rule per match -- so that it can be held to
// the numpy restatement (tests/landmark_util.py) without a GPU and the device to it.  Never part of the product library.
// Build: g++ -O2 -ffp-contract=off -shared -fPIC -o liblandmark_harness.so landmark_harness.cc
#include <stdint.h>

#include <vector>

#include "../../ptz-calib_amd/csrc/ptz_landmark.h"

using namespace ptz;

namespace {

// view v of the CSR: valid or not, its reference and its feature's row in the raw arrays
bool view_of(int32_t n_ref, const int64_t* feat_ptr, const float* kp, const double* ref_cams, const double* ref_R, const int32_t* trk_img,
             const int32_t* trk_feat, int dist, int64_t v, int32_t* r, int64_t* row, double* ray)
{
  *r = trk_img[v];
  if (*r < 0 || *r >= n_ref) return false;
  const int32_t f = trk_feat[v];
  if (f < 0 || f >= feat_ptr[*r + 1] - feat_ptr[*r]) return false;
  *row = feat_ptr[*r] + f;
  return landmark_view_ray(ref_cams + 15 * (int64_t)*r, ref_R + 9 * (int64_t)*r, dist, kp[2 * *row], kp[2 * *row + 1], ray);
}

}  // namespace

extern "C" {

// the map build; outputs sized for n_track landmarks.  Returns n_lm.
int32_t h_landmark_build(int32_t n_ref, const int64_t* feat_ptr, const uint8_t* desc, int32_t D, const float* kp, const double* ref_cams,
                         const double* ref_R, int32_t n_track, const int64_t* trk_ptr, const int32_t* trk_img, const int32_t* trk_feat,
                         int32_t dist, int32_t min_views, int32_t* lm_track, double* lm_ray, int32_t* lm_home, int32_t* lm_views,
                         uint8_t* lm_desc)
{
  int32_t n_lm = 0;
  std::vector<int32_t> S((size_t)D);
  for (int32_t t = 0; t < n_track; ++t) {
    double s[3] = {0.0, 0.0, 0.0}, ray[3], L[3];
    int32_t n = 0, r;
    int64_t row;
    for (int k = 0; k < D; ++k) S[k] = 0;
    for (int64_t v = trk_ptr[t]; v < trk_ptr[t + 1]; ++v) {
      if (!view_of(n_ref, feat_ptr, kp, ref_cams, ref_R, trk_img, trk_feat, dist, v, &r, &row, ray)) continue;
      s[0] = s[0] + ray[0]; s[1] = s[1] + ray[1]; s[2] = s[2] + ray[2];
      for (int k = 0; k < D; ++k) S[k] += desc[row * D + k];
      ++n;
    }
    if (n < min_views || n < 1 || !landmark_unit(s, L)) continue;
    double best = -__builtin_huge_val();
    int32_t home = -1, first = -1;
    for (int64_t v = trk_ptr[t]; v < trk_ptr[t + 1]; ++v) {
      if (!view_of(n_ref, feat_ptr, kp, ref_cams, ref_R, trk_img, trk_feat, dist, v, &r, &row, ray)) continue;
      if (first < 0) first = r;
      const double z = landmark_home_z(ref_R + 9 * (int64_t)r, L);
      if (z > best) { best = z; home = r; }
    }
    lm_track[n_lm] = t;
    lm_ray[3 * (int64_t)n_lm] = L[0]; lm_ray[3 * (int64_t)n_lm + 1] = L[1]; lm_ray[3 * (int64_t)n_lm + 2] = L[2];
    lm_home[n_lm] = home >= 0 ? home : first;
    lm_views[n_lm] = n;
    for (int k = 0; k < D; ++k) lm_desc[(int64_t)n_lm * D + k] = landmark_desc_byte(S[k], n);
    ++n_lm;
  }
  return n_lm;
}

// the assembly; the outputs as ptz_landmark_assemble has them.  Returns the kept matches.
int64_t h_landmark_assemble(int32_t n_query, int32_t n_ref, int32_t n_lm, const int64_t* match_ptr, const int32_t* idx_a, const float* uv_b,
                            const double* lm_ray, const int32_t* lm_home, const double* ref_cams, const double* ref_R,
                            const int32_t* query_wh, int32_t* anchor_ref, int64_t* out_ptr, float* out_uv_ref, float* out_uv_cur,
                            int32_t* out_src, double* cam_ref, double* cam_cur)
{
  std::vector<int32_t> votes((size_t)n_ref);
  int64_t o = 0;
  out_ptr[0] = 0;
  for (int q = 0; q < n_query; ++q) {
    for (int r = 0; r < n_ref; ++r) votes[r] = 0;
    for (int64_t i = match_ptr[q]; i < match_ptr[q + 1]; ++i) {
      const int32_t r = landmark_vote(idx_a, lm_home, n_lm, n_ref, i);
      if (r >= 0) ++votes[r];
    }
    uint64_t best = 0;
    for (int r = 0; r < n_ref; ++r) {
      const uint64_t key = landmark_anchor_key(votes[r], r);
      if (key > best) best = key;
    }
    const int32_t a = best ? reloc_key_pos(best) : -1;
    anchor_ref[q] = a;
    const int32_t ra = a >= 0 ? a : 0;
    reloc_cameras(ref_cams + 15 * (int64_t)ra, query_wh[2 * q], query_wh[2 * q + 1], 2, cam_ref + 15 * (int64_t)q, cam_cur + 15 * (int64_t)q);
    if (a >= 0)
      for (int64_t i = match_ptr[q]; i < match_ptr[q + 1]; ++i) {
        if (landmark_vote(idx_a, lm_home, n_lm, n_ref, i) < 0) continue;
        const RelocPixel px = landmark_transfer(ref_R + 9 * (int64_t)a, ref_cams[15 * (int64_t)a], lm_ray + 3 * (int64_t)idx_a[i]);
        if (!px.keep) continue;
        out_uv_ref[2 * o] = px.u; out_uv_ref[2 * o + 1] = px.v;
        out_uv_cur[2 * o] = uv_b[2 * i]; out_uv_cur[2 * o + 1] = uv_b[2 * i + 1];
        out_src[o] = (int32_t)i;
        ++o;
      }
    out_ptr[q + 1] = o;
  }
  return o;
}
}
