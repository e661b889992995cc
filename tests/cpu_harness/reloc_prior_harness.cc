// reloc_prior_harness.cc -- TEST INFRASTRUCTURE.  Host instantiation of ptz-calib_amd/csrc/ptz_reloc_prior.h in the order the
// kernels of ptz_reloc_prior.hip use it: the scores of a query over all references, the list by counting in ascending index, the H of
// every listed slot, the prior's part of the initial camera -- so that it can be held to the numpy restatement
// (tests/reloc_prior_util.py) without a GPU and the device to it.  Never part of the product library.
// Build: g++ -O2 -ffp-contract=off -shared -fPIC -o libreloc_prior_harness.so reloc_prior_harness.cc
#include <stdint.h>

#include "../../ptz-calib_amd/csrc/ptz_reloc_prior.h"

using namespace ptz;

extern "C" {

void h_prior_homography(const double* cam_from, const double* R_from, const double* cam_to, const double* R_to, double* H)
{
  prior_homography(cam_from, R_from, cam_to, R_to, H);
}

void h_prior_query_K(const double* prior, int32_t w, int32_t h, int32_t factor_type, double* K4) { prior_query_K(prior, w, h, factor_type, K4); }

// the outputs as ptz_reloc_prior_pairs has them
void h_reloc_prior(int32_t n_ref, const double* ref_cams, const double* ref_R, int32_t n_query, const double* prior_cams, const double* prior_R,
                   const int32_t* query_wh, int32_t factor_type, int32_t R, int32_t min_overlap, int32_t* shortlist, int32_t* n_short,
                   int32_t* overlap, double* H_slot)
{
  for (int64_t q = 0; q < n_query; ++q) {
    double Kq[4], H[9];
    const int32_t w = query_wh[2 * q], h = query_wh[2 * q + 1];
    prior_query_K(prior_cams + 15 * q, w, h, factor_type, Kq);
    int32_t* v = overlap + q * n_ref;
    for (int64_t r = 0; r < n_ref; ++r) v[r] = prior_overlap(ref_cams + 15 * r, ref_R + 9 * r, Kq, prior_R + 9 * q, w, h, H);
    int32_t taken = 0;
    for (int32_t r = 0; r < n_ref; ++r) {
      if (!prior_takes(v, n_ref, r, R, min_overlap)) continue;
      shortlist[R * q + taken] = r;
      prior_homography(ref_cams + 15 * (int64_t)r, ref_R + 9 * (int64_t)r, Kq, prior_R + 9 * q, H_slot + 9 * (R * q + taken));
      ++taken;
    }
    for (int32_t s = taken; s < R; ++s) {
      shortlist[R * q + s] = -1;
      for (int k = 0; k < 9; ++k) H_slot[9 * (R * q + s) + k] = 0.0;
    }
    n_short[q] = taken;
  }
}

void h_reloc_prior_camera(int32_t n_query, double* cam_cur, const double* prior_cams, int32_t factor_type)
{
  for (int64_t q = 0; q < n_query; ++q) reloc_prior_camera(cam_cur + 15 * q, prior_cams + 15 * q, factor_type);
}
}
