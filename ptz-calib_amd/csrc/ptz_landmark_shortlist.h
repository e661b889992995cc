// ptz_landmark_shortlist.h -- the contract of the landmark shortlist (ptz_landmark_shortlist.hip): a few probe features of a query
// vote for cells of the landmark map, and only the landmarks of the cells with the most votes are matched.  One header for host and
// device, all integer, built on ptz_desc_shortlist.h, whose rules it reuses and does not restate.  A host build
// (tests/cpu_harness/landmark_shortlist_harness.cc) gives the device's arrays and numpy restates them (tests/landmark_shortlist_util.py).
//
// HOME SET.  Every landmark has a home, the reference whose optical axis is nearest its ray (ptz_landmark.h): a cell of the view
//   sphere.  The map's landmarks are grouped by home: image r of the home set holds the landmarks with home == r in ASCENDING
//   landmark index, home_ptr [n_ref + 1] and home_lm [n_lm] give the grouping (a counting sort, which is stable).  A reference that
//   is home of nothing is an empty image.
// VOTES AND LISTS.  ptz_desc_shortlist.h with "reference" read as "home image": the probes of sl_probe_feature, a probe votes for
//   home r when its top-2 over the landmarks of home r passes sl_votes_for, the ranking is sl_takes, the list is written in
//   ascending home index, -1 in the unused slots.  The options are ptz_shortlist_options and the matcher's ratio and max_dist2.
// VIEW FROM HOMES.  Given shortlist [R n_query], the view of query q is every landmark whose home is on q's list, in ascending
//   landmark index -- so a tie in the matcher resolves to the lowest landmark, as in the dense run: vis_ptr [n_query + 1],
//   vis_lm [n_vis].  A home listed twice counts once.  An entry outside [0, n_ref) other than -1 is an error in the host form
//   (lm_home_entry_ok) and ignored in the device form (lm_home_word).  The key points of the view's set are zeros, as they are
//   for the map's own set.
// MATCHES.  ptz_desc_match_pairs over the pairs (view image q, query image q) with the caller's match options; idx_a is view-local
//   and lifted through vis_lm.
// WHOLE MAP.  A list that names every non-empty home makes the view the whole map in order, and the matches are then those of the
//   dense landmark run, array for array.
#pragma once

#include "ptz_desc_shortlist.h"

namespace ptz {

constexpr int32_t kLmHomeWords = 8192 / 32;  // a bitmap over homes: the map's limit of 8192 references (kLandmarkMaxRefs), 1 KiB

// the grouping: false if a home is outside [0, n_ref) (home_ptr and home_lm are then unspecified)
PTZ_HD bool lm_home_groups(const int32_t* home, int32_t n_lm, int32_t n_ref, int64_t* home_ptr, int32_t* home_lm)
{
  for (int32_t r = 0; r <= n_ref; ++r) home_ptr[r] = 0;
  for (int32_t l = 0; l < n_lm; ++l) {
    if (home[l] < 0 || home[l] >= n_ref) return false;
    ++home_ptr[home[l] + 1];
  }
  for (int32_t r = 0; r < n_ref; ++r) home_ptr[r + 1] += home_ptr[r];
  for (int32_t l = 0; l < n_lm; ++l) home_lm[home_ptr[home[l]]++] = l;  // entry r is now the END of group r: the start of r + 1
  for (int32_t r = n_ref; r > 0; --r) home_ptr[r] = home_ptr[r - 1];
  home_ptr[0] = 0;
  return true;
}

// the host form's check of one list entry
PTZ_HD bool lm_home_entry_ok(int32_t e, int32_t n_ref) { return e == -1 || (e >= 0 && e < n_ref); }

// one word of a query's bitmap over homes from its list [R]: the bits of the entries in [32 w, 32 w + 32) and in [0, n_ref)
PTZ_HD uint32_t lm_home_word(const int32_t* list, int32_t R, int32_t n_ref, int32_t w)
{
  uint32_t bits = 0;
  for (int32_t k = 0; k < R; ++k) {
    const int32_t e = list[k];
    if (e >= 0 && e < n_ref && (e >> 5) == w) bits |= 1u << (e & 31);
  }
  return bits;
}

// landmark with home h is in the view of the query whose bitmap is `bits`
PTZ_HD bool lm_home_listed(const uint32_t* bits, int32_t n_ref, int32_t h) { return h >= 0 && h < n_ref && ((bits[h >> 5] >> (h & 31)) & 1u) != 0; }

}  // namespace ptz
