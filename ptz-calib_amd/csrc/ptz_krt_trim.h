// ptz_krt_trim.h -- the outlier rule of the trimmed relocalization (ptz_krt_solve_batch_trimmed*) and the exact lower median of
// the residual report (ptz_krt_residuals_batch).
//
// PTZ_HD like ptz_ba_trim.h, whose threshold it reuses: the kernels of ptz_krt_resid.hip and the host (tests/cpu_harness/
// krt_trim_harness.cc) instantiate the same functions.
//
// The rule.  Matches of a query share no ray, so -- unlike the bundle adjustment's, which takes one observation per track and round --
// every match is judged on its own, and judged AGAIN every round:
//   universe U   the query's matches whose input match_mask byte is non-zero (all, if match_mask = NULL); nothing else ever enters;
//   counted      the matches of the current kept set K that the border guard of the distortion variants does not skip
//                (krt_optimizer.cc:97-101; their err_px is -1).  A skipped match stays in K, adds nothing, is never rejected;
//   threshold    t = max(trim_px, k_sigma * median / 1.1774), median = the exact lower median of |e_m| over the counted matches of K:
//                element (n - 1) / 2 of the sorted errors.  k_sigma = 0: t = trim_px;
//   new set      K' = { m in U : m skipped by the guard, or |e_m| <= t } -- with re-admission: a good match that a dragged early fit
//                pushed above the threshold comes back;
//   a query is finished when K' == K; when K' would count fewer than min_keep matches (flagged, keeps K); when it has run max_rounds
//   solves (flagged); when a solve of it was not accepted (flagged, decided by the caller of this header).
#pragma once

#include "ptz_ba_trim.h"

namespace ptz {

struct KrtTrimRule {
  double trim_px;  // > 0
  double k_sigma;  // >= 0
  int max_rounds;  // >= 1
  int min_keep;    // >= 0
};

// what a round decides for a query (the values of the flags in ptz_calib_amd.h, PTZ_TRIM_MAX_ROUNDS and PTZ_KRT_TRIM_MIN_KEEP)
constexpr int kKrtTrimContinue = -1, kKrtTrimDone = 0, kKrtTrimMaxRounds = 2, kKrtTrimMinKeep = 4, kKrtTrimRejected = 8;

PTZ_HD bool krt_trim_rule_valid(const KrtTrimRule& r)
{
  return r.trim_px > 0.0 && r.trim_px < 1e300 && r.k_sigma >= 0.0 && r.k_sigma < 1e300 && r.max_rounds >= 1 && r.min_keep >= 0;
}
PTZ_HD bool krt_trim_skipped(double err) { return err < 0.0; }  // the report's -1.0
PTZ_HD bool krt_trim_counted(bool in_kept, double err) { return in_kept && !krt_trim_skipped(err); }
PTZ_HD double krt_trim_threshold(const KrtTrimRule& r, double median)
{
  const TrimRule b = {r.trim_px, r.k_sigma, 2};
  return trim_threshold(b, median);
}
PTZ_HD bool krt_trim_keeps(bool in_universe, double err, double t) { return in_universe && (krt_trim_skipped(err) || err <= t); }
// n_changed: matches whose membership differs between K and K'; n_new_counted: counted matches of K'; rounds_run: solves so far
PTZ_HD int krt_trim_decide(const KrtTrimRule& r, long long n_changed, long long n_new_counted, int rounds_run)
{
  if (n_changed == 0) return kKrtTrimDone;
  if (n_new_counted < (long long)r.min_keep) return kKrtTrimMinKeep;
  if (rounds_run >= r.max_rounds) return kKrtTrimMaxRounds;
  return kKrtTrimContinue;
}

// The errors are non-negative doubles, whose bit patterns order like the values: the pattern of element k of the sorted list is the
// LARGEST v with (number of patterns below v) <= k, fixed bit by bit from the top.  below(v): the number of counted patterns < v (a
// pattern of the sign bit's half is never asked for).  No sort, no histogram, no atomics: 63 counting passes.
PTZ_HD unsigned long long krt_trim_key(double err)
{
  union { double d; unsigned long long u; } c;
  c.d = err;
  return c.u & 0x7fffffffffffffffull;
}
PTZ_HD double krt_trim_key_value(unsigned long long key)
{
  union { double d; unsigned long long u; } c;
  c.u = key;
  return c.d;
}
template <class Below> PTZ_HD unsigned long long krt_trim_kth_key(long long k, Below below)
{
  unsigned long long prefix = 0;
  for (int bit = 62; bit >= 0; --bit) {
    const unsigned long long cand = prefix | (1ull << bit);
    if (below(cand) <= k) prefix = cand;
  }
  return prefix;
}

// One round of one query, serially (the host's form; the kernel spreads the same functions over the lanes of a group).
//   err [n] the report's err_px at the round's camera, in_u / in_k [n] bytes (in_u may be null: all), rounds_run solves so far.
// Writes t and median (NaN without a counted match), new_k [n] = K' and returns kKrtTrim*: only with kKrtTrimContinue does K' replace K.
inline int krt_trim_round(const KrtTrimRule& r, long long n, const double* err, const unsigned char* in_u, const unsigned char* in_k,
                          int rounds_run, unsigned char* new_k, double* t_out, double* median_out)
{
  long long cnt = 0;
  for (long long m = 0; m < n; ++m) cnt += krt_trim_counted(in_k[m] != 0, err[m]) ? 1 : 0;
  double median = krt_trim_key_value(0x7ff8000000000000ull);
  if (cnt > 0) {
    const unsigned long long key = krt_trim_kth_key(trim_median_index(cnt), [&](unsigned long long v) {
      long long c = 0;
      for (long long m = 0; m < n; ++m) c += (krt_trim_counted(in_k[m] != 0, err[m]) && krt_trim_key(err[m]) < v) ? 1 : 0;
      return c;
    });
    median = krt_trim_key_value(key);
  }
  const double t = krt_trim_threshold(r, median);
  long long changed = 0, new_counted = 0;
  for (long long m = 0; m < n; ++m) {
    const bool keep = krt_trim_keeps(in_u ? in_u[m] != 0 : true, err[m], t);
    new_k[m] = keep ? 1 : 0;
    changed += keep != (in_k[m] != 0) ? 1 : 0;
    new_counted += (keep && !krt_trim_skipped(err[m])) ? 1 : 0;
  }
  *t_out = t;
  *median_out = median;
  return krt_trim_decide(r, changed, new_counted, rounds_run);
}

}  // namespace ptz
