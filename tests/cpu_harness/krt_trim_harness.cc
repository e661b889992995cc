// krt_trim_harness.cc -- TEST INFRASTRUCTURE.  Host instantiation of the trimmed relocalization's rule in
// ptz-calib_amd/csrc/ptz_krt_trim.h (what k_krt_trim_step spreads over the lanes of a group) so it can be held to a numpy
// restatement without a GPU, and used as "the rule header on the host" of the manual loop the device loop must equal.  Never part
// of the product library.  With KRT_TRIM_HARNESS_MAIN it is a stand-alone program (for a sanitizer build): it runs the rule on
// generated errors of every size 0 .. 200 against a sort and returns 0 if they agree.
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../ptz-calib_amd/csrc/ptz_krt_trim.h"

using namespace ptz;

extern "C" {
// One round of one query: err [n] (the report's err_px), in_u (may be null: all) / in_k [n] bytes.  Returns the decision (-1 go
// on with new_k, 0 done, 2 max_rounds, 4 min_keep; -100 invalid options); t, median and new_k [n] are written.
int h_krt_trim_round(double trim_px, double k_sigma, int max_rounds, int min_keep, int64_t n, const double* err, const unsigned char* in_u,
                     const unsigned char* in_k, int rounds_run, unsigned char* new_k, double* t, double* median)
{
  const KrtTrimRule r = {trim_px, k_sigma, max_rounds, min_keep};
  if (!krt_trim_rule_valid(r)) return -100;
  return krt_trim_round(r, n, err, in_u, in_k, rounds_run, new_k, t, median);
}
}

#ifdef KRT_TRIM_HARNESS_MAIN
int main()
{
  uint64_t s = 12345;
  auto next = [&s]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) / 9007199254740992.0; };
  int bad = 0;
  for (int n = 0; n <= 200; ++n) {
    std::vector<double> err(n);
    std::vector<unsigned char> u(n), k(n), nk(n);
    for (int m = 0; m < n; ++m) {
      err[m] = next() < 0.1 ? -1.0 : (next() < 0.2 ? 30.0 * next() : 2.0 * next());
      if (m % 7 == 3 && m > 0) err[m] = err[m - 1];  // ties
      u[m] = next() < 0.9;
      k[m] = u[m] && next() < 0.8;
    }
    std::vector<double> c;
    for (int m = 0; m < n; ++m)
      if (k[m] && err[m] >= 0) c.push_back(err[m]);
    std::sort(c.begin(), c.end());
    double t, med;
    const KrtTrimRule r = {4.0, 3.0, 8, 8};
    const int d = krt_trim_round(r, n, err.data(), u.data(), k.data(), 1, nk.data(), &t, &med);
    if (c.empty() ? !std::isnan(med) : med != c[(c.size() - 1) / 2]) { printf("median differs at n = %d\n", n); ++bad; }
    const double te = c.empty() ? 4.0 : std::max(4.0, 3.0 * c[(c.size() - 1) / 2] / 1.1774);
    if (t != te) { printf("threshold differs at n = %d\n", n); ++bad; }
    long long chg = 0, cnt = 0;
    for (int m = 0; m < n; ++m) {
      const bool keep = u[m] && (err[m] < 0 || err[m] <= t);
      if (keep != (nk[m] != 0)) { printf("set differs at n = %d\n", n); ++bad; }
      chg += keep != (k[m] != 0);
      cnt += keep && err[m] >= 0;
    }
    const int de = chg == 0 ? 0 : (cnt < 8 ? 4 : -1);
    if (d != de) { printf("decision differs at n = %d: %d, expected %d\n", n, d, de); ++bad; }
  }
  printf("krt_trim_harness: %d mismatches\n", bad);
  return bad ? 1 : 0;
}
#endif
