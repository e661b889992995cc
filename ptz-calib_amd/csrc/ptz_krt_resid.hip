// ptz_krt_resid.hip -- residual report of relocalized cameras and the trimmed relocalization, batched over queries (gfx950).
//
// ptz_krt_residuals_batch: what a caller of ptz_krt_solve_batch cannot see -- which matches the fit rests on.  One evaluation of the
// LM's own functors at the refined camera (krt_eval in the EXACT form, the one the solve takes its final cost with), the camera moved
// into the reference's local frame by krt_cov_local_frame (k_krt's prologue, shared with the covariance).
// ptz_krt_solve_batch_trimmed: solve, report, rule (ptz_krt_trim.h), compaction (ptz_gate_compact.h), solve again -- all rounds
// enqueued on one stream, no host round trip between them.
//
// Kernel shape.  A group of G lanes per query, G = 64 (a wave) or 16 (a DPP row) as k_krt takes it (krt_group_size).  Lane l takes
// matches l, l + G, l + 2 G, ..; the errors of its first eight stay in registers for the median and the rule, later ones are read
// back from err_px (each lane reads what it wrote).  No LDS: a reference ray is used once, so k_krt's ray cache would cache nothing.
// ONE reduction order whatever G: the sum of squares is kept in 64 partial sums -- partial v takes matches v, v + 64, .. -- which a
// wave holds one per lane and a row of sixteen lanes four per lane (v = l, l + 16, l + 32, l + 48); the wave's butterfly adds lane
// l ^ 32, l ^ 16, l ^ 8, .. l ^ 1, the row first adds (p[l] + p[l + 32]) + (p[l + 16] + p[l + 48]) in registers -- the butterfly's
// first two steps -- and then l ^ 8 .. l ^ 1.  Same operands, same order: a query's bits depend on its own data only, not on its
// neighbours, their number, the group size or the run.  The median is a selection by counting over the bit patterns of the
// non-negative doubles (ptz_krt_trim.h): integers only.  No floating-point atomics.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

#include "ptz_common.h"
#include "ptz_pool.h"
#include "ptz_krt_device.h"
#include "ptz_krt_cov.h"
#include "ptz_krt_trim.h"
#include "ptz_gate_compact.h"

namespace ptz {
namespace {

static_assert(kKrtTrimMaxRounds == PTZ_TRIM_MAX_ROUNDS && kKrtTrimMinKeep == PTZ_KRT_TRIM_MIN_KEEP && kKrtTrimRejected == PTZ_KRT_TRIM_REJECTED,
              "ptz_krt_trim.h and ptz_calib_amd.h name the same flags");

constexpr int TRIM_ROUNDS_LIMIT = 64;  // rounds one call enqueues at most
constexpr int RESID_E = 8;  // errors of a query a lane keeps in registers: 128 matches at G = 16, 512 at G = 64

struct KrtResidOut {
  double *err, *err3, *rms, *mx, *median, *rms3;
  int* count;
};
struct ResidLane {
  double e[RESID_E];  // err_px of match lane + G i; -1 past the query's end
  unsigned counted;   // bit i: that match counts (in the mask, not skipped)
};
struct ResidStats {
  double rms, mx, median, rms3d;
  int count;
};

// the 64 partial sums of a group (see the head of the file) added in the wave butterfly's order
template <int G> __device__ __forceinline__ double group_sum64(const double (&p)[64 / G])
{
  if constexpr (G == 64) return wave_sum(p[0]);
  else return group_sum<16>((p[0] + p[2]) + (p[1] + p[3]));
}

// The report of query q by its group.  mask (nullable): the matches that count; err / err3 (nullable): err_px / err3d_px of the whole
// batch.  want_median needs err when the query has more than RESID_E * G matches.  Every lane of the group returns the same st.
template <int KTYPE, bool P3, int G>
__device__ __forceinline__ void krt_resid_query(const KrtBatch& in, int q, int lane, const unsigned char* mask, double* err, double* err3,
                                                bool want_median, ResidLane& ln, ResidStats& st)
{
  constexpr int NF = KrtDims<KTYPE>::NF, NV = 64 / G;
  static_assert(RESID_E % NV == 0, "the register part ends on a whole turn of the partial sums");
  const long long m0 = in.match_ptr[q];
  const int M = (int)(in.match_ptr[q + 1] - m0);
  const long long p0 = P3 ? in.point_ptr[q] : 0;
  const int NP = P3 ? (int)(in.point_ptr[q + 1] - p0) : 0;
  double ref[15], cur[15], x[15], Rref[9], R[9];
#pragma unroll
  for (int k = 0; k < 15; ++k) { ref[k] = in.cam_ref[(size_t)q * 15 + k]; cur[k] = in.cam_cur[(size_t)q * 15 + k]; }
  krt_cov_local_frame(ref, cur, x, Rref, R);
  const double kref[4] = {ref[0], ref[1], ref[2], ref[3]};
  const double dref[5] = {ref[10], ref[11], ref[12], ref[13], ref[14]};
  const double fy = (KTYPE & 2) ? x[1] : x[0];
  double ss[NV], mx = 0;
  int cnt = 0;
#pragma unroll
  for (int j = 0; j < NV; ++j) ss[j] = 0;
  // |e_m| of match m, -1 if the border guard skips it; counted: in the mask and not skipped
  auto eval = [&](int m, bool& counted) -> double {
    const float2 a = in.uv_ref[m0 + m], b = in.uv_cur[m0 + m];
    double r1[3], res[2], J[2][NF];
    bool skip;
    MatchEval<KTYPE>::ray1(kref, dref, a.x, a.y, r1, skip);
    krt_eval<KTYPE, false, true>(R, nullptr, x[0], fy, x[2], x[3], x + 10, r1, skip, b.x, b.y, res, J);
    const double e = skip ? -1.0 : sqrt(__builtin_fma(res[0], res[0], res[1] * res[1]));
    if (err) err[m0 + m] = e;
    counted = !skip && (!mask || mask[m0 + m] != 0);
    return e;
  };
  ln.counted = 0;
#pragma unroll
  for (int i = 0; i < RESID_E; ++i) {
    const int m = lane + G * i;
    ln.e[i] = -1.0;
    if (m < M) {
      bool c;
      const double e = eval(m, c);
      ln.e[i] = e;
      if (c) { ss[i % NV] = __builtin_fma(e, e, ss[i % NV]); mx = fmax(mx, e); ++cnt; ln.counted |= 1u << i; }
    }
  }
  for (int i0 = RESID_E; G * i0 < M; i0 += NV) {  // (the bound is the group's: every lane makes the same turns)
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int m = lane + G * (i0 + j);
      if (m < M) {
        bool c;
        const double e = eval(m, c);
        if (c) { ss[j] = __builtin_fma(e, e, ss[j]); mx = fmax(mx, e); ++cnt; }
      }
    }
  }
  double s3[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) s3[j] = 0;
  if (P3) {
    for (int i0 = 0; G * i0 < NP; i0 += NV) {
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        const int i = lane + G * (i0 + j);
        if (i < NP) {
          const float2 b = in.pt_uv[p0 + i];
          const double* X = in.pt_xyz + 3 * (p0 + i);
          double Xl[3], res[2], J[2][NF];  // R_local_world X_w + t_local_world (krt_optimizer.cc:357-362)
          Xl[0] = Rref[0] * X[0] + Rref[1] * X[1] + Rref[2] * X[2] + ref[7];
          Xl[1] = Rref[3] * X[0] + Rref[4] * X[1] + Rref[5] * X[2] + ref[8];
          Xl[2] = Rref[6] * X[0] + Rref[7] * X[1] + Rref[8] * X[2] + ref[9];
          krt_eval_2d3d<KTYPE, false>(R, nullptr, x[0], fy, x[2], x[3], x + 10, x + 7, Xl, b.x, b.y, res, J);
          const double e = sqrt(__builtin_fma(res[0], res[0], res[1] * res[1]));
          if (err3) err3[p0 + i] = e;
          s3[j] = __builtin_fma(e, e, s3[j]);
        }
      }
    }
  }
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const double sum = group_sum64<G>(ss);
  const double top = group_max<G>(mx);
  const int n = (int)group_sum<G>((double)cnt);  // (an integer held as a double: exact)
  st.count = n;
  st.rms = n > 0 ? sqrt(sum / (double)n) : nan;
  st.mx = n > 0 ? top : nan;
  st.rms3d = nan;
  if (P3) {
    const double sum3 = group_sum64<G>(s3);
    if (NP > 0) st.rms3d = sqrt(sum3 / (double)NP);
  }
  st.median = nan;
  if (want_median && n > 0) {
    unsigned long long key[RESID_E];  // a match that does not count: above every pattern asked for
#pragma unroll
    for (int i = 0; i < RESID_E; ++i) key[i] = ((ln.counted >> i) & 1u) ? krt_trim_key(ln.e[i]) : ~0ull;
    const unsigned long long kth = krt_trim_kth_key(trim_median_index(n), [&](unsigned long long v) -> long long {
      int c = 0;
#pragma unroll
      for (int i = 0; i < RESID_E; ++i) c += key[i] < v ? 1 : 0;
      for (int m = lane + G * RESID_E; m < M; m += G) {
        const double e = err[m0 + m];
        c += (!krt_trim_skipped(e) && (!mask || mask[m0 + m] != 0) && krt_trim_key(e) < v) ? 1 : 0;
      }
      return (long long)group_sum<G>((double)c);  // (an integer held as a double: exact; measured faster than eight ballots a pass)
    });
    st.median = krt_trim_key_value(kth);
  }
}

template <int KTYPE, bool P3, int G>
__global__ __launch_bounds__(256) void k_krt_resid(KrtBatch in, const unsigned char* __restrict__ mask, const int* __restrict__ accepted,
                                                   KrtResidOut out)
{
  const int q = blockIdx.x * (256 / G) + (int)threadIdx.x / G;
  if (q >= in.n_query) return;  // (whole groups leave: the cross-lane moves stay inside a group)
  if (accepted && accepted[q] == 0) return;  // the solve never wrote this query's camera: nothing of it is read or written
  const int lane = threadIdx.x % G;
  ResidLane ln;
  ResidStats st;
  krt_resid_query<KTYPE, P3, G>(in, q, lane, mask, out.err, out.err3, out.median != nullptr, ln, st);
  if (lane != 0) return;
  if (out.rms) out.rms[q] = st.rms;
  if (out.mx) out.mx[q] = st.mx;
  if (out.median) out.median[q] = st.median;
  if (out.count) out.count[q] = st.count;
  if (out.rms3) out.rms3[q] = st.rms3d;
}

// One round's report and rule for the queries still active, behind their solve: in.cam_cur = the loop's working cameras.
// umask (nullable): the universe; kmask: the kept set, the round's solve ran on it -- replaced by K' only if the query goes on.
template <int KTYPE, bool P3, int G>
__global__ __launch_bounds__(256) void k_krt_trim_step(KrtBatch in, const unsigned char* __restrict__ umask, unsigned char* kmask, double* err,
                                                       const int* __restrict__ acc_round, int* __restrict__ active, KrtTrimRule rule, int round,
                                                       ptz_krt_trim_report* __restrict__ rep, int* __restrict__ live)
{
  const int q = blockIdx.x * (256 / G) + (int)threadIdx.x / G;
  if (q >= in.n_query) return;
  if (active[q] == 0) return;
  const int lane = threadIdx.x % G;
  const long long m0 = in.match_ptr[q];
  const int M = (int)(in.match_ptr[q + 1] - m0);
  int chg = 0, newc = 0, newk = 0, nk = 0, nu = 0;
  auto in_u = [&](int m) { return umask ? umask[m0 + m] != 0 : true; };
  if (acc_round[q] == 0) {  // the round's solve was not accepted under the open bound: the camera stays where it was
    for (int m = lane; m < M; m += G) { nk += kmask[m0 + m] != 0 ? 1 : 0; nu += in_u(m) ? 1 : 0; }
    nk = (int)group_sum<G>((double)nk);
    nu = (int)group_sum<G>((double)nu);
    if (lane == 0) {
      rep[q].rounds = round + 1;
      rep[q].flags = kKrtTrimRejected;
      rep[q].n_kept = nk;
      rep[q].n_removed = nu - nk;
      active[q] = 0;
    }
    return;
  }
  ResidLane ln;
  ResidStats st;
  krt_resid_query<KTYPE, P3, G>(in, q, lane, kmask, err, nullptr, true, ln, st);
  const double t = krt_trim_threshold(rule, st.median);
  auto judge = [&](int m, double e) {
    const bool u = in_u(m), k = kmask[m0 + m] != 0, keep = krt_trim_keeps(u, e, t);
    chg += keep != k ? 1 : 0;
    newk += keep ? 1 : 0;
    newc += (keep && !krt_trim_skipped(e)) ? 1 : 0;
    nk += k ? 1 : 0;
    nu += u ? 1 : 0;
  };
#pragma unroll
  for (int i = 0; i < RESID_E; ++i)
    if (lane + G * i < M) judge(lane + G * i, ln.e[i]);
  for (int m = lane + G * RESID_E; m < M; m += G) judge(m, err[m0 + m]);
  chg = (int)group_sum<G>((double)chg);
  newk = (int)group_sum<G>((double)newk);
  newc = (int)group_sum<G>((double)newc);
  nk = (int)group_sum<G>((double)nk);
  nu = (int)group_sum<G>((double)nu);
  const int d = krt_trim_decide(rule, chg, newc, round + 1);
  if (d == kKrtTrimContinue) {
#pragma unroll
    for (int i = 0; i < RESID_E; ++i)
      if (lane + G * i < M) kmask[m0 + lane + G * i] = krt_trim_keeps(in_u(lane + G * i), ln.e[i], t) ? 1 : 0;
    for (int m = lane + G * RESID_E; m < M; m += G) kmask[m0 + m] = krt_trim_keeps(in_u(m), err[m0 + m], t) ? 1 : 0;
  }
  if (lane == 0) {
    const int kept = d == kKrtTrimContinue ? newk : nk;
    rep[q].rounds = round + 1;
    rep[q].flags = d == kKrtTrimContinue ? 0 : d;
    rep[q].n_kept = kept;
    rep[q].n_removed = nu - kept;
    rep[q].threshold = t;
    if (round == 0) rep[q].rms_first = st.rms;
    rep[q].rms_last = st.rms;
    rep[q].median_last = st.median;
    active[q] = d == kKrtTrimContinue ? 1 : 0;
    if (d == kKrtTrimContinue) atomicAdd(&live[round + 1], 1);  // (an integer, read as zero / not zero by the next round's compaction)
  }
}

__global__ void k_krt_trim_init_query(int n_query, const double* __restrict__ cam_cur, double* __restrict__ cam_work, int* __restrict__ active,
                                      int* __restrict__ acc_round, ptz_krt_trim_report* __restrict__ rep, int* __restrict__ live)
{
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q <= TRIM_ROUNDS_LIMIT) live[q] = q == 0 ? n_query : 0;  // queries with work per round: all in round 0 (the grid has 256 threads at least)
  if (q >= n_query) return;
  for (int k = 0; k < 15; ++k) cam_work[(size_t)q * 15 + k] = cam_cur[(size_t)q * 15 + k];
  active[q] = 1;
  acc_round[q] = 0;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  ptz_krt_trim_report r;
  r.rounds = 0; r.flags = 0; r.n_removed = 0; r.n_kept = 0;
  r.threshold = nan; r.rms_first = nan; r.rms_last = nan; r.median_last = nan;
  rep[q] = r;
}
__global__ void k_krt_trim_init_match(long long n_match, const unsigned char* __restrict__ umask, unsigned char* __restrict__ kmask)
{
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_match) kmask[i] = (!umask || umask[i] != 0) ? 1 : 0;
}
// accepted = (last solve accepted under the open bound) && CheckResults' error test with the caller's bound (krt_optimizer.cc:504-533);
// only then does the camera go out
__global__ void k_krt_trim_finish_query(int n_query, const double* __restrict__ cam_work, const ptz_lm_summary* __restrict__ summ,
                                        const int* __restrict__ acc_round, double max_reproj_error, double* __restrict__ cam_cur,
                                        int* __restrict__ accepted)
{
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n_query) return;
  const double reproj = sqrt(2.0) * sqrt((2 * summ[q].final_cost) / summ[q].num_residuals);
  const bool ok = acc_round[q] != 0 && reproj < max_reproj_error;
  accepted[q] = ok ? 1 : 0;
  if (ok)
    for (int k = 0; k < 15; ++k) cam_cur[(size_t)q * 15 + k] = cam_work[(size_t)q * 15 + k];
}
__global__ void k_krt_trim_finish_match(long long n_match, const unsigned char* __restrict__ kmask, unsigned char* __restrict__ kept)
{
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_match) kept[i] = kmask[i];
}

#define PTZ_KRT_BY_TYPE(LAUNCH, factor_type, p3, G)                      \
  do {                                                                   \
    switch ((factor_type) * 4 + ((p3) ? 2 : 0) + ((G) == 16 ? 1 : 0)) {  \
      case 0: LAUNCH(0, false, 64); break;                               \
      case 1: LAUNCH(0, false, 16); break;                               \
      case 2: LAUNCH(0, true, 64); break;                                \
      case 3: LAUNCH(0, true, 16); break;                                \
      case 4: LAUNCH(1, false, 64); break;                               \
      case 5: LAUNCH(1, false, 16); break;                               \
      case 6: LAUNCH(1, true, 64); break;                                \
      case 7: LAUNCH(1, true, 16); break;                                \
      case 8: LAUNCH(2, false, 64); break;                               \
      case 9: LAUNCH(2, false, 16); break;                               \
      case 10: LAUNCH(2, true, 64); break;                               \
      case 11: LAUNCH(2, true, 16); break;                               \
      case 12: LAUNCH(3, false, 64); break;                              \
      case 13: LAUNCH(3, false, 16); break;                              \
      case 14: LAUNCH(3, true, 64); break;                               \
      default: LAUNCH(3, true, 16); break;                               \
    }                                                                    \
  } while (0)

void launch_krt_resid(const KrtBatch& in, int factor_type, int G, const unsigned char* d_mask, const int* d_acc, const KrtResidOut& out,
                      hipStream_t st)
{
  const int qpb = 256 / G;
  const dim3 grid((in.n_query + qpb - 1) / qpb), block(256);
#define PTZ_RESID_LAUNCH(T, P, GG) hipLaunchKernelGGL((k_krt_resid<T, P, GG>), grid, block, 0, st, in, d_mask, d_acc, out)
  PTZ_KRT_BY_TYPE(PTZ_RESID_LAUNCH, factor_type, in.point_ptr != nullptr, G);
#undef PTZ_RESID_LAUNCH
}

void launch_krt_trim_step(const KrtBatch& in, int factor_type, int G, const unsigned char* d_umask, unsigned char* d_kmask, double* d_err,
                          const int* d_acc_round, int* d_active, const KrtTrimRule& rule, int round, ptz_krt_trim_report* d_rep, int* d_live,
                          hipStream_t st)
{
  const int qpb = 256 / G;
  const dim3 grid((in.n_query + qpb - 1) / qpb), block(256);
  // (2D-3D points are reported, not trimmed: the step never looks at them)
#define PTZ_STEP_LAUNCH(T, P, GG) \
  hipLaunchKernelGGL((k_krt_trim_step<T, false, GG>), grid, block, 0, st, in, d_umask, d_kmask, d_err, d_acc_round, d_active, rule, round, d_rep, d_live)
  PTZ_KRT_BY_TYPE(PTZ_STEP_LAUNCH, factor_type, in.point_ptr != nullptr, G);
#undef PTZ_STEP_LAUNCH
}

// the loop's device state, cut from one block
struct TrimWork {
  double* cam;          // [n][15] working cameras: what the rounds' solves read and write
  double* err;          // [n_match] the round's err_px
  unsigned char* kmask; // [n_match] the kept set
  int *active, *acc_round, *cnt;  // [n]
  int* live;            // [TRIM_ROUNDS_LIMIT + 1] queries that have work in round r
  long long* optr;      // [n + 1] the compacted CSR
  float2 *oref, *ocur;  // [n_match]
  ptz_krt_trim_report* rep;  // [n] (used when the caller wants no report)
};
size_t trim_work_cut(int n_query, long long n_match, char* base, TrimWork* w)
{
  const size_t n = (size_t)n_query, nm = (size_t)(n_match > 0 ? n_match : 1);
  BlockLayout lay;
  auto take = [&](size_t bytes) { const size_t at = lay.take(bytes); return base ? base + at : nullptr; };
  char* p_cam = take(sizeof(double) * 15 * n);
  char* p_err = take(sizeof(double) * nm);
  char* p_k = take(nm);
  char* p_act = take(sizeof(int) * n);
  char* p_acc = take(sizeof(int) * n);
  char* p_cnt = take(sizeof(int) * n);
  char* p_optr = take(sizeof(long long) * (n + 1));
  char* p_oref = take(sizeof(float2) * nm);
  char* p_ocur = take(sizeof(float2) * nm);
  char* p_rep = take(sizeof(ptz_krt_trim_report) * n);
  char* p_live = take(sizeof(int) * (TRIM_ROUNDS_LIMIT + 1));
  if (w) {
    w->cam = (double*)p_cam; w->err = (double*)p_err; w->kmask = (unsigned char*)p_k; w->active = (int*)p_act; w->acc_round = (int*)p_acc;
    w->cnt = (int*)p_cnt; w->optr = (long long*)p_optr; w->oref = (float2*)p_oref; w->ocur = (float2*)p_ocur; w->rep = (ptz_krt_trim_report*)p_rep;
    w->live = (int*)p_live;
  }
  return lay.total();
}

// Every round of the trimmed solve on `st`, device pointers throughout: [compaction of the kept sets | k_krt with the open bound on
// the queries still active | report + rule + decision] x max_rounds between the copy of the cameras into the workspace and the final
// acceptance.  A query that is finished is left alone by every kernel (`active`); a round no query reaches costs its launches only:
// w.live[r] counts the queries that go into round r, and the compaction -- whose scan walks all n counts in one workgroup --
// returns at once where it reads 0.
void enqueue_trimmed(const KrtBatch& in, long long n_match, int factor_type, double max_reproj_error, const unsigned char* d_umask,
                     const KrtTrimRule& rule, const ptz_lm_options& o, ptz_lm_summary* d_sum, int* d_acc, unsigned char* d_kept,
                     ptz_krt_trim_report* d_rep, const TrimWork& w, hipStream_t st)
{
  const int n = in.n_query;
  const int G = krt_group_size(n, o.krt_lanes_per_query);  // of the CALL's size, every round
  ptz_krt_trim_report* rep = d_rep ? d_rep : w.rep;
  const unsigned mgrid = (unsigned)((n_match + 255) / 256);
  hipLaunchKernelGGL(k_krt_trim_init_query, dim3((n + 255) / 256), dim3(256), 0, st, n, (const double*)in.cam_cur, w.cam, w.active, w.acc_round, rep, w.live);
  if (n_match > 0) hipLaunchKernelGGL(k_krt_trim_init_match, dim3(mgrid), dim3(256), 0, st, n_match, d_umask, w.kmask);
  KrtBatch at = in;
  at.cam_cur = w.cam;
  for (int r = 0; r < rule.max_rounds; ++r) {
    KrtBatch kept = at;
    if (r > 0 || d_umask) {  // (else the kept set is every match: the caller's arrays ARE the packed ones)
      // the kept matches of the active queries from the ORIGINAL arrays, in their order (a finished query packs nothing)
      enqueue_compact(n, (const int64_t*)in.match_ptr, (const int32_t*)w.active, w.kmask, 0, w.cnt, (int64_t*)w.optr, in.uv_ref, in.uv_cur,
                      w.oref, w.ocur, nullptr, st, w.live + r);
      kept.match_ptr = w.optr; kept.uv_ref = w.oref; kept.uv_cur = w.ocur;
    }
    krt_enqueue(kept, factor_type, o, 1e300, G, d_sum, w.acc_round, w.active, st);
    launch_krt_trim_step(at, factor_type, G, d_umask, w.kmask, w.err, w.acc_round, w.active, rule, r, rep, w.live, st);
  }
  hipLaunchKernelGGL(k_krt_trim_finish_query, dim3((n + 255) / 256), dim3(256), 0, st, n, (const double*)w.cam, (const ptz_lm_summary*)d_sum,
                     (const int*)w.acc_round, max_reproj_error, in.cam_cur, d_acc);
  if (d_kept && n_match > 0) hipLaunchKernelGGL(k_krt_trim_finish_match, dim3(mgrid), dim3(256), 0, st, n_match, (const unsigned char*)w.kmask, d_kept);
}

inline bool factor_type_ok(int factor_type) { return factor_type >= PTZ_KRT_F && factor_type <= PTZ_KRT_FxfyDist; }

}  // namespace
}  // namespace ptz

using namespace ptz;

extern "C" int32_t ptz_krt_residuals_batch_device(int32_t n_query, const int64_t* d_match_ptr, const float* d_uv_ref, const float* d_uv_cur,
                                                  const int64_t* d_point_ptr, const float* d_pts2d, const double* d_pts3d,
                                                  const double* d_cam_ref, const double* d_cam_cur, int32_t factor_type,
                                                  const uint8_t* d_match_mask, const int32_t* d_accepted, int32_t lanes_per_query,
                                                  double* d_err_px, double* d_err3d_px, double* d_rms, double* d_max, double* d_median,
                                                  int32_t* d_count, double* d_rms3d, void* hip_stream)
{
  if (n_query < 0) return PTZ_EINVAL;
  if (d_point_ptr && (!d_pts2d || !d_pts3d)) return PTZ_EINVAL;
  if (!d_err_px && !d_err3d_px && !d_rms && !d_max && !d_median && !d_count && !d_rms3d) return PTZ_EINVAL;
  if (d_median && !d_err_px) return PTZ_EINVAL;  // the selection reads a long query's errors back from err_px: no scratch of its own
  if (!factor_type_ok(factor_type)) return PTZ_EUNSUPPORTED;
  if (n_query == 0) return PTZ_OK;
  if (!d_match_ptr || !d_uv_ref || !d_uv_cur || !d_cam_ref || !d_cam_cur) return PTZ_EINVAL;
  clear_stale_error(__func__);
  int device = -1;
  if (const int rc = owning_device(d_cam_cur, hip_stream, &device)) return rc;
  PTZ_DEVICE_GUARD(device);
  const KrtBatch in = krt_batch_of(n_query, d_match_ptr, d_uv_ref, d_uv_cur, d_point_ptr, d_pts2d, d_pts3d, d_cam_ref, d_cam_cur);
  const KrtResidOut out = {d_err_px, d_point_ptr ? d_err3d_px : nullptr, d_rms, d_max, d_median, d_rms3d, d_count};
  launch_krt_resid(in, factor_type, krt_group_size(n_query, lanes_per_query), d_match_mask, d_accepted, out, (hipStream_t)hip_stream);
  PTZ_HIP_TRY(hipGetLastError());
  return PTZ_OK;
}

extern "C" int32_t ptz_krt_residuals_batch(int32_t n_query, const int64_t* match_ptr, const float* uv_ref, const float* uv_cur,
                                           const int64_t* point_ptr, const float* pts2d, const double* pts3d, const double* cam_ref,
                                           const double* cam_cur, int32_t factor_type, const uint8_t* match_mask, const int32_t* accepted,
                                           int32_t lanes_per_query, int32_t device_id, double* err_px, double* err3d_px, double* rms,
                                           double* max, double* median, int32_t* count, double* rms3d, double* device_ms)
{
  if (n_query < 0) return PTZ_EINVAL;
  const bool p3 = point_ptr != nullptr;
  if (p3 && (!pts2d || !pts3d)) return PTZ_EINVAL;
  if (!err_px && !err3d_px && !rms && !max && !median && !count && !rms3d) return PTZ_EINVAL;
  if (!factor_type_ok(factor_type)) return PTZ_EUNSUPPORTED;
  if (n_query == 0) return PTZ_OK;
  if (device_id < 0) return PTZ_EINVAL;
  const KrtHostBatch hb = {n_query, match_ptr, uv_ref, uv_cur, point_ptr, pts2d, pts3d, cam_ref, cam_cur};
  if (const int rc = check_host_batch(hb, kKrtCheckAll)) return rc;
  clear_stale_error(__func__);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device_id) return PTZ_ENODEVICE;
  PTZ_DEVICE_GUARD(device_id);
  // one pooled device block: [inputs | results]
  const size_t nq = (size_t)n_query, nmx = (size_t)std::max<int64_t>(hb.n_match(), 1), npx = (size_t)std::max<int64_t>(hb.n_point(), 1), D = sizeof(double);
  BlockLayout lay;
  const KrtBatchSlots slots = krt_batch_reserve(lay, n_query, hb.n_match(), hb.n_point(), match_mask != nullptr, accepted != nullptr);
  const size_t o_res = lay.total();
  const size_t o_err = lay.take(D * nmx), o_e3 = lay.take(D * npx), o_rms = lay.take(D * nq), o_max = lay.take(D * nq), o_med = lay.take(D * nq),
               o_rms3 = lay.take(D * nq), o_cnt = lay.take(sizeof(int) * nq), total = lay.total();
  CallHeld h;
  if (const int rc = h.acquire(device_id, total)) return rc;
  char* b = h.base;
  KrtBatch in;
  PTZ_HIP_TRY(krt_batch_upload(hb, match_mask, accepted, slots, h, false, &in));
  PTZ_HIP_TRY(hipEventRecord(h.ev[0], h.st));
  // err_px is always taken on the device: the median of a long query reads it back
  const KrtResidOut out = {(double*)(b + o_err), p3 ? (double*)(b + o_e3) : nullptr, (double*)(b + o_rms), (double*)(b + o_max),
                           median ? (double*)(b + o_med) : nullptr, (double*)(b + o_rms3), (int*)(b + o_cnt)};
  launch_krt_resid(in, factor_type, krt_group_size(n_query, lanes_per_query), match_mask ? (const unsigned char*)(b + slots.mask) : nullptr,
                   accepted ? (const int*)(b + slots.accepted) : nullptr, out, h.st);
  PTZ_HIP_TRY(hipEventRecord(h.ev[1], h.st));
  // the outputs of a query with accepted = 0 stay as the caller had them: the device's copies come back into a buffer of their own
  std::vector<char> hr(total - o_res);
  PTZ_HIP_TRY(hipMemcpyAsync(hr.data(), b + o_res, total - o_res, hipMemcpyDeviceToHost, h.st));
  PTZ_HIP_TRY(stream_wait(h.st));
  PTZ_HIP_TRY(hipGetLastError());  // a refused kernel launch must not pass for a result
  auto hd = [&](size_t off) { return reinterpret_cast<const double*>(hr.data() + (off - o_res)); };
  const int* hcnt = reinterpret_cast<const int*>(hr.data() + (o_cnt - o_res));
  for (int q = 0; q < n_query; ++q) {
    if (accepted && accepted[q] == 0) continue;
    const int64_t a = match_ptr[q], m = match_ptr[q + 1] - a;
    if (err_px && m > 0) memcpy(err_px + a, hd(o_err) + a, D * m);
    if (err3d_px && p3 && point_ptr[q + 1] > point_ptr[q]) memcpy(err3d_px + point_ptr[q], hd(o_e3) + point_ptr[q], D * (point_ptr[q + 1] - point_ptr[q]));
    if (rms) rms[q] = hd(o_rms)[q];
    if (max) max[q] = hd(o_max)[q];
    if (median) median[q] = hd(o_med)[q];
    if (count) count[q] = hcnt[q];
    if (rms3d) rms3d[q] = hd(o_rms3)[q];
  }
  if (device_ms) *device_ms = h.elapsed_ms();
  return PTZ_OK;
}

extern "C" void ptz_krt_trim_options_default(ptz_krt_trim_options* o)
{
  if (!o) return;
  o->trim_px = 4.0; o->k_sigma = 3.0; o->max_rounds = 8; o->min_keep = 8;
}

extern "C" int64_t ptz_krt_trim_workspace_bytes(int32_t n_query, int64_t n_match)
{
  if (n_query < 0 || n_match < 0) return PTZ_EINVAL;
  return (int64_t)trim_work_cut(n_query, n_match, nullptr, nullptr);
}

static bool trim_rule_from(const ptz_krt_trim_options* trim, KrtTrimRule* rule)
{
  ptz_krt_trim_options t;
  if (trim) t = *trim; else ptz_krt_trim_options_default(&t);
  *rule = KrtTrimRule{t.trim_px, t.k_sigma, t.max_rounds, t.min_keep};
  return krt_trim_rule_valid(*rule) && t.max_rounds <= TRIM_ROUNDS_LIMIT;
}

extern "C" int32_t ptz_krt_solve_batch_trimmed_device(int32_t n_query, int64_t n_match, const int64_t* d_match_ptr, const float* d_uv_ref,
                                                      const float* d_uv_cur, const int64_t* d_point_ptr, const float* d_pts2d,
                                                      const double* d_pts3d, const double* d_cam_ref, double* d_cam_cur, int32_t factor_type,
                                                      double max_reproj_error, const uint8_t* d_match_mask, const ptz_krt_trim_options* trim,
                                                      const ptz_lm_options* opt, ptz_lm_summary* d_summaries, int32_t* d_accepted,
                                                      uint8_t* d_kept, ptz_krt_trim_report* d_report, void* d_workspace,
                                                      int64_t workspace_bytes, void* hip_stream)
{
  if (n_query < 0 || n_match < 0) return PTZ_EINVAL;
  if (d_point_ptr && (!d_pts2d || !d_pts3d)) return PTZ_EINVAL;
  KrtTrimRule rule;
  if (!trim_rule_from(trim, &rule)) return PTZ_EINVAL;
  if (!factor_type_ok(factor_type)) return PTZ_EUNSUPPORTED;
  if (n_query == 0) return PTZ_OK;
  if (!d_match_ptr || !d_uv_ref || !d_uv_cur || !d_cam_ref || !d_cam_cur || !d_summaries || !d_accepted || !d_workspace) return PTZ_EINVAL;
  if (workspace_bytes < (int64_t)trim_work_cut(n_query, n_match, nullptr, nullptr)) return PTZ_EINVAL;
  if ((reinterpret_cast<uintptr_t>(d_workspace) & 255) != 0) return PTZ_EINVAL;
  ptz_lm_options o;
  if (opt) o = *opt; else ptz_lm_options_default(&o);
  clear_stale_error(__func__);
  int device = -1;
  if (const int rc = owning_device(d_cam_cur, hip_stream, &device)) return rc;
  if (opt && opt->device_id != 0 && opt->device_id != device) return PTZ_EINVAL;
  PTZ_DEVICE_GUARD(device);
  TrimWork w;
  trim_work_cut(n_query, n_match, (char*)d_workspace, &w);
  const KrtBatch in = krt_batch_of(n_query, d_match_ptr, d_uv_ref, d_uv_cur, d_point_ptr, d_pts2d, d_pts3d, d_cam_ref, d_cam_cur);
  enqueue_trimmed(in, n_match, factor_type, max_reproj_error, d_match_mask, rule, o, d_summaries, d_accepted, d_kept, d_report, w,
                  (hipStream_t)hip_stream);
  PTZ_HIP_TRY(hipGetLastError());
  return PTZ_OK;
}

extern "C" int32_t ptz_krt_solve_batch_trimmed(int32_t n_query, const int64_t* match_ptr, const float* uv_ref, const float* uv_cur,
                                               const int64_t* point_ptr, const float* pts2d, const double* pts3d, const double* cam_ref,
                                               double* cam_cur, int32_t factor_type, double max_reproj_error, const uint8_t* match_mask,
                                               const ptz_krt_trim_options* trim, const ptz_lm_options* opt, ptz_lm_summary* summaries,
                                               int32_t* accepted, uint8_t* kept, ptz_krt_trim_report* report, double* device_ms)
{
  if (n_query < 0) return PTZ_EINVAL;
  if (point_ptr && (!pts2d || !pts3d)) return PTZ_EINVAL;
  KrtTrimRule rule;
  if (!trim_rule_from(trim, &rule)) return PTZ_EINVAL;
  if (!factor_type_ok(factor_type)) return PTZ_EUNSUPPORTED;
  if (n_query == 0) return PTZ_OK;
  if (!summaries || !accepted) return PTZ_EINVAL;
  const KrtHostBatch hb = {n_query, match_ptr, uv_ref, uv_cur, point_ptr, pts2d, pts3d, cam_ref, cam_cur};
  if (const int rc = check_host_batch(hb, kKrtCheckAll)) return rc;
  ptz_lm_options o;
  if (opt) o = *opt; else ptz_lm_options_default(&o);
  if (o.device_id < 0) return PTZ_EINVAL;
  clear_stale_error(__func__);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= o.device_id) return PTZ_ENODEVICE;
  PTZ_DEVICE_GUARD(o.device_id);
  // one pooled device block: [inputs | cam_cur (in / out) | summaries | accepted | kept | report | the loop's state]
  const int64_t nm = hb.n_match();
  const size_t nq = (size_t)n_query, nmx = (size_t)std::max<int64_t>(nm, 1), D = sizeof(double);
  BlockLayout lay;
  const KrtBatchSlots slots = krt_batch_reserve(lay, n_query, nm, hb.n_point(), match_mask != nullptr, false);
  const size_t o_ccur = slots.cam_cur, o_sum = lay.take(sizeof(ptz_lm_summary) * nq), o_acc = lay.take(sizeof(int) * nq), o_kept = lay.take(nmx),
               o_rep = lay.take(sizeof(ptz_krt_trim_report) * nq), o_work = lay.take(trim_work_cut(n_query, nm, nullptr, nullptr));
  CallHeld h;
  if (const int rc = h.acquire(o.device_id, lay.total())) return rc;
  char* b = h.base;
  KrtBatch in;
  PTZ_HIP_TRY(krt_batch_upload(hb, match_mask, nullptr, slots, h, false, &in));
  PTZ_HIP_TRY(hipEventRecord(h.ev[0], h.st));
  TrimWork w;
  trim_work_cut(n_query, nm, b + o_work, &w);
  enqueue_trimmed(in, nm, factor_type, max_reproj_error, match_mask ? (const unsigned char*)(b + slots.mask) : nullptr, rule, o,
                  (ptz_lm_summary*)(b + o_sum), (int*)(b + o_acc), (unsigned char*)(b + o_kept), (ptz_krt_trim_report*)(b + o_rep), w, h.st);
  PTZ_HIP_TRY(hipEventRecord(h.ev[1], h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(cam_cur, b + o_ccur, D * 15 * nq, hipMemcpyDeviceToHost, h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(summaries, b + o_sum, sizeof(ptz_lm_summary) * nq, hipMemcpyDeviceToHost, h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(accepted, b + o_acc, sizeof(int) * nq, hipMemcpyDeviceToHost, h.st));
  if (kept && nm > 0) PTZ_HIP_TRY(hipMemcpyAsync(kept, b + o_kept, (size_t)nm, hipMemcpyDeviceToHost, h.st));
  if (report) PTZ_HIP_TRY(hipMemcpyAsync(report, b + o_rep, sizeof(ptz_krt_trim_report) * nq, hipMemcpyDeviceToHost, h.st));
  PTZ_HIP_TRY(stream_wait(h.st));
  PTZ_HIP_TRY(hipGetLastError());  // a refused kernel launch must not pass for a solve
  if (device_ms) *device_ms = h.elapsed_ms();
  return PTZ_OK;
}
