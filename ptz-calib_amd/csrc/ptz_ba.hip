// ptz_ba.hip -- PTZ-IBA global bundle adjustment on MI355X (gfx950): batched Levenberg-Marquardt over
// independent scenes, everything between the packed observations and the refined parameters on device.
//
// Replaces PTZRayOptimizer::Solve (src/core/ptzray_optimizer.cc:454-489) from AddConstraints2d2d
// (:799-885) through ceres::Solve (:469-475): residual blocks with ScaledLoss(track length) weights,
// SubsetParameterization masks (free: focal, rvec, ray [, k1]), the Ceres 1.14 trust-region LM policy
// (Jacobi scaling, LM diagonal clamp, step-quality radius update,
// function/parameter/gradient tolerances), Schur elimination of the 3x3 ray blocks (row S5) and the
// solve of the reduced camera system (ptz_chol.hip).
//
// Per LM pass and scene (all scenes of the batch advance in lock-step, finished scenes early-out):
//   lm_pre      finalize the previous iteration, termination checks               [1 block / scene]
//   ray_prep    E = (V + D^2)^-1 per ray, z = E g_r                                [thread / ray]
//   cam_diag    LM diagonal of the camera blocks                                   [thread / camera]
//   schur       row-block i of the reduced system: T_a = W_a E staged in LDS, S_ii, b_i, then
//               S_ij = - sum_{tracks seen by i and j} T_a W_b^T for j < i          [workgroup / camera]
//               (b is written as row n of the padded S)
//   cholesky    S y_c = b  (ptz_chol.hip: panel + MFMA syrk per 64-wide block column, back-substitution)
//   cam_update  candidate camera, its rotation block                              [thread / camera]
//   eval        y_r = E (g_r - sum_a Jr_a^T Jc_a y_c), candidate ray, model cost change
//               -(J d)^T (r + J d / 2) and candidate cost (Jacobians recomputed)   [thread / ray]
//   lm_post     step validity, tolerances, rho, accept/reject, radius              [1 block / scene]
//   (if accepted) cam_prep, lin_ray, lin_cam: re-linearise at the new point
// Observation records are 16 B (2 x f32 pixel, i32 camera, i32 ray); a workgroup of lin_ray/eval/backsub
// stages its scene's camera blocks (rotation, SO(3) Jacobian, intrinsics, Jacobi scales) in LDS once and
// every thread then reads them by camera id.  All reductions are fixed-order (bitwise reproducible).
#include <algorithm>
#include <cmath>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

#include "ptz_common.h"
#include "ptz_pool.h"
#include "ptz_factor.h"
#include "ptz_pass_shape.h"

#include "ptz_ba_kernels.h"
#include "ptz_view_kernels.h"
#include "ptz_ba_cov.h"
#include "ptz_ba_cov_georef.h"
#include "ptz_ba_resid.h"
#include <rocprim/rocprim.hpp>

namespace ptz {

// =============================================================================================================
// host side
// =============================================================================================================
enum ProfSlot { P_LIN = 0, P_LMCTL, P_RAYPREP, P_CLEAR, P_SCHUR, P_RHS, P_CHOL_PANEL, P_CHOL_SYRK, P_CHOL_BACK,
                P_BACKSUB, P_EVAL, P_SYNC, P_NSLOT };
static const char* kSlotNames[PTZ_PROF_SLOTS] = {"linearize", "lm_control", "ray_prep", "clear", "schur", "rhs",
                                                 "chol_panel", "chol_syrk", "chol_backsolve", "backsub", "eval",
                                                 "host_sync", "", "", "", ""};

}  // namespace ptz

using namespace ptz;

// chol_factor_solve split so that the three kernel families can be timed separately
namespace ptz {
void chol_factor_solve_profiled(const CholBatch& cb, double* x, hipStream_t stream, void* prof, bool fused, int path_count);
}

// The launch shape of one LM pass.  A batch keeps a ladder of them (ptz_ba_batch::shapes): full size, then compacted shapes of
// 2, 8, 32 ... slots, each with the workgroup size, the kernel variants and the factorisation path a batch of that size would get
// -- the stragglers of a 1000-scene batch then cost what a handful of scenes cost.  The ladder shape that covers the scenes last
// reported active gives a pass its VARIANT fields (everything below `path_slots`).  Its grid EXTENT is a separate matter
// (pass_extent, ptz_pass_shape.h): a pass replayed from a captured graph has the ladder shape's own extent; a pass enqueued launch
// by launch covers exactly the reported count, through the device's compacted list (blockIdx.y -> slot -> scene) as soon as one
// scene of the group has retired, so no workgroup is launched for a scene known to be finished.
struct PassShape {
  int slots = 0;          // grid extent over scenes
  int path_slots = 0;     // slot count of the ladder shape the variants come from: decides the factorisation path (chol_chain_fits)
  bool compact = false;   // blockIdx.y is a slot of the compacted list
  int ray_block = 1024;   // rays per workgroup of the ray-centric kernels
  bool small_blocks = false, fused = false;  // SMALL kernel variants; one-launch-per-column factorisation
  bool fuse_ctl = false;  // LM control and the camera update inside k_eval / k_lin_cam (no k_lm_pre / k_lm_post / k_cam_update launches)
  int eval_lanes = 1;     // lanes per ray in k_eval (4: the form of a few scenes, see k_eval)
  int max_chunk = 0;
  size_t lin_smem = 0, eval_smem = 0;
};

struct ptz_ba_batch {
  int n_scene = 0, type = 0, nc = 4, device = 0;
  std::vector<SceneDev> scenes;
  int total_cam = 0, total_ray = 0, total_obs = 0, total_pair = 0, total_ent = 0, total_run = 0, total_chunk = 0;  // total_chunk: partial-sum slots (waves of 64 rays + 1 per scene)
  int ray_block = RAY_BLOCK;
  bool schur_tg = false;         // a camera with more observations than k_schur's LDS table holds: table in global memory
  bool schur_w = false;          // PTZ_BA_SCHUR_W=1: round 2's Schur kernel over materialised W rows (kept for A/B measurements)
  bool schur_f = false;          // PTZRay, table in LDS: k_schur_f (factored 8-double rows, four workgroups per compute unit; PTZ_BA_SCHUR_F=0: k_schur)
  bool schur_wg4 = true;         // PTZ_BA_SCHUR_WG4=0: k_schur_f held at three workgroups per compute unit by its LDS request
  int schur_lds_ent = 0;         // entries of the camera list the Schur kernel stages in LDS (k_schur: max_cam_ent; k_schur_f: none)
  bool gtab = false;             // camera tables too large for LDS: the GTAB instantiations read them from global memory
  int n_group_hint(int n) const { if (const char* e = getenv("PTZ_BA_STREAMS")) return std::max(1, atoi(e)); return n >= 32 ? 2 : 1; }
  int max_cam = 0, max_ray = 0, max_chunk = 0, max_pair = 0, max_n = 0, max_cam_obs = 0, max_cam_ent = 0, max_cam_pair = 0, max_cam_run = 0;
  ptz_lm_options opt;
  Dev d;
  std::vector<void*> allocs;
  hipEvent_t create_ev = nullptr;    // end of ptz_ba_batch_create's work on `io`
  double* rkinv_dev = nullptr;       // ptz_ba_batch_set_state_pix2ray: the cameras' R^-1 K^-1 [9 total_cam]
  std::vector<void*> staged_pinned;  // staging blocks of uploads still in flight on `io` (released behind the next wait for it)
  void release_staged() { for (void* p : staged_pinned) ptzpool::pinned_release(p); staged_pinned.clear(); }
  hipStream_t stream = nullptr;   // stream of the group being enqueued (LAUNCH / prof_* use it)
  hipStream_t io = nullptr;       // uploads of ptz_ba_batch_create (before the group streams exist); see copy_on()
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // scenes are split into independent groups, one HIP stream each, so that the latency-bound kernels of one
  // group (diagonal-tile factorisation, back-substitution, LM control) overlap the throughput kernels of another
  int n_group = 1;
  std::vector<hipStream_t> streams;
  std::vector<hipEvent_t> fork_ev, join_ev;
  std::vector<int> group_first, group_count;
  std::vector<Dev> dg;
  // Cholesky look-ahead: one auxiliary stream and two events per group stream
  std::vector<hipStream_t> aux;
  std::vector<hipEvent_t> la_ev;
  bool lookahead = true;
  bool left_looking = true;  // left-looking column updates instead of right-looking trailing updates
  int group_of(hipStream_t st) const { for (size_t g = 0; g < streams.size(); ++g) if (streams[g] == st) return (int)g; return -1; }
  hipStream_t aux_stream(hipStream_t st) const { const int g = group_of(st); return (lookahead && g >= 0 && g < (int)aux.size()) ? aux[g] : nullptr; }
  void lookahead_events(hipStream_t st, hipEvent_t* t, hipEvent_t* r) const { const int g = group_of(st); *t = la_ev[2 * g]; *r = la_ev[2 * g + 1]; }
  // pass pipeline control (Dev::grp_ctl / host_ctl): 4 ints per scene group, device block + pinned host mirror
  int* d_ctl = nullptr;
  int* h_ctl = nullptr;      // pinned; read by the host while the device writes (fine-grained host memory)
  int* h_ctl_dev = nullptr;  // the device's address of h_ctl
  int ctl_groups = 0;        // groups the control blocks were sized for
  int ahead = 3;             // LM passes the host may have enqueued beyond the last one known to have reached its step evaluation
  // one captured LM pass per scene group (kernel arguments never change during a batch's life), replayed per pass
  bool use_graph = true;
  std::vector<PassShape> shapes;                        // [0] = full size, then compacted shapes by ascending slot count
  std::vector<std::vector<hipGraphExec_t>> pass_graph;  // [group][shape]
  int* d_act = nullptr;                                 // compacted scene lists, n_scene ints (each group its own range)
  bool compaction = true;
  bool exact_fit = true;                                // eagerly enqueued passes cover exactly the reported count (PTZ_BA_EXACT_FIT=0: the ladder's extents)
  double *cam0 = nullptr, *ray0 = nullptr, *tlw0 = nullptr;  // device copies of the initial state
  std::vector<int> sched_kmin;  // CholBatch::sched_kmin
  double* dsp0 = nullptr;  // PTZRayDistDisp: initial displacement block, one copy per camera (zeros unless ptz_ba_batch_set_disp)
  int has3d = 0, total_o3 = 0;
  // Rays are renumbered inside the library, longest track first (see build_pairs): ray_perm[ray_off + j] = the caller's
  // scene-local index of internal ray j.  set_state / get_state / linearize translate.
  std::vector<int> ray_perm;
  const int* d_ray_perm = nullptr;  // the same on the device (ptz_ba_batch_get_state gathers the result there)
  // shared intrinsics: per global camera, the global index of the first camera of its group (source of the initial values)
  std::vector<int> first_of_group;
  int max_grp = 0;
  bool has_state = false;
  bool views_mode = false;  // built by ptz_ba_batch_create_views: structure arrays at upper-bound extents, ray order on the device only
  int n_solves = 0;  // solves of this batch so far
  double last_ms = 0;
  // profiling
  bool profiling = false;
  std::vector<hipEvent_t> ev_pool;
  std::vector<std::pair<int, int>> ev_used;  // (slot, event index of the start; stop = +1)
  double prof_ms[PTZ_PROF_SLOTS] = {0};
  int64_t prof_n[PTZ_PROF_SLOTS] = {0};

  template <typename T> int alloc(T** p, size_t count)
  {
    void* q = nullptr;
    if (ptzpool::dev_acquire(device, sizeof(T) * std::max<size_t>(count, 1), &q) != hipSuccess) return PTZ_ENOMEM;
    allocs.push_back(q);
    *p = (T*)q;
    return PTZ_OK;
  }
  void prof_begin(int slot)
  {
    if (!profiling) return;
    if (ev_used.size() * 2 + 2 > ev_pool.size()) {
      for (int i = 0; i < 2; ++i) { hipEvent_t e; (void)ptzpool::event_acquire(device, true, &e); ev_pool.push_back(e); }
    }
    const int idx = (int)ev_used.size() * 2;
    ev_used.push_back({slot, idx});
    (void)hipEventRecord(ev_pool[idx], stream);
  }
  void prof_end()
  {
    if (!profiling) return;
    (void)hipEventRecord(ev_pool[ev_used.back().second + 1], stream);
  }
  void prof_collect()
  {
    for (auto& u : ev_used) {
      float ms = 0;
      if (hipEventElapsedTime(&ms, ev_pool[u.second], ev_pool[u.second + 1]) == hipSuccess) {
        prof_ms[u.first] += ms;
        prof_n[u.first] += 1;
      }
    }
    ev_used.clear();
  }
};

namespace {
// Elimination order of a reduced camera system at tile granularity.
//
// bisect_tiles: the tiles `ids` (natural numbers, ascending) with adjacency adj(a, e); looks for a separator made of a prefix
// [0, w1) and an interval [m, m + w2) of the list -- the two cuts of a ring whose images are numbered along it, or the middle
// cut of a band -- such that the rest falls apart; the parts are dealt to two lanes.  cls[i] = 0 / 1 (lane, 0 the longer) or
// 2 (separator).  The dependent chain of the factorisation of these tiles is then max(lane) + separator instead of their
// number; returns false unless that saves at least `min_saving`.
template <typename Adj>
inline bool bisect_tiles(const std::vector<int>& ids, Adj&& adj, int min_tiles, int min_saving, std::vector<int>& cls)
{
  const int nf = (int)ids.size();
  if (nf < min_tiles) return false;
  int best_cost = nf + 1;
  std::vector<int> comp(nf), stack;
  bool found = false;
  cls.assign(nf, 2);
  for (int w1 = 0; w1 <= 4; ++w1)
    for (int w2 = 0; w2 <= 4; ++w2)
      for (int m = w1; m + w2 <= nf; ++m) {
        if (w2 == 0 && m > w1) break;
        if (w1 + w2 == 0) continue;
        int ncomp = 0;  // tiles outside the separator: connected components
        for (int t = 0; t < nf; ++t) comp[t] = (t < w1 || (t >= m && t < m + w2)) ? -2 : -1;
        for (int t = 0; t < nf; ++t) {
          if (comp[t] != -1) continue;
          comp[t] = ncomp;
          stack.assign(1, t);
          while (!stack.empty()) {
            const int u = stack.back(); stack.pop_back();
            for (int v = 0; v < nf; ++v)
              if (comp[v] == -1 && adj(ids[u], ids[v])) { comp[v] = ncomp; stack.push_back(v); }
          }
          ++ncomp;
        }
        if (ncomp < 2) continue;
        std::vector<int> size(ncomp, 0), order(ncomp);
        for (int t = 0; t < nf; ++t) if (comp[t] >= 0) ++size[comp[t]];
        for (int c = 0; c < ncomp; ++c) order[c] = c;
        std::stable_sort(order.begin(), order.end(), [&](int a, int e) { return size[a] > size[e]; });
        int la = 0, lb = 0;
        std::vector<int> lane_of(ncomp);
        for (int c : order) { if (la <= lb) { lane_of[c] = 0; la += size[c]; } else { lane_of[c] = 1; lb += size[c]; } }
        const int cost = std::max(la, lb) + (w1 + w2);
        if (cost > nf - min_saving || cost >= best_cost) continue;
        found = true;
        best_cost = cost;
        const int big = la >= lb ? 0 : 1;  // lane 0 is the longer one
        for (int t = 0; t < nf; ++t) cls[t] = comp[t] < 0 ? 2 : (lane_of[comp[t]] == big ? 0 : 1);
      }
  return found;
}

// m0: lower-triangular tile adjacency (nt x nt, natural order, not closed under fill); tiles >= first_dense (T_l_w block, rhs
// row, padding) stay last, in place.  The free tiles are bisected, and each lane once more when that shortens it (a band of
// four tiles with two sub-diagonals: ends first, middle after): the order is lane 0 (its parts, its separator), lane 1, the
// top separator, the tail.  Which block columns can then be factored side by side is read off the filled structure
// (level_schedule); perm[t] = position of natural tile t; lanes at positions [0, lane_a) and [lane_a, lane_a + lane_b).
// Returns false (natural order) unless the top-level bisection shortens the chain by two or more.
inline bool plan_dissection(int nt, int first_dense, const unsigned char* m0, int* perm, int* lane_a, int* lane_b, bool nested = true)
{
  const int nf = std::min(first_dense, nt);
  auto adj = [&](int a, int e) { return a == e ? false : (a > e ? m0[a * nt + e] : m0[e * nt + a]) != 0; };
  std::vector<int> ids(nf), cls;
  for (int t = 0; t < nf; ++t) ids[t] = t;
  if (!bisect_tiles(ids, adj, 6, 2, cls)) return false;
  int pos = 0, n_lane[2] = {0, 0};
  for (int lane = 0; lane < 2; ++lane) {
    std::vector<int> mine, sub;
    for (int t = 0; t < nf; ++t) if (cls[t] == lane) mine.push_back(t);
    n_lane[lane] = (int)mine.size();
    if (nested && bisect_tiles(mine, adj, 4, 1, sub)) {
      for (int pass = 0; pass < 3; ++pass)
        for (size_t k = 0; k < mine.size(); ++k) if (sub[k] == pass) perm[mine[k]] = pos++;
    }
    else for (int t : mine) perm[t] = pos++;
  }
  for (int t = 0; t < nf; ++t) if (cls[t] == 2) perm[t] = pos++;
  for (int t = nf; t < nt; ++t) perm[t] = pos++;
  *lane_a = n_lane[0]; *lane_b = n_lane[1];
  return true;
}

// Steps of the factorisation from the FILLED tile structure m (nt x nt, lower, in elimination order): block column t can be
// factored once every column k < t with m[t][k] != 0 is done, so its step is one more than the largest of theirs; columns of
// one step neither depend on nor couple with each other.  sched[step * CHOL_STEP_COLS + slot] = column or -1, ascending inside
// a step.  A step with more than CHOL_STEP_COLS columns spills its extra columns into later steps (still correct: a column
// may always be factored later than its earliest step as long as its dependants move with it -- so the levels are recomputed
// with the spilled columns' new steps).  Returns the number of steps.
inline int level_schedule(int nt, const unsigned char* m, int* sched)
{
  std::vector<int> level(nt, 0), used(nt + 1, 0);
  for (int t = 0; t < nt; ++t) {
    int lv = 0;
    for (int k = 0; k < t; ++k)
      if (m[t * nt + k]) lv = std::max(lv, level[k] + 1);
    while (used[lv] >= CHOL_STEP_COLS) ++lv;  // (levels are at most nt - 1: column t has at most t predecessors)
    level[t] = lv;
    ++used[lv];
  }
  int steps = 0;
  for (int t = 0; t < nt; ++t) steps = std::max(steps, level[t] + 1);
  for (int i = 0; i < nt * CHOL_STEP_COLS; ++i) sched[i] = -1;
  std::vector<int> fill(steps, 0);
  for (int t = 0; t < nt; ++t) sched[level[t] * CHOL_STEP_COLS + fill[level[t]]++] = t;
  return steps;
}

// The tile mask `mask` in the elimination order `perm` (nullptr: the natural order), closed under the fill of the right-looking
// factorisation, into the zeroed `m`; and the steps: from the filled structure when an order was planned, one block column after
// the other otherwise.  Returns the number of steps.
inline int fill_and_schedule(int nt, const unsigned char* mask, const int* perm, unsigned char* m, int* sched)
{
  for (int a = 0; a < nt; ++a)
    for (int e = 0; e <= a; ++e) {
      if (!mask[a * nt + e]) continue;
      const int pa = perm ? perm[a] : a, pe = perm ? perm[e] : e;
      m[std::max(pa, pe) * nt + std::min(pa, pe)] = 1;
    }
  for (int k = 0; k < nt; ++k)
    for (int x = k + 1; x < nt; ++x) {
      if (!m[x * nt + k]) continue;
      for (int y = k + 1; y <= x; ++y)
        if (m[y * nt + k]) m[x * nt + y] = 1;
    }
  if (perm) return level_schedule(nt, m, sched);
  for (int i = 0; i < nt * CHOL_STEP_COLS; ++i) sched[i] = -1;
  for (int t = 0; t < nt; ++t) sched[CHOL_STEP_COLS * t] = t;
  return nt;
}

// threads of a k_schur workgroup = the most runs a camera's entries are cut into (ptz_ba_kernels.h schur_threads<TYPE>())
inline int schur_threads_of(int factor_type) { (void)factor_type; return 256; }

// LDS a k_schur_f<TYPE, false> workgroup may ask for and still be resident four times per compute unit (160 KB / 4: 561 rows at C4)
constexpr size_t SCHUR_F_WG4_LDS = 160 * 1024 / 4;

// NW: camera columns with a 2D-2D Jacobian (Dims<TYPE>::NW); max_ent: entries of the largest camera's list where the kernel
// stages it in LDS (k_schur; 0 for k_schur_f, which reads its runs from global memory)
inline size_t schur_lds_bytes(int max_obs, int NC, int np, bool legacy, int threads, int NW = 0, int max_ent = 0, int row = 0)
{
  // legacy (k_schur_w): T rows of the largest camera, the reduction strip, the scene's tile order (one int per 64 columns)
  if (legacy) return sizeof(double) * ((size_t)max_obs * NC * 3 + (size_t)(SCHUR_THREADS / 64) * (NC + NC * (NC + 1) / 2) + (size_t)(np / CHOL_NB + 1) / 2 + 1);
  // k_schur: the reduction strip, the tile order, then ONE region that first holds, per observation of the largest camera, its T'
  // row and the ray's direction (NW * 3 + 3 doubles rounded up to an odd count, NW <= NC) and later one sum per run (NW^2 | 1)
  if (NW <= 0) NW = NC;
  const size_t table = (size_t)max_obs * (row > 0 ? row : ((NW * 3 + 3) | 1)), sums = (size_t)threads * ((NW * NW) | 1);  // row > 0: k_schur_f's factored rows
  return sizeof(double) * ((size_t)(threads / 64) * (NW + NW * (NW + 1) / 2) + (size_t)(np / CHOL_NB + 2) / 2 + std::max(table, sums) + 2) +
         2 * (size_t)((max_ent + 3) & ~3);
}

// The dynamic LDS a batch's Schur launches ask for (the pass launches and the residency line of PTZ_BA_DEBUG_TIMING): the batch's
// kernel and table home, and PTZ_BA_SCHUR_WG4=0 -- k_schur_f<TYPE, false> is resident four times per compute unit up to
// SCHUR_F_WG4_LDS bytes, the switch asks for 1 KB more
inline size_t schur_launch_lds(const ptz_ba_batch* b, int NC, int NW, int np, int threads)
{
  const size_t smem = schur_lds_bytes(b->schur_tg ? 0 : b->max_cam_obs, NC, np, b->schur_w, threads, NW, b->schur_lds_ent, b->schur_f ? SCHUR_F_ROW : 0);
  return b->schur_f && !b->schur_tg && !b->schur_wg4 ? std::max(smem, SCHUR_F_WG4_LDS + 1024) : smem;
}

// Every host <-> device copy of a batch goes through a stream of its own and waits for THAT stream only.  hipMemcpy / hipMemset
// run on the null stream, which synchronises with every other (blocking) stream of the process: batches driven from several
// host threads (the lock-step PTZ-IBA, ptz_ba_solve_sharded's dealers) then wait for each other's solves inside their copies.
inline hipError_t copy_on(hipStream_t st, void* dst, const void* src, size_t bytes, hipMemcpyKind kind)
{
  if (bytes == 0) return hipSuccess;
  // small copies go through a pinned block of the pool: an asynchronous copy from / to pageable memory waits inside the runtime
  // (the same interrupt-driven wait stream_wait() avoids); large ones keep the direct path, their transfer time dominates
  void* pin = nullptr;
  if (bytes <= ((size_t)16 << 20) && ptzpool::pinned_acquire(bytes, &pin) == hipSuccess) {
    hipError_t e;
    if (kind == hipMemcpyHostToDevice) {
      memcpy(pin, src, bytes);
      e = hipMemcpyAsync(dst, pin, bytes, kind, st);
      if (e == hipSuccess) e = stream_wait(st);
    }
    else {
      e = hipMemcpyAsync(pin, src, bytes, kind, st);
      if (e == hipSuccess) e = stream_wait(st);
      if (e == hipSuccess) memcpy(dst, pin, bytes);
    }
    ptzpool::pinned_release(pin);
    return e;
  }
  (void)hipGetLastError();
  hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, st);
  if (e == hipSuccess) e = stream_wait(st);
  return e;
}

template <typename T> int upload(ptz_ba_batch* b, const std::vector<T>& h, const T** dev)
{
  T* p = nullptr;
  int rc = b->alloc(&p, h.size());
  if (rc) return rc;
  if (copy_on(b->io, p, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice) != hipSuccess) return PTZ_ENODEVICE;
  *dev = p;
  return PTZ_OK;
}

// Many small host arrays -> ONE device block through ONE pinned staging buffer and one copy (a synchronous hipMemcpy from
// pageable memory costs 10-15 us each whatever its size; a batch has about twenty of them).  Large batches, whose structure
// would need a staging buffer of more than 64 MB, keep the per-array uploads.
// std::vector whose resize() leaves trivially-constructible elements uninitialised (the batch-wide observation arrays are
// sized once and then filled in place by the builder threads; zero-filling 600 MB first costs more than building them)
template <typename T> struct NoInitAlloc : std::allocator<T> {
  template <typename U> struct rebind { using other = NoInitAlloc<U>; };
  template <typename U> void construct(U* p) noexcept { ::new (static_cast<void*>(p)) U; }
  template <typename U, typename... A> void construct(U* p, A&&... a) { ::new (static_cast<void*>(p)) U(std::forward<A>(a)...); }
};
template <typename T> using RawVec = std::vector<T, NoInitAlloc<T>>;

struct StagedUpload {
  struct Item { const void* src; size_t bytes; const void** dst; };
  std::vector<Item> items;
  template <typename T, typename A> void add(const std::vector<T, A>& h, const T** dev)
  {
    items.push_back({h.data(), sizeof(T) * h.size(), reinterpret_cast<const void**>(dev)});
  }
  // wait = false: the copy is left in flight on b->io (kernels enqueued there see the data; the caller's next wait for that stream
  // -- followed by b->release_staged() -- ends it)
  int commit(ptz_ba_batch* b, bool wait = true)
  {
    auto up = [](size_t x) { return (std::max<size_t>(x, 1) + 255) & ~(size_t)255; };
    size_t total = 0;
    for (const Item& it : items) total += up(it.bytes);
    void* pinned = nullptr;
    if (total > ((size_t)64 << 20) || ptzpool::pinned_acquire(total, &pinned) != hipSuccess) {
      (void)hipGetLastError();
      for (const Item& it : items) {
        char* p = nullptr;
        int rc = b->alloc(&p, it.bytes);
        if (rc) return rc;
        if (copy_on(b->io, p, it.src, it.bytes, hipMemcpyHostToDevice) != hipSuccess) return PTZ_ENODEVICE;
        *it.dst = p;
      }
      return PTZ_OK;
    }
    char* dev = nullptr;
    int rc = b->alloc(&dev, total);
    if (rc) { ptzpool::pinned_release(pinned); return rc; }
    size_t off = 0;
    for (const Item& it : items) {
      if (it.bytes) memcpy((char*)pinned + off, it.src, it.bytes);
      *it.dst = dev + off;
      off += up(it.bytes);
    }
    hipError_t e = hipMemcpyAsync(dev, pinned, total, hipMemcpyHostToDevice, b->io);
    if (e == hipSuccess && !wait) { b->staged_pinned.push_back(pinned); return PTZ_OK; }
    if (e == hipSuccess) e = stream_wait(b->io);
    ptzpool::pinned_release(pinned);
    return e == hipSuccess ? PTZ_OK : PTZ_ENODEVICE;
  }
};

#define LAUNCH(kern, grid, block, smem, ...) ptz::launch(kern, grid, block, smem, b->stream, __VA_ARGS__)
// the ray-centric kernels come in four shapes: small / large workgroups x camera tables staged in LDS / read from global memory
#define PTZ_LAUNCH_RAY(kern, grid, smem, dev)                                                                       \
  do {                                                                                                              \
    if (sh.small_blocks) {                                                                                          \
      if (b->gtab) LAUNCH((kern<TYPE, true, true>), grid, dim3(sh.ray_block), smem, dev);                           \
      else LAUNCH((kern<TYPE, true, false>), grid, dim3(sh.ray_block), smem, dev);                                  \
    }                                                                                                               \
    else {                                                                                                          \
      if (b->gtab) LAUNCH((kern<TYPE, false, true>), grid, dim3(sh.ray_block), smem, dev);                          \
      else LAUNCH((kern<TYPE, false, false>), grid, dim3(sh.ray_block), smem, dev);                                 \
    }                                                                                                               \
  } while (0)

inline double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// run-time switches: read where they are used, on every create (tests change them between two creates of one process)
inline bool env_flag(const char* name, bool dflt) { const char* e = getenv(name); return e ? atoi(e) != 0 : dflt; }
inline int env_int(const char* name, int dflt, int lo) { const char* e = getenv(name); return e ? std::max(lo, atoi(e)) : dflt; }

// fn(first, step) on nt threads, the caller's among them
template <typename F> void run_strided(int nt, F&& fn)
{
  if (nt <= 1) { fn(0, 1); return; }
  std::vector<std::thread> th;
  for (int t = 1; t < nt; ++t) th.emplace_back(fn, t, nt);
  fn(0, nt);
  for (auto& x : th) x.join();
}

// FNV-1a, the hash of the structure diagnostics
constexpr uint64_t FNV_BASIS = 1469598103934665603ull;
inline void fnv_mix(uint64_t& h, const void* ptr, size_t bytes) { for (size_t i = 0; i < bytes; ++i) { h ^= ((const unsigned char*)ptr)[i]; h *= 1099511628211ull; } }

// A batch under construction (and the one-shot solves' batch): every way out destroys it, a half-built one included --
// ptz_ba_batch_destroy and the pool's releases take null members
struct BatchDeleter { void operator()(ptz_ba_batch* b) const { ptz_ba_batch_destroy(b); } };
using BatchOwner = std::unique_ptr<ptz_ba_batch, BatchDeleter>;
// (the creation path's early return; no clean-up hides in it, the owner does that)
#define PTZ_TRY(x) do { if (const int32_t rc_ = (x)) return rc_; } while (0)

// rays per workgroup of the ray-centric kernels: one rig's ~13 k rays on 1024-ray workgroups keep 14 compute units busy,
// so a few scenes use small workgroups; large batches amortise the LDS camera tables over many rays (results do not
// depend on it: per-ray sums are reduced per wave of 64 rays)
inline int ray_block_for(int slots)
{
  if (const char* e = getenv("PTZ_BA_RAY_BLOCK")) return std::min(RAY_BLOCK, std::max(64, (atoi(e) / 64) * 64));
  return slots <= 4 ? 128 : (slots <= 32 ? 256 : RAY_BLOCK);
}

// The cap on dynamic LDS is a property of the kernel, not of a batch: each set of kernels has its caps raised ONCE per device, so
// that batches of different sizes can live side by side (a per-batch value would let a small batch created later lower the cap
// under a large one), and because hipFuncSetAttribute under a lock on every batch creation was a measurable share of a view
// batch's 0.4 ms of enqueueing in the 64-rig lock step.  A set whose `raise` returns false stays undone: the next create tries again.
enum CapSet { CAPS_PAIRS, CAPS_VIEW_SORT, CAPS_PASS, CAP_SETS };
static bool once_per_device(CapSet set, int device, bool (*raise)())
{
  static std::mutex mu;
  static std::vector<char> done[CAP_SETS];
  std::lock_guard<std::mutex> lk(mu);
  if ((int)done[set].size() <= device) done[set].resize(device + 1, 0);
  if (!done[set][device] && raise()) done[set][device] = 1;
  return done[set][device] != 0;
}

// k_pairs' dynamic LDS beyond 64 KiB (very wide rigs)
static bool raise_pairs_caps()
{
  (void)hipFuncSetAttribute((const void*)k_pairs<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 64);
  (void)hipFuncSetAttribute((const void*)k_pairs<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 64);
  return true;
}

template <int TYPE> void enqueue_linearize(ptz_ba_batch* b)
{
  const Dev& d = b->d;
  const PassShape& sh = b->shapes[0];
  b->prof_begin(P_LIN);
  LAUNCH(k_cam_prep<TYPE>, dim3((b->max_cam + 63) / 64, b->n_scene), dim3(64), 0, d);
  PTZ_LAUNCH_RAY(k_lin_ray, dim3(sh.max_chunk, b->n_scene), sh.lin_smem, d);
  if (d.W) LAUNCH((k_lin_cam<TYPE, true>), dim3((b->max_cam + 3) / 4, b->n_scene), dim3(256), 0, d);  // parity tests / legacy Schur path
  else LAUNCH((k_lin_cam<TYPE, false>), dim3((b->max_cam + 3) / 4, b->n_scene), dim3(256), 0, d);
  if (Dims<TYPE>::HAS3D) LAUNCH(k_lin_3d<TYPE>, dim3(b->n_scene), dim3(256), 0, d);
  if (d.shared) LAUNCH(k_group_grad<TYPE>, dim3(b->n_scene), dim3(256), 0, d);
  b->prof_end();
}

static void make_groups(ptz_ba_batch* b)
{
  const int B = b->n_scene;
  // per-family timings are only meaningful when no other group's kernels share the device: profiling runs one group
  const int G = b->profiling ? 1 : std::max(1, std::min(std::min(b->n_group, B), b->ctl_groups));
  b->group_first.clear(); b->group_count.clear(); b->dg.clear();
  for (int g = 0; g < G; ++g) {
    const int lo = (int)((int64_t)B * g / G), hi = (int)((int64_t)B * (g + 1) / G);
    b->group_first.push_back(lo);
    b->group_count.push_back(hi - lo);
    Dev d = b->d;  // per-scene arrays are re-based; everything else is addressed through SceneDev offsets
    const size_t np = d.chol.np, nt = np / CHOL_NB;
    d.n_scene = hi - lo;
    d.scene += lo; d.lm += lo; d.active += lo; d.ray_fail += lo; d.tail_cnt += 2 * (size_t)lo;
    d.yc += (size_t)lo * np;
    d.chol.count = hi - lo;
    d.chol.A += (size_t)lo * np * np;
    if (d.chol.Linv) d.chol.Linv += (size_t)lo * nt * CHOL_NB * CHOL_NB;
    d.chol.Ldiag += (size_t)lo * nt * CHOL_NB * CHOL_NB;
    d.chol.Dinv += (size_t)lo * nt * 4 * 16 * 16;
    d.chol.n += lo; d.chol.fail += lo; d.chol.active = d.active;
    if (d.chol.tmask) d.chol.tmask += (size_t)lo * nt * nt;
    if (d.chol.sched) d.chol.sched += (size_t)lo * nt * CHOL_STEP_COLS;
    if (d.tperm) { d.tperm += (size_t)lo * nt; d.chol.xperm = d.tperm; }
    d.grp_ctl = b->d_ctl + 4 * g;
    d.host_ctl = b->h_ctl_dev + 4 * g;
    d.act = b->d_act + lo;
    d.use_act = 0;
    if (d.chol.L) d.chol.L = b->d.chol.L + (size_t)g * std::min(b->n_scene, CHOL_CHAIN_SLOTS) * np * np;  // slots of finished L tiles per group
    if (d.chol.chain_ctl) d.chol.chain_ctl = b->d.chol.chain_ctl + (size_t)g * chol_chain_ctl_ints((int)np);  // (a block per stream)
    if (d.chol.bs_items) { d.chol.bs_items += (size_t)lo * 4 * chol_backsolve_max_groups((int)np); d.chol.bs_groups += lo; }
    b->dg.push_back(d);
  }
  if ((int)b->pass_graph.size() != G || (G > 0 && b->pass_graph[0].size() != b->shapes.size())) {  // the grouping changed (profiling on / off): recorded passes are stale
    for (auto& v : b->pass_graph) for (auto ge : v) if (ge) (void)hipGraphExecDestroy(ge);
    b->pass_graph.assign(G, std::vector<hipGraphExec_t>(b->shapes.size(), nullptr));
  }
  while ((int)b->streams.size() < G) {
    hipStream_t st; (void)ptzpool::stream_acquire(b->device, &st); b->streams.push_back(st);
    hipEvent_t e1, e2; (void)ptzpool::event_acquire(b->device, false, &e1); (void)ptzpool::event_acquire(b->device, false, &e2);
    b->fork_ev.push_back(e1); b->join_ev.push_back(e2);
    hipStream_t ax; (void)ptzpool::stream_acquire(b->device, &ax); b->aux.push_back(ax);
    hipEvent_t e3, e4; (void)ptzpool::event_acquire(b->device, false, &e3); (void)ptzpool::event_acquire(b->device, false, &e4);
    b->la_ev.push_back(e3); b->la_ev.push_back(e4);
  }
}

// What a pass's kernels are given: the group's Dev with the launch shape's fields set.  fast / fuse: see enqueue_pass.
template <int TYPE> Dev pass_dev(const ptz_ba_batch* b, const Dev& dgrp, const PassShape& sh, bool* fast_out = nullptr, bool* fuse_out = nullptr)
{
  Dev d = dgrp;
  d.use_act = sh.compact ? 1 : 0;
  d.ray_block = sh.ray_block;
  d.chol.count = sh.slots;
  d.chol.act = sh.compact ? d.act : nullptr;
  d.chol.act_n = d.grp_ctl + 2;
  if (!sh.fused) d.chol.L = nullptr;  // (the second matrix marks the one-launch-per-column path)
  // Scenes without annotation residuals and shared blocks: the camera-side linearisation of the CANDIDATE is evaluated before the
  // step is judged (k_lin_cam, Dev::spec_lin), and one control point per pass judges the step and opens the next iteration
  // (lm_step_wave) -- a launch of its own (k_lm_step), or in launch shapes of a few scenes the tail of k_lin_cam (Dev::fuse_ctl, with
  // the camera update in k_eval's prologue).  The others keep k_lm_post / k_lin_cam at the accepted point / k_lm_pre.
  // (Not for large launch shapes: there the speculative linearisation of the steps that end up rejected costs more than the second
  //  control launch it saves -- C4: linearise 19 -> 27 ms per solve against 3 ms of control.  Both forms take the same decisions
  //  with the same bits, so a scene may change between them from pass to pass.  Round 2's Schur kernel reads W rows of the
  //  CURRENT point, which are not double-buffered.)
  const bool fast = TYPE < 3 && !d.shared && !b->schur_w && sh.fuse_ctl;
  const bool fuse = sh.fuse_ctl && fast;
  d.spec_lin = fast ? 1 : 0;
  d.fuse_ctl = fuse ? 1 : 0;
  if (fast_out) *fast_out = fast;
  if (fuse_out) *fuse_out = fuse;
  return d;
}

// Which Schur kernel a launch took (ptz_debug_batch_reduced_system reports it): 0 k_schur_w, 1 k_schur, 2 k_schur_f
struct SchurLaunch { int kernel = -1, threads = 0; };

// The reduced camera system of the scenes of one pass, enqueued on b->stream: ray preparation (LM diagonal, E blocks, the system's
// structural tiles cleared) and the Schur kernel of the batch.  `d` is pass_dev()'s.  One body for the solver's passes and for
// ptz_debug_batch_reduced_system, which reads back what these launches leave.
template <int TYPE> SchurLaunch enqueue_reduced_system(ptz_ba_batch* b, const Dev& d, const PassShape& sh)
{
  constexpr int NC = Dims<TYPE>::NC;
  const int B = sh.slots;
  hipStream_t st = b->stream;
  SchurLaunch sl;
  const int schur_thr = schur_threads<TYPE>();
  const size_t schur_smem = schur_launch_lds(b, NC, Dims<TYPE>::NW, d.chol.np, schur_thr);
  b->prof_begin(P_RAYPREP);
  {
    const int nt = d.chol.np / CHOL_NB;
    const int per = std::max(1, sh.ray_block / 256);  // tiles of the lower triangle a workgroup clears
    if (d.chol.tmask) LAUNCH(k_ray_prep<TYPE>, dim3(sh.max_chunk + (nt * (nt + 1) / 2 + per - 1) / per, B), dim3(sh.ray_block), 0, d, sh.max_chunk);
    else {  // dense debugging path (PTZ_BA_DENSE_CHOL): whole matrices zeroed by a memset
      LAUNCH(k_ray_prep<TYPE>, dim3(sh.max_chunk, B), dim3(sh.ray_block), 0, d, sh.max_chunk);
      chol_clear(d.chol, st);
    }
  }
  if (d.shared) LAUNCH(k_group_diag<TYPE>, dim3(b->max_grp * NC, B), dim3(64), 0, d);
  b->prof_end();
  b->prof_begin(P_SCHUR);
  if (b->schur_w) {
    sl.kernel = 0; sl.threads = SCHUR_THREADS;
    if (b->schur_tg) LAUNCH((k_schur_w<TYPE, true>), dim3(b->max_cam, B), dim3(SCHUR_THREADS), schur_smem, d);
    else LAUNCH((k_schur_w<TYPE, false>), dim3(b->max_cam, B), dim3(SCHUR_THREADS), schur_smem, d);
  }
  else if (b->schur_f) {
    if constexpr (Dims<TYPE>::FACTOR == 0) {
      sl.kernel = 2; sl.threads = 256;
      if (b->schur_tg) LAUNCH((k_schur_f<TYPE, true>), dim3(b->max_cam, B), dim3(256), schur_smem, d);
      else LAUNCH((k_schur_f<TYPE, false>), dim3(b->max_cam, B), dim3(256), schur_smem, d);
    }
  }
  else {
    sl.kernel = 1; sl.threads = schur_thr;
    if (b->schur_tg) LAUNCH((k_schur<TYPE, true>), dim3(b->max_cam, B), dim3(schur_thr), schur_smem, d);
    else LAUNCH((k_schur<TYPE, false>), dim3(b->max_cam, B), dim3(schur_thr), schur_smem, d);
  }
  if (Dims<TYPE>::HAS3D) LAUNCH(k_schur_3d<TYPE>, dim3(B), dim3(64), 0, d);
  if (d.shared) LAUNCH(k_fold_system<TYPE>, dim3(B), dim3(1024), sizeof(double) * (size_t)(b->max_n + 4) + (size_t)(d.chol.np / CHOL_NB) * (d.chol.np / CHOL_NB), d);
  b->prof_end();
  return sl;
}

// one LM pass of one group in launch shape `sh`, enqueued on b->stream; returns after enqueueing (no synchronisation).
// A pass = one trust-region step and the bookkeeping that OPENS the next one (k_lm_pre last: the first iteration is opened by
// solve_impl's prologue), so that launch shapes with and without launches of their own for LM control can follow one another.
template <int TYPE> void enqueue_pass(ptz_ba_batch* b, const Dev& dgrp, const PassShape& sh)
{
  bool fast = false, fuse = false;
  const Dev d = pass_dev<TYPE>(b, dgrp, sh, &fast, &fuse);
  const int path_slots = sh.path_slots > 0 ? sh.path_slots : sh.slots;
  const int B = sh.slots;
  hipStream_t st = b->stream;
  enqueue_reduced_system<TYPE>(b, d, sh);
  chol_factor_solve_profiled(d.chol, d.yc, st, b, sh.fused, path_slots);
  if (d.shared) LAUNCH(k_group_expand<TYPE>, dim3(B), dim3(256), 0, d);
  if (!fuse) {
    b->prof_begin(P_BACKSUB);
    LAUNCH(k_cam_update<TYPE>, dim3((b->max_cam + 63) / 64, B), dim3(64), 0, d);
    b->prof_end();
  }
  b->prof_begin(P_EVAL);
  if constexpr (TYPE < 3) {
    if (fuse && sh.eval_lanes == 4) LAUNCH((k_eval<TYPE, true, false, true, 4>), dim3(sh.max_chunk, B), dim3(sh.ray_block * 4), sh.eval_smem, d);
    else if (fuse) LAUNCH((k_eval<TYPE, true, false, true>), dim3(sh.max_chunk, B), dim3(sh.ray_block), sh.eval_smem, d);
    else PTZ_LAUNCH_RAY(k_eval, dim3(sh.max_chunk, B), sh.eval_smem, d);
  }
  else PTZ_LAUNCH_RAY(k_eval, dim3(sh.max_chunk, B), sh.eval_smem, d);
  if (Dims<TYPE>::HAS3D) LAUNCH(k_eval_3d<TYPE>, dim3(B), dim3(256), 0, d);
  b->prof_end();
  if (!fast) {
    b->prof_begin(P_LMCTL);
    LAUNCH(k_lm_post<TYPE>, dim3(B), dim3(LM_THREADS), 0, d);
    b->prof_end();
  }
  {
    const Dev& dd = d;
    b->prof_begin(P_LIN);
    // (no k_lin_ray inside a pass: the ray side of an accepted step's linearisation was left by k_eval's second pass,
    //  LmState::ray_lin_ready; k_lin_ray runs for iteration zero only, enqueue_linearize)
    if (dd.W && b->schur_w) LAUNCH((k_lin_cam<TYPE, true>), dim3((b->max_cam + 3) / 4, B), dim3(256), 0, dd);
    else LAUNCH((k_lin_cam<TYPE, false>), dim3((b->max_cam + 3) / 4, B), dim3(256), 0, dd);
    if (Dims<TYPE>::HAS3D) LAUNCH(k_lin_3d<TYPE>, dim3(B), dim3(256), 0, dd);
    if (dd.shared) LAUNCH(k_group_grad<TYPE>, dim3(B), dim3(256), 0, dd);
    b->prof_end();
  }
  b->prof_begin(P_LMCTL);
  if (!fast) LAUNCH(k_lm_pre<TYPE>, dim3(B), dim3(LM_THREADS), 0, d);
  else if (!fuse) LAUNCH(k_lm_step<TYPE>, dim3(B), dim3(LM_THREADS), 0, d);
  if (b->shapes.size() > 1 && b->compaction) LAUNCH(k_compact, dim3(1), dim3(1024), 0, d);  // (batches too small for a compacted shape skip it)
  b->prof_end();
}

// ---- the prologue of a solve, in the pieces ptz_debug_batch_reduced_system runs too ----
// The scene groups and their control words on the host: nothing of this batch is in flight.  Leaves b->stream = stream 0.
static void begin_solve(ptz_ba_batch* b)
{
  make_groups(b);
  const int G = (int)b->dg.size();
  b->stream = b->streams[0];
  for (int i = 0; i < 4 * b->ctl_groups; ++i) __atomic_store_n(&b->h_ctl[i], 0, __ATOMIC_RELEASE);  // nothing of this batch is in flight
  for (int g = 0; g < G; ++g) __atomic_store_n(&b->h_ctl[4 * g + 2], b->group_count[g], __ATOMIC_RELEASE);
}

// x <- initial state, scales <- 1, LM state reset (whole batch, stream 0)
template <int TYPE> void enqueue_solve_init(ptz_ba_batch* b)
{
  constexpr int NC = Dims<TYPE>::NC;
  const Dev& d = b->d;
  const int B = b->n_scene;
  const size_t n15 = (size_t)15 * b->total_cam, n3 = (size_t)3 * b->total_ray, nnc = (size_t)b->total_cam * NC;
  const size_t most = std::max(std::max(n15, n3), std::max(std::max(nnc, (size_t)6 * B), d.dsp_x ? d.dsp_stride : (size_t)0));
  LAUNCH(k_solve_init, dim3((unsigned)((most + 255) / 256)), dim3(256), 0, d, (const double*)b->cam0, (const double*)b->ray0, (const double*)b->dsp0,
         (const double*)b->tlw0, n15, n3, nnc);
}

// The groups' control words on the device; then iteration zero's books are closed and the first step is opened (every pass ends
// with the same bookkeeping for the next)
template <int TYPE> void enqueue_open_first_step(ptz_ba_batch* b)
{
  const int G = (int)b->dg.size();
  for (int g = 0; g < G; ++g) hipLaunchKernelGGL(k_ctl_reset, dim3(1), dim3(64), 0, b->stream, b->dg[g]);
  b->prof_begin(P_LMCTL);
  for (int g = 0; g < G; ++g) {
    LAUNCH(k_lm_pre<TYPE>, dim3(b->group_count[g]), dim3(LM_THREADS), 0, b->dg[g]);
    if (b->shapes.size() > 1 && b->compaction) LAUNCH(k_compact, dim3(1), dim3(1024), 0, b->dg[g]);
  }
  b->prof_end();
}

template <int TYPE> int solve_impl(ptz_ba_batch* b, ptz_lm_summary* out)
{
  constexpr int NC = Dims<TYPE>::NC;
  const Dev& d = b->d;
  const int B = b->n_scene;
  const bool dbg = getenv("PTZ_BA_DEBUG_TIMING") != nullptr;
  auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double t_start = now();
  double t_enq = 0, t_sync = 0;
  begin_solve(b);
  const int G = (int)b->dg.size();
  hipStream_t s0 = b->streams[0];
  PTZ_HIP_TRY(hipEventRecord(b->ev0, s0));
  enqueue_solve_init<TYPE>(b);
  // IterationZero: evaluate, Jacobi scales from the column norms, re-evaluate scaled
  enqueue_linearize<TYPE>(b);
  if (b->opt.jacobi_scaling) {
    LAUNCH(k_jacobi_scale<TYPE>, dim3((std::max(b->max_cam, b->max_ray) + 255) / 256, B), dim3(256), 0, d);
    if (d.shared) LAUNCH(k_group_scale<TYPE>, dim3(b->max_grp * NC, B), dim3(64), 0, d);
    enqueue_linearize<TYPE>(b);
  }
  enqueue_open_first_step<TYPE>(b);
  // fork: every group's stream continues after the common prologue
  PTZ_HIP_TRY(hipEventRecord(b->fork_ev[0], s0));
  for (int g = 1; g < G; ++g) PTZ_HIP_TRY(hipStreamWaitEvent(b->streams[g], b->fork_ev[0], 0));
  const int max_it = b->opt.max_num_iterations;
  // Every group runs its own pass pipeline and the host is not part of it: LM control lives on the device (k_lm_pre /
  // k_lm_post), every kernel of a pass returns at once for a scene that has terminated, so the host simply keeps `ahead`
  // passes enqueued beyond the last one the device is known to have reached, and stops when the device reports that the
  // group's last scene has retired (two words in pinned memory per group, polled; no stream synchronisation, no copy).
  // Passes enqueued past that point are empty launches.  Groups drift out of phase, so the latency-bound part of one
  // group's pass (block-column chain of the factorisation, LM control) overlaps the throughput kernels of another.
  // (a batch's FIRST solve enqueues its passes eagerly: recording and instantiating a graph costs more than it saves when the
  // batch is solved once, as every bundle adjustment of the incremental pipeline is)
  const bool graph = b->use_graph && !b->profiling && !b->lookahead && b->d.chol.tmask != nullptr && b->n_solves > 0;
  ++b->n_solves;
  auto graph_of = [&](int g, int si) -> hipGraphExec_t {  // built on first use: one pass, one node per launch, a linear chain
    if (b->pass_graph[g][si]) return b->pass_graph[g][si];
    GraphRecorder rec;
    bool ok = hipGraphCreate(&rec.graph, 0) == hipSuccess;
    if (ok) {
      b->stream = b->streams[g];
      g_recorder = &rec;
      PassShape shg = b->shapes[si];
      if (si == 0) shg.slots = b->group_count[g];
      shg.path_slots = shg.slots;
      enqueue_pass<TYPE>(b, b->dg[g], shg);
      g_recorder = nullptr;
      ok = rec.ok && hipGraphInstantiate(&b->pass_graph[g][si], rec.graph, nullptr, nullptr, 0) == hipSuccess;
    }
    if (rec.graph) (void)hipGraphDestroy(rec.graph);
    if (!ok) { (void)hipGetLastError(); b->pass_graph[g][si] = nullptr; b->use_graph = false; }
    return b->pass_graph[g][si];
  };
  std::vector<char> galive(G, 1);
  std::vector<int> enq(G, 0), shape_used, ladder;
  for (const PassShape& s : b->shapes) ladder.push_back(s.slots);
  struct PassLog { int g, si, slots, cnt; };
  std::vector<PassLog> pass_log;  // PTZ_BA_DEBUG_TIMING: what the host chose for every enqueued pass
  // Watchdog.  The loop below only ever waits on words the DEVICE writes; if a launch was refused, a kernel faulted or the
  // progress word stops moving for any other reason, nothing would ever clear the wait.  So whenever no group has made
  // progress for `watchdog_ms`, every waiting group's stream is asked for its state: an error ends the solve with
  // PTZ_ENODEVICE; an IDLE stream whose passes have all run without the progress word catching up is credited with them
  // (`credit`) and fed further passes -- the pipeline degrades to enqueue-and-wait, results unchanged -- and a group that needs
  // that more often than a solve has passes is given up on.  Never a spin without end, never a re-exec.
  std::vector<int> credit(G, 0), stalls(G, 0);
  double watchdog_ms = 50.0;
  if (const char* e = getenv("PTZ_BA_WATCHDOG_MS")) watchdog_ms = std::max(0.1, atof(e));
  double t_progress = now();
  int watchdog_rc = PTZ_OK;
  int alive = G;
  while (alive > 0) {
    bool progressed = false;
    for (int g = 0; g < G; ++g) {
      if (!galive[g]) continue;
      if (__atomic_load_n(&b->h_ctl[4 * g + 1], __ATOMIC_ACQUIRE)) { galive[g] = 0; --alive; progressed = true; continue; }
      if (enq[g] >= max_it) { galive[g] = 0; --alive; progressed = true; continue; }  // every step the options allow is enqueued (the last pass's k_lm_pre closes the books)
      if (enq[g] - std::max(__atomic_load_n(&b->h_ctl[4 * g], __ATOMIC_ACQUIRE), credit[g]) >= b->ahead) continue;
      const double te0 = now();
      b->stream = b->streams[g];
      // launch shape: the variants of the smallest ladder shape that covers the scenes last reported active (the count only ever
      // decreases, so a stale value is an upper bound); the extent is the ladder shape's for a replayed graph and the count itself
      // for a pass enqueued here (pass_extent)
      const int cnt = __atomic_load_n(&b->h_ctl[4 * g + 2], __ATOMIC_ACQUIRE);
      const bool replay = graph && b->use_graph;
      const PassExtent ext = pass_extent(cnt, b->group_count[g], ladder.data(), b->compaction ? (int)ladder.size() : 1, replay, b->exact_fit);
      const int si = ext.shape;
      PassShape sh = b->shapes[si];
      sh.path_slots = si == 0 ? b->group_count[g] : sh.slots;
      sh.slots = ext.slots;
      sh.compact = ext.compact;
      if (dbg) {
        if (shape_used.size() < b->shapes.size()) shape_used.resize(b->shapes.size(), 0);
        ++shape_used[si];
        pass_log.push_back({g, si, sh.slots, cnt});
      }
      // (one or two rigs: the passes are enqueued as they are -- a pass is ~200 us of device time against ~25 us of host time for its
      //  six launches, and between two REPLAYED graphs the device idles 8.4 us: 5.20 -> 5.09 ms per 25-iteration solve of the C2 rig,
      //  A/B on one box)
      hipGraphExec_t ge = (replay && sh.slots > 2) ? graph_of(g, si) : nullptr;
      if (ge) PTZ_HIP_TRY(hipGraphLaunch(ge, b->streams[g]));
      else { b->stream = b->streams[g]; enqueue_pass<TYPE>(b, b->dg[g], sh); }
      ++enq[g];
      progressed = true;
      t_enq += now() - te0;
    }
    if (progressed) { t_progress = now(); continue; }
    const double ts0 = now();
    __builtin_ia32_pause();
    if (ts0 - t_progress > watchdog_ms) {
      for (int g = 0; g < G && watchdog_rc == PTZ_OK; ++g) {
        if (!galive[g]) continue;
        const hipError_t q = hipStreamQuery(b->streams[g]);
        if (q == hipErrorNotReady) continue;  // still working: a long pass, not a stall
        const hipError_t le = hipGetLastError();
        if (q != hipSuccess || le != hipSuccess) {
          fprintf(stderr, "[ptz_ba] scene group %d: the device reported %s after %d enqueued LM passes; giving up on this solve\n", g,
                  hipGetErrorName(q != hipSuccess ? q : le), enq[g]);
          watchdog_rc = PTZ_ENODEVICE;
          break;
        }
        // idle and healthy: everything enqueued has run.  Retired meanwhile?  Then the next sweep sees it.
        if (__atomic_load_n(&b->h_ctl[4 * g + 1], __ATOMIC_ACQUIRE)) continue;
        if (__atomic_load_n(&b->h_ctl[4 * g], __ATOMIC_ACQUIRE) >= enq[g]) continue;  // the word caught up
        if (++stalls[g] > max_it + 8) {
          fprintf(stderr, "[ptz_ba] scene group %d: no progress reports from the device (%d enqueued passes ran to completion without one); giving up on this solve\n", g, enq[g]);
          watchdog_rc = PTZ_ENODEVICE;
          break;
        }
        credit[g] = enq[g];
      }
      if (watchdog_rc != PTZ_OK) break;
      t_progress = now();
    }
    t_sync += now() - ts0;
  }
  if (watchdog_rc != PTZ_OK) {
    for (int g = 0; g < G; ++g) (void)stream_wait(b->streams[g]);  // nothing of this batch may be in flight when the caller frees it
    (void)hipGetLastError();
    return watchdog_rc;
  }
  if (dbg) for (size_t k = 0; k < shape_used.size(); ++k) fprintf(stderr, "[ptz_ba] launch shape %zu (%d slots%s): %d passes\n", k, b->shapes[k].slots, b->shapes[k].compact ? ", compacted" : "", shape_used[k]);
  if (dbg) for (int g = 0; g < G; ++g) fprintf(stderr, "[ptz_ba] group %d: %d passes enqueued, %d reached by the device when the host stopped\n", g, enq[g], b->h_ctl[4 * g]);
  // join
  for (int g = 1; g < G; ++g) {
    PTZ_HIP_TRY(hipEventRecord(b->join_ev[g], b->streams[g]));
    PTZ_HIP_TRY(hipStreamWaitEvent(s0, b->join_ev[g], 0));
  }
  b->stream = s0;
  PTZ_HIP_TRY(hipEventRecord(b->ev1, s0));
  // the scenes' LM states come back behind the last pass, inside the solve's ONE wait
  void* lm_pin = nullptr;
  if (ptzpool::pinned_acquire(sizeof(LmState) * B, &lm_pin) == hipSuccess) {
    if (hipMemcpyAsync(lm_pin, d.lm, sizeof(LmState) * B, hipMemcpyDeviceToHost, s0) != hipSuccess) { (void)hipGetLastError(); ptzpool::pinned_release(lm_pin); lm_pin = nullptr; }
  }
  else (void)hipGetLastError();
  {
    const hipError_t we = stream_wait(s0);
    b->release_staged();  // (uploads of create / set_state that were left in flight)
    if (we != hipSuccess) { if (lm_pin) ptzpool::pinned_release(lm_pin); PTZ_HIP_TRY(we); }
  }
  {
    const hipError_t le = hipGetLastError();  // a kernel launch that was refused (resources, arguments) must not pass for a solve
    if (le != hipSuccess) { if (lm_pin) ptzpool::pinned_release(lm_pin); PTZ_HIP_TRY(le); }
  }
  float ms = 0;
  (void)hipEventElapsedTime(&ms, b->ev0, b->ev1);
  b->last_ms = ms;
  b->prof_collect();
  if (dbg) fprintf(stderr, "[ptz_ba] groups %d: total %.2f ms, enqueue %.2f ms, sync-wait %.2f ms, device %.2f ms\n", G, now() - t_start, t_enq, t_sync, ms);
  {
    std::vector<LmState> h(B);
    if (lm_pin) { memcpy(h.data(), lm_pin, sizeof(LmState) * B); ptzpool::pinned_release(lm_pin); }
    else PTZ_HIP_TRY(copy_on(b->stream, h.data(), d.lm, sizeof(LmState) * B, hipMemcpyDeviceToHost));
    int timeouts = 0;
    for (int i = 0; i < B; ++i) timeouts += h[i].chain_timeouts;
    if (dbg && !pass_log.empty()) {
      // Launch extents against the scenes that were really active: pass p of a group works on the scenes that took more than p
      // LM steps.  Per ladder shape: slots launched, live scenes, empty slots (slots without a live scene), summed over its passes.
      // PTZ_BA_DEBUG_TIMING=2 lists every pass: group, pass, shape, slots, the host's (stale) count, live scenes.
      const bool each = atoi(getenv("PTZ_BA_DEBUG_TIMING")) >= 2;
      std::vector<int> pass_of(G, 0);
      std::vector<long long> slots_sum(b->shapes.size(), 0), live_sum(b->shapes.size(), 0), stale_sum(b->shapes.size(), 0);
      for (const PassLog& pl : pass_log) {
        const int p = pass_of[pl.g]++;
        int live = 0;
        for (int i = b->group_first[pl.g]; i < b->group_first[pl.g] + b->group_count[pl.g]; ++i) live += h[i].num_lm_steps > p;
        slots_sum[pl.si] += pl.slots; live_sum[pl.si] += live; stale_sum[pl.si] += pl.cnt;
        if (each) fprintf(stderr, "[ptz_ba] pass g%d p%d: shape %d, %d slots, host count %d, live %d\n", pl.g, p, pl.si, pl.slots, pl.cnt, live);
      }
      for (size_t k = 0; k < b->shapes.size(); ++k)
        if (slots_sum[k]) fprintf(stderr, "[ptz_ba] launch shape %zu: slots x passes %lld, host count x passes %lld, live scenes x passes %lld, empty slots x passes %lld\n",
                                  k, slots_sum[k], stale_sum[k], live_sum[k], slots_sum[k] - live_sum[k]);
    }
    if (timeouts) {  // never a silently different trajectory: a hand-over that did not arrive is a device problem, not a rejected step
      fprintf(stderr, "[ptz_ba] %d linear solve(s) of this batch lost a tile hand-over of the one-launch factorisation (bounded wait ran out); "
                      "the solve is reported as failed\n", timeouts);
      return PTZ_ENODEVICE;
    }
    for (int i = 0; out && i < B; ++i) {
      ptz_lm_summary& s = out[i];
      s.termination_type = h[i].termination;
      s.num_iterations = h[i].n_summaries - 1;
      s.num_lm_steps = h[i].num_lm_steps;
      s.num_successful_steps = h[i].num_successful;
      s.num_unsuccessful_steps = h[i].num_unsuccessful;
      s.num_residuals = 2 * b->scenes[i].n_obs + 2 * b->scenes[i].n_o3;
      s.num_linear_solves = h[i].num_linear_solves;
      s.num_jacobian_evals = h[i].num_jac_evals;
      s.initial_cost = h[i].initial_cost;
      s.final_cost = h[i].final_cost;
      s.final_radius = h[i].radius;
      s.final_gradient_max_norm = h[i].grad_max;
    }
  }
  return PTZ_OK;
}

}  // namespace

namespace ptz {
// defined here (needs ptz_ba_batch) but uses the kernels of ptz_chol.hip through chol_factor_solve pieces
// (its left-looking loop stands a second time, without the profiling brackets, in ptz_debug_chol_solve, ptz_chol.hip, where the
// kernel tests reach it: a change to either loop belongs in both)
void chol_factor_solve_profiled(const CholBatch& cb, double* x, hipStream_t stream, void* prof, bool fused, int path_count)
{
  // One-step look-ahead: after the triangular solve of block column k, the small update of block column k+1 stays on
  // the main stream, so the (latency-bound) diagonal factorisation and triangular solve of step k+1 start at once,
  // while the bulk of the trailing update (tile columns >= k+2) runs on the auxiliary stream.
  ptz_ba_batch* b = (ptz_ba_batch*)prof;
  const int nt = cb.np / CHOL_NB;
  hipStream_t aux = b->aux_stream(stream);
  const bool la = aux != nullptr && nt >= 3;
  hipEvent_t evT = nullptr, evR = nullptr;
  if (la) b->lookahead_events(stream, &evT, &evR);
  bool rest_pending = false;
  if (fused) {  // a few scenes: the whole factorisation in one launch (chol_chain_kernel), or one launch per step of the schedule (chol_col_step_kernel)
    // (the path is that of the ladder shape, `path_count` systems, whatever the launch's own extent cb.count)
    if (cb.L && cb.Linv && cb.chain_ctl && chol_chain_fits(path_count, cb.np)) {
      b->prof_begin(P_CHOL_SYRK);
      chol_chain_launch(cb, stream);
      b->prof_end();
    }
    else {
      b->prof_begin(P_CHOL_PANEL);
      chol_diag_launch(cb, -1, stream);
      b->prof_end();
      for (int st = 0; st + 1 < chol_step_count(cb); ++st) {
        b->prof_begin(P_CHOL_SYRK);
        chol_col_step_launch(cb, st, stream);
        b->prof_end();
      }
    }
    b->prof_begin(P_CHOL_BACK);
    chol_backsolve_launch(cb, x, stream);
    b->prof_end();
    return;
  }
  if (b->left_looking) {
    for (int k = 0; k < nt; ++k) {
      if (k > 0) {
        b->prof_begin(P_CHOL_SYRK);
        chol_update_col_launch(cb, k, stream, /*fuse_diag=*/true);  // also factors the diagonal tile of column k
        b->prof_end();
      }
      b->prof_begin(P_CHOL_PANEL);
      chol_panel_launch(cb, k, stream, /*diag_done=*/k > 0);
      b->prof_end();
    }
    b->prof_begin(P_CHOL_BACK);
    chol_tile_inverse_launch(cb, stream);
    chol_backsolve_launch(cb, x, stream);
    b->prof_end();
    return;
  }
  for (int k = 0; k < nt; ++k) {
    const int m = nt - k - 1;
    b->prof_begin(P_CHOL_PANEL);
    chol_panel_launch(cb, k, stream, /*diag_done=*/k > 0);  // the trailing update of step k - 1 factored this diagonal tile
    b->prof_end();
    if (m <= 0) continue;
    if (!la) {
      b->prof_begin(P_CHOL_SYRK);
      chol_syrk_launch(cb, k, stream, 0, /*fuse_diag=*/true);
      b->prof_end();
      continue;
    }
    (void)hipEventRecord(evT, stream);              // panel k (L_ik tiles) is final
    (void)hipStreamWaitEvent(aux, evT, 0);
    if (rest_pending) (void)hipStreamWaitEvent(stream, evR, 0);  // column k+1 was last touched by rest(k-1)
    b->prof_begin(P_CHOL_SYRK);
    chol_syrk_launch(cb, k, stream, 1, /*fuse_diag=*/true);
    b->prof_end();
    if (m >= 2) {
      hipStream_t keep = b->stream;
      b->stream = aux;
      b->prof_begin(P_CHOL_SYRK);
      chol_syrk_launch(cb, k, aux, 2);
      b->prof_end();
      b->stream = keep;
      (void)hipEventRecord(evR, aux);
      rest_pending = true;
    }
  }
  if (la && rest_pending) (void)hipStreamWaitEvent(stream, evR, 0);
  b->prof_begin(P_CHOL_BACK);
  chol_tile_inverse_launch(cb, stream);
  chol_backsolve_launch(cb, x, stream);
  b->prof_end();
}
}  // namespace ptz

// One rig's tracks, resident in HBM (ptz_rig_create), and the bounds a view of it is sized by.
struct ptz_rig {
  int device = 0, n_img = 0, n_track = 0;
  int64_t n_view = 0;
  const int* d_trk_ptr = nullptr;
  const int* d_trk_img = nullptr;
  const float2* d_trk_uv = nullptr;
  int64_t ent_bound = 0;           // camera-pair entries of the whole rig: sum over the tracks of L (L - 1) / 2
  int max_track_len = 0;           // views of the rig's longest track: bounds the length field of a view batch's sort key (ptz_ba_batch_create_views)
  std::vector<int> img_obs, img_ent;  // per image: its views, and its entries as the HIGHER camera of a pair
  std::vector<void*> allocs;
};

// ---- covariance (ptz_ba_cov.hip): what that file is given of a batch ------------------------------------------------------------
// the scenes' real extents (a view batch finds them on the device) and the half of the double-buffered state that is current
namespace ptz {
namespace {
__global__ void k_ba_cov_pack(Dev d, int initial_state, BaCovScene* out)
{
  const int sc = blockIdx.x * blockDim.x + threadIdx.x;
  if (sc >= d.n_scene) return;
  const SceneDev s = d.scene[sc];
  BaCovScene o;
  o.n_cam = s.n_cam; o.n_ray = s.n_ray; o.n_obs = s.n_obs; o.n_pair = s.n_pair;
  o.cam_off = s.cam_off; o.ray_off = s.ray_off; o.obs_off = s.obs_off; o.pair_off = s.pair_off;
  o.idx = s.idx; o.cur = initial_state ? 0 : d.lm[sc].cur;
  o.o3_off = s.o3_off; o.n_o3 = s.n_o3;
  out[sc] = o;
}
}  // namespace
}  // namespace ptz

// =============================================================================================================
// C-ABI
// =============================================================================================================
extern "C" {

void ptz_lm_options_default(ptz_lm_options* o)
{
  memset(o, 0, sizeof(*o));
  o->max_num_iterations = 200;
  o->device_id = 0;
  o->max_num_consecutive_invalid_steps = 5;
  o->jacobi_scaling = 1;
  o->initial_trust_region_radius = 1e4;
  o->max_trust_region_radius = 1e16;
  o->min_trust_region_radius = 1e-32;
  o->min_relative_decrease = 1e-3;
  o->min_lm_diagonal = 1e-6;
  o->max_lm_diagonal = 1e32;
  o->function_tolerance = 1e-6;
  o->gradient_tolerance = 1e-10;
  o->parameter_tolerance = 1e-8;
}

const char* ptz_version(void) { return "ptz-calib_amd 0.1 (gfx950)"; }

int32_t ptz_device_count(void)
{
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int32_t ptz_ba_plan_tile_order(int32_t nt, int32_t first_dense, const uint8_t* mask, int32_t* perm, int32_t* lanes,
                               int32_t* sched, int32_t* n_steps)
{
  if (nt <= 0 || !mask || !perm || !lanes) return PTZ_EINVAL;
  int la = 0, lb = 0;
  const bool planned = plan_dissection(nt, first_dense, mask, perm, &la, &lb);
  if (!planned) { for (int t = 0; t < nt; ++t) perm[t] = t; la = lb = 0; }
  lanes[0] = la; lanes[1] = lb;
  if (sched && n_steps) {  // the function batches run: permuted mask, fill, levels
    std::vector<unsigned char> m((size_t)nt * nt, 0);
    n_steps[0] = fill_and_schedule(nt, mask, planned ? perm : nullptr, m.data(), sched);
  }
  return planned ? 1 : 0;
}

int32_t ptz_ba_cam_block_dim(int32_t factor_type)
{
  if (factor_type == PTZ_BA_PTZRay) return 4;
  if (factor_type == PTZ_BA_PTZRayDist) return 5;
  if (factor_type == PTZ_BA_PTZRayFxfyDist) return 6;
  if (factor_type == PTZ_BA_PTZRayDistDisp) return 8;  // [f, k1, r1, r2, r3, d0, d1, d2]
  return PTZ_EUNSUPPORTED;
}

int32_t ptz_ba_batch_cam_block_dim(const ptz_ba_batch* b) { return b ? b->nc : PTZ_EINVAL; }

void ptz_ba_batch_destroy(ptz_ba_batch* b)
{
#ifdef PTZ_CHOL_TIMELINE
  if (b && b->d.chol.np > 0) chol_chain_timeline_print(b->d.chol.np / 64);
#endif
  if (!b) return;
  DeviceGuard guard(b->device);
  // nothing of this batch may still be running when its memory is handed to the next one
  for (auto st : b->streams) (void)stream_wait(st);
  for (auto st : b->aux) (void)stream_wait(st);
  if (b->io) (void)stream_wait(b->io);
  b->release_staged();
  const int dv = b->device;
  for (void* p : b->allocs) ptzpool::dev_release(dv, p);
  for (auto e : b->ev_pool) ptzpool::event_release(dv, true, e);
  if (b->h_ctl) ptzpool::pinned_release(b->h_ctl);
  for (auto& v : b->pass_graph) for (auto ge : v) if (ge) (void)hipGraphExecDestroy(ge);
  ptzpool::event_release(dv, true, b->ev0);
  ptzpool::event_release(dv, true, b->ev1);
  if (b->create_ev) ptzpool::event_release(dv, false, b->create_ev);
  for (auto st : b->streams) ptzpool::stream_release(dv, st);
  for (auto st : b->aux) ptzpool::stream_release(dv, st);
  ptzpool::stream_release(dv, b->io);
  for (auto e : b->la_ev) ptzpool::event_release(dv, false, e);
  for (auto e : b->fork_ev) ptzpool::event_release(dv, false, e);
  for (auto e : b->join_ev) ptzpool::event_release(dv, false, e);
  delete b;
}

namespace {
// Camera-pair entry lists of one scene (the off-diagonal blocks of the reduced system): for every ray, every (a, b) with
// cam(a) > cam(b); a is stored as its position in cam(a)'s observation list (the LDS slot of T_a in k_schur).  Independent of
// every other scene apart from the base offset of its observations, so batches build these lists on several host threads.
struct PairBuild {
  std::vector<int> pci, pcj, pptr, pbrow;  // pptr: scene-local entry offsets (n_pair + 1); pbrow: first W row of camera cj
  std::vector<unsigned> ent;        // copied into the batch-wide array (in parallel, per wave) and released
  std::vector<uint2> runs;          // k_schur's runs: {first entry (scene-local here), pair among the camera's | entries << 16}
  std::vector<int> prun;            // first run of every pair (scene-local), n_pair + 1
  int64_t n_ent = 0;
  int n_pair = 0, max_cam_obs = 0, max_cam_ent = 0, max_cam_pair = 0, max_cam_run = 0, err = PTZ_OK;
};

// Where a scene's observation-side arrays go in the batch-wide host arrays (all offsets are prefix sums of the scene sizes,
// known before any scene is built, so the worker threads write them in place).
struct ObsDest {
  float2* uv; int* cam; int* ray; int* camobs; int* camray; float2* camuv;  // + obs_off
  int* rayptr; double* w;                                      // + ray_off (+ scene index for the pointer array)
  int* camptr; int* campair; int* camrun;                      // + cam_off + scene index
  int* wpos;                                                   // + obs_off
};  // (member order = the order of the initialiser in build_scene_wave)

// The batch-wide host arrays of the observation side and where every scene's part of them begins
struct HostObs {
  std::vector<size_t> obs_base, ray_base, cam_base;  // [n + 1]
  RawVec<float2> uv, camuv;
  RawVec<int> cam, ray, camobs, camray, wpos;
  std::vector<int> rayptr, camptr, campair, camrun;
  std::vector<double> w;
  void set_bases(int n, const ptz_ba_problem* p)
  {
    obs_base.assign(n + 1, 0); ray_base.assign(n + 1, 0); cam_base.assign(n + 1, 0);
    for (int i = 0; i < n; ++i) { obs_base[i + 1] = obs_base[i] + (size_t)p[i].n_obs; ray_base[i + 1] = ray_base[i] + p[i].n_ray; cam_base[i + 1] = cam_base[i] + p[i].n_cam; }
  }
  void resize_all(int n)  // (uninitialised where RawVec: every element is written by the builder threads)
  {
    const size_t to = obs_base[n], tr = ray_base[n], tc = cam_base[n];
    uv.resize(to); camuv.resize(to); cam.resize(to); ray.resize(to); camobs.resize(to); camray.resize(to); wpos.resize(to);
    rayptr.resize(tr + n); w.resize(tr); camptr.resize(tc + n); campair.resize(tc + n); camrun.resize(tc + n);
  }
};

// Scratch vectors of build_pairs, handed from call to call (a batch builds its scenes on short-lived worker threads, several
// batches at a time in the lock-step PTZ-IBA): a vector that keeps its capacity costs no allocation and, above all, no page
// faults -- fresh memory was a third of the structure stage's time.
struct BuildScratch {
  std::vector<int> len, first, start, cnt_ray, cnt_cam, fill, pos, pair_cnt, pair_fill, cam_first, cam_ent;
  std::vector<char> asc;
};
struct ScratchPool {
  std::mutex mu;
  std::vector<BuildScratch*> free_list;
  BuildScratch* get()
  {
    {
      std::lock_guard<std::mutex> lk(mu);
      if (!free_list.empty()) { BuildScratch* s = free_list.back(); free_list.pop_back(); return s; }
    }
    return new BuildScratch();
  }
  void put(BuildScratch* s)
  {
    std::lock_guard<std::mutex> lk(mu);
    if (free_list.size() < 32) { free_list.push_back(s); return; }
    delete s;
  }
};
inline ScratchPool* scratch_pool()
{
  static ScratchPool* p = new ScratchPool();  // never destroyed: worker threads may outlive static destructors
  return p;
}
struct ScratchLease {
  BuildScratch* s;
  ScratchLease() : s(scratch_pool()->get()) {}
  ~ScratchLease() { scratch_pool()->put(s); }
};

void build_pairs(const ptz_ba_problem& p_in, int obase, int ray_off, const ObsDest& od, PairBuild& out, int* ray_perm, int max_runs,
                 bool pairs_on_device = false)
{
  // Internal ray order: by track length, longest first, then by the track's first camera (stable).  The ray-centric kernels give one lane to a ray and walk its
  // observations; with the caller's order a wave of 64 rays waits for its longest track (4 .. 19 observations on a C2 rig, the
  // mean over waves of the longest is 14.5 against a mean length of 7.5), sorted it does not (1.01 x the mean).  Observations
  // keep their order inside a track; ray_perm[j] = the caller's index of internal ray j.
  ScratchLease lease;
  BuildScratch& sc = *lease.s;
  ptz_ba_problem p = p_in;
  std::vector<int>& cnt_ray = sc.cnt_ray;
  std::vector<int>& cnt_cam = sc.cnt_cam;
  cnt_ray.assign(p.n_ray + 1, 0);
  cnt_cam.assign(p.n_cam + 1, 0);
  {
    std::vector<int>&len = sc.len, &first = sc.first, &start = sc.start;
    len.assign(p.n_ray, 0);
    first.assign(p.n_ray + 1, 0);
    for (int64_t a = 0; a < p.n_obs; ++a) ++len[p_in.obs_ray[a]];
    int max_len = 0;
    for (int j = 0; j < p.n_ray; ++j) {
      if (len[j] == 0) { out.err = PTZ_EINVAL; return; }  // every ray has >= 1 observation
      first[j + 1] = first[j] + len[j];
      max_len = std::max(max_len, len[j]);
    }
    // counting sort by (length descending, first camera of the track ascending), stable: rays of one wave then also look at
    // the same few cameras at the same time, and their reads of the camera table in LDS are broadcasts instead of bank conflicts
    // (coarser spatial keys in front of the length -- 2 to 16 sectors of the camera range -- were measured: no further gain)
    const size_t nkey = (size_t)(max_len + 1) * (size_t)std::max(p.n_cam, 1);
    auto key = [&](int j) {
      const int c = p_in.obs_cam[first[j]];
      return (size_t)(max_len - len[j]) * (size_t)p.n_cam + (size_t)(c >= 0 && c < p.n_cam ? c : 0);
    };
    start.assign(nkey + 2, 0);
    for (int j = 0; j < p.n_ray; ++j) ++start[key(j) + 1];
    for (size_t l = 0; l <= nkey; ++l) start[l + 1] += start[l];
    for (int j = 0; j < p.n_ray; ++j) ray_perm[start[key(j)]++] = j;
    // the observations in the internal order go straight into the batch-wide arrays (no copy of the problem in between)
    int at = 0;
    for (int jn = 0; jn < p.n_ray; ++jn) {
      const int jo = ray_perm[jn];
      od.w[jn] = p_in.ray_weight[jo];
      cnt_ray[jn] = at;
      for (int a = first[jo]; a < first[jo + 1]; ++a, ++at) {
        const int c = p_in.obs_cam[a];
        od.uv[at] = make_float2(p_in.obs_uv[2 * a], p_in.obs_uv[2 * a + 1]);
        od.cam[at] = c;
        od.ray[at] = jn;
        ++cnt_cam[c + 1];
      }
    }
    cnt_ray[p.n_ray] = at;
    p.obs_uv = reinterpret_cast<const float*>(od.uv); p.obs_cam = od.cam; p.obs_ray = od.ray; p.ray_weight = od.w;
  }
  for (int j = 0; j <= p.n_ray; ++j) od.rayptr[j] = obase + cnt_ray[j];
  for (int c = 0; c < p.n_cam; ++c) cnt_cam[c + 1] += cnt_cam[c];
  std::vector<int>& pos = sc.pos;
  pos.resize(p.n_obs);
  {  // camera-major observation lists; pos[a] = rank of observation a in its camera's list (camera-major order = ascending a)
    std::vector<int>& fill = sc.fill;
    fill.assign(cnt_cam.begin(), cnt_cam.end() - 1);
    for (int64_t a = 0; a < p.n_obs; ++a) {
      const int c = p.obs_cam[a];
      const int slot = fill[c]++;
      pos[a] = slot - cnt_cam[c];
      od.camobs[slot] = obase + (int)a;
      od.camray[slot] = ray_off + p.obs_ray[a];
      od.camuv[slot] = od.uv[a];
      od.wpos[a] = obase + slot;
    }
    for (int c = 0; c < p.n_cam; ++c) out.max_cam_obs = std::max(out.max_cam_obs, fill[c] - cnt_cam[c]);
    for (int c = 0; c <= p.n_cam; ++c) od.camptr[c] = obase + cnt_cam[c];
  }
  if (pairs_on_device) {
    // pairs, entries and runs are made by k_pairs from the arrays above (ptz_ba_batch_create): only the entry count is needed here
    int64_t ne = 0;
    for (int j = 0; j < p.n_ray; ++j) { const int64_t L = cnt_ray[j + 1] - cnt_ray[j]; ne += L * (L - 1) / 2; }
    if (ne > 0x7fffffff) { out.err = PTZ_EINVAL; return; }
    out.n_ent = ne;
    out.n_pair = 0;
    return;
  }
  // counting sort by (ci, cj): pairs ascending in ci * n_cam + cj, the entries of a pair in ray order (stable).
  // The (a, b) pairs with cam(a) > cam(b) of every ray are walked twice in ray order -- once to count them per camera pair,
  // once to drop them into their slots -- rather than kept as a list (round 2 kept two 4-byte indices per entry, 3 MB per C2
  // scene written and re-read: 6.4 -> 4.0 ms per scene on one host thread).  Observations of a track come camera-ascending
  // from the packing (track asc, image asc: ptzray_optimizer.cc:801-850), in which case the pairs are simply (a, b < a); any
  // other order takes the general double loop.  (Walking camera by camera instead, with n_cam counters that stay in L1, was
  // measured: slower, the walk then chases observation -> track -> cameras in random order.)
  const size_t ncc = (size_t)p.n_cam * p.n_cam;
  std::vector<int>& pair_cnt = sc.pair_cnt;
  pair_cnt.assign(ncc, 0);
  std::vector<char>& asc = sc.asc;
  asc.resize(p.n_ray);
  int64_t n_ent = 0;
  auto for_each_entry = [&](auto&& fn) -> bool {  // fn(a, bb, slot of (cam(a), cam(bb)) in the n_cam x n_cam table)
    for (int j = 0; j < p.n_ray; ++j) {
      const int r0 = cnt_ray[j], r1 = cnt_ray[j + 1];
      if (asc[j]) {
        for (int a = r0 + 1; a < r1; ++a) {
          const size_t row = (size_t)p.obs_cam[a] * p.n_cam;
          for (int bb = r0; bb < a; ++bb) fn(a, bb, row + p.obs_cam[bb]);
        }
      }
      else {
        for (int a = r0; a < r1; ++a)
          for (int bb = r0; bb < r1; ++bb) {
            const int ci = p.obs_cam[a], cj = p.obs_cam[bb];
            if (ci == cj && a != bb) return false;  // an image appears once per track (tracks.cc:77)
            if (ci > cj) fn(a, bb, (size_t)ci * p.n_cam + cj);
          }
      }
    }
    return true;
  };
  for (int j = 0; j < p.n_ray; ++j) {
    bool ascending = true;
    for (int a = cnt_ray[j] + 1; a < cnt_ray[j + 1]; ++a) ascending &= p.obs_cam[a] > p.obs_cam[a - 1];
    asc[j] = ascending ? 1 : 0;
  }
  if (!for_each_entry([&](int, int, size_t cell) { ++pair_cnt[cell]; ++n_ent; })) { out.err = PTZ_EINVAL; return; }
  if (n_ent > 0x7fffffff) { out.err = PTZ_EINVAL; return; }
  int npair = 0;
  std::vector<int>&cam_first = sc.cam_first, &cam_ent = sc.cam_ent, &pair_fill = sc.pair_fill;
  cam_first.assign(p.n_cam + 1, -1);
  cam_ent.assign(p.n_cam, 0);
  pair_fill.resize(ncc);  // next free entry slot of a pair (scene-local); only the cells of existing pairs are read
  {
    int run = 0;
    for (int ci = 0; ci < p.n_cam; ++ci)
      for (int cj = 0; cj < ci; ++cj) {
        const int c = pair_cnt[(size_t)ci * p.n_cam + cj];
        if (c == 0) continue;
        out.pci.push_back(ci);
        out.pcj.push_back(cj);
        out.pbrow.push_back(obase + cnt_cam[cj]);
        out.pptr.push_back(run);
        if (cam_first[ci] < 0) cam_first[ci] = npair;
        pair_fill[(size_t)ci * p.n_cam + cj] = run;
        cam_ent[ci] += c;
        run += c;
        ++npair;
      }
    out.pptr.push_back(run);
  }
  out.ent.resize((size_t)n_ent);
  for_each_entry([&](int a, int bb, size_t cell) {
    out.ent[pair_fill[cell]++] = (unsigned)pos[a] | ((unsigned)pos[bb] << 16);  // (LDS slot of T_a, W row of b relative to camera cj's first row)
  });
  // per-camera pair ranges (pairs are sorted by ci): cameras without pairs get an empty range
  cam_first[p.n_cam] = npair;
  for (int c = 0; c < p.n_cam; ++c) out.max_cam_ent = std::max(out.max_cam_ent, cam_ent[c]);
  for (int c = p.n_cam - 1; c >= 0; --c) if (cam_first[c] < 0) cam_first[c] = cam_first[c + 1];
  for (int c = 0; c <= p.n_cam; ++c) od.campair[c] = cam_first[c];
  for (int c = 0; c < p.n_cam; ++c) out.max_cam_pair = std::max(out.max_cam_pair, cam_first[c + 1] - cam_first[c]);
  // Runs of k_schur's second phase.  A camera's entries (its pairs one after the other) are cut into pieces of one length L
  // that never straddle two pairs, L the smallest for which the camera has at most max_runs (= threads) pieces: a thread of the
  // camera's workgroup then sums exactly one piece, and all threads have the same amount of work whatever the lengths of the
  // pairs.  (A view with more pairs than threads gets one run per pair and several rounds; k_schur then keeps its table in
  // global memory, see schur_tg.)
  out.prun.assign(npair + 1, 0);
  for (int c = 0; c < p.n_cam; ++c) {
    od.camrun[c] = (int)out.runs.size();
    const int p0 = cam_first[c], p1 = cam_first[c + 1];
    if (p1 == p0) continue;
    int max_len = 0;
    for (int pi = p0; pi < p1; ++pi) max_len = std::max(max_len, out.pptr[pi + 1] - out.pptr[pi]);
    auto pieces = [&](int L) { int64_t n = 0; for (int pi = p0; pi < p1; ++pi) n += (out.pptr[pi + 1] - out.pptr[pi] + L - 1) / L; return n; };
    // smallest L in [1, max_len] with pieces(L) <= max_runs (max_len if there is none).  pieces() is non-increasing in L and
    // pieces(L) >= entries / L, so the search starts at ceil(entries / max_runs) -- usually the answer or one below it -- and
    // walks up (a bisection over [1, max_len] cost nine rounds of integer divisions per camera, 0.3 ms per 170-view scene)
    const int total = out.pptr[p1] - out.pptr[p0];
    int lo = std::max(1, std::min(max_len, (total + max_runs - 1) / max_runs));
    while (lo < max_len && pieces(lo) > max_runs) ++lo;
    const int L = std::min(lo, 65535);
    for (int pi = p0; pi < p1; ++pi) {
      out.prun[pi] = (int)out.runs.size();
      for (int e = out.pptr[pi]; e < out.pptr[pi + 1]; e += L)
        out.runs.push_back(make_uint2((unsigned)e, (unsigned)(pi - p0) | ((unsigned)std::min(L, out.pptr[pi + 1] - e) << 16)));
    }
    out.max_cam_run = std::max(out.max_cam_run, (int)out.runs.size() - od.camrun[c]);
  }
  od.camrun[p.n_cam] = (int)out.runs.size();
  out.prun[npair] = (int)out.runs.size();
  out.n_pair = npair;
  out.n_ent = n_ent;
}

// Scenes [first, first + count) on up to n_threads host threads: the observation-side arrays and the ray order are written in
// place, the pair lists of scene first + k go to wave[k]
void build_scene_wave(const ptz_ba_problem* problems, int first, int count, int n_threads, HostObs& h, int* ray_perm, std::vector<PairBuild>& wave,
                      bool pairs_on_device)
{
  wave.assign(count, PairBuild());
  run_strided(std::min(n_threads, count), [&](int t0, int step) {
    for (int k = t0; k < count; k += step) {
      const int s = first + k;
      const size_t ob = h.obs_base[s], rb = h.ray_base[s], cb = h.cam_base[s];
      const ObsDest od = {h.uv.data() + ob, h.cam.data() + ob, h.ray.data() + ob, h.camobs.data() + ob, h.camray.data() + ob, h.camuv.data() + ob,
                          h.rayptr.data() + rb + s, h.w.data() + rb, h.camptr.data() + cb + s, h.campair.data() + cb + s,
                          h.camrun.data() + cb + s, h.wpos.data() + ob};
      build_pairs(problems[s], (int)ob, (int)rb, od, wave[k], ray_perm + rb, schur_threads_of(problems[s].factor_type), pairs_on_device);
    }
  });
}
}  // namespace

static int32_t create_impl(int32_t n, const ptz_ba_problem* problems, const ptz_rig_view* views, int32_t view_type, const ptz_lm_options* opt,
                           ptz_ba_batch** out);
int32_t ptz_ba_batch_create(int32_t n, const ptz_ba_problem* problems, const ptz_lm_options* opt, ptz_ba_batch** out)
{
  if (n <= 0 || !problems || !out) return PTZ_EINVAL;
  return create_impl(n, problems, nullptr, 0, opt, out);
}
int32_t ptz_ba_batch_create_views(int32_t n, const ptz_rig_view* views, int32_t factor_type, const ptz_lm_options* opt, ptz_ba_batch** out)
{
  if (n <= 0 || !views || !out) return PTZ_EINVAL;
  if (factor_type != PTZ_BA_PTZRay && factor_type != PTZ_BA_PTZRayDist && factor_type != PTZ_BA_PTZRayFxfyDist) return PTZ_EUNSUPPORTED;
  for (int i = 0; i < n; ++i) {
    const ptz_rig_view& v = views[i];
    if (!v.rig || v.n_cam <= 0 || !v.cam_image || v.rig->n_track <= 0) return PTZ_EINVAL;
    for (int c = 0; c < v.n_cam; ++c)
      if (v.cam_image[c] < 0 || v.cam_image[c] >= v.rig->n_img || (c > 0 && v.cam_image[c] <= v.cam_image[c - 1])) return PTZ_EINVAL;
  }
  return create_impl(n, nullptr, views, factor_type, opt, out);
}

// ---- the stages of create_impl, in the order it runs them --------------------------------------------------------------------
namespace {
// What the stages hand to one another; lives as long as create_impl runs
struct CreateCtx {
  int n = 0;
  const ptz_ba_problem* problems = nullptr;  // the packed problems, or the stand-ins of the views (vprob)
  const ptz_rig_view* views = nullptr;       // nullptr: packed problems
  std::vector<ptz_ba_problem> vprob;
  ptz_lm_options o;
  // sizes decided up front
  int type = 0, NC = 0, CBS = 0, CDS = 0, has3d = 0, pre_max_cam = 0, pre_max_cam_obs = 0, n_threads = 1;  // n_threads: of the scene waves
  size_t pairs_lds = 0;
  bool disp = false, gpu_pairs = false, pairs_check = false;  // pair lists by k_pairs; and by the host as well, compared word for word
  // the host structure
  HostObs h;
  std::vector<int> h_pci, h_pcj, h_pptr, h_pbrow, h_prun, h_o3cam, h_grpptr, h_grpmem;
  RawVec<unsigned> h_ent;
  std::vector<uint2> h_runs; std::vector<double> h_o3xyz; std::vector<float2> h_o3uv;
  std::vector<unsigned char> h_grpcls, h_camflag, h_adj;  // h_adj, views: tile adjacency of every scene's reduced system, marked on the device
  bool any_shared = false, dbg_t = false;
  double ts_ent = 0;
};

// validate + sizes (host only; no device touched before this passes)
int32_t create_validate(int32_t n, const ptz_ba_problem* problems, const ptz_rig_view* views, int32_t view_type, const ptz_lm_options* opt, CreateCtx& c)
{
  c.n = n; c.views = views;
  if (views) {  // stand-ins that carry the sizes the layout is made for
    c.vprob.resize(n);
    for (int i = 0; i < n; ++i) {
      memset(&c.vprob[i], 0, sizeof(ptz_ba_problem));
      c.vprob[i].n_cam = views[i].n_cam; c.vprob[i].n_ray = views[i].rig->n_track; c.vprob[i].n_obs = views[i].rig->n_view;
      c.vprob[i].factor_type = view_type;
    }
    problems = c.vprob.data();
  }
  c.problems = problems;
  c.dbg_t = getenv("PTZ_BA_DEBUG_TIMING") != nullptr;
  if (opt) c.o = *opt; else ptz_lm_options_default(&c.o);
  if (c.o.max_num_iterations <= 0) return PTZ_EINVAL;  // CheckValid, ptzray_optimizer.cc:521
  const int type = c.type = problems[0].factor_type;
  if (type != PTZ_BA_PTZRay && type != PTZ_BA_PTZRayDist && type != PTZ_BA_PTZRayFxfyDist && type != PTZ_BA_PTZRayDistDisp) return PTZ_EUNSUPPORTED;
  c.disp = type == PTZ_BA_PTZRayDistDisp;
  std::vector<int> cam_hist;
  // (pre_max_cam, pre_max_cam_obs decide whether the pair lists are built on the device, before anything is built)
  for (int i = 0; views && i < n; ++i) {
    for (int k = 0; k < views[i].n_cam; ++k) c.pre_max_cam_obs = std::max(c.pre_max_cam_obs, views[i].rig->img_obs[views[i].cam_image[k]]);
    c.pre_max_cam = std::max(c.pre_max_cam, views[i].n_cam);
  }
  for (int i = 0; !views && i < n; ++i) {
    const ptz_ba_problem& p = problems[i];
    if (p.factor_type != type) return PTZ_EINVAL;
    if (p.n_cam <= 0 || p.n_ray <= 0 || p.n_obs <= 0) return PTZ_EINVAL;  // num_cams_ == 0 -> false (:517)
    if (!p.obs_uv || !p.obs_cam || !p.obs_ray || !p.ray_weight) return PTZ_EINVAL;
    if (p.n_obs3d < 0 || (p.n_obs3d > 0 && (!p.obs3d_uv || !p.obs3d_xyz || !p.obs3d_cam))) return PTZ_EINVAL;
    for (int a = 0; a < p.n_obs3d; ++a)
      if (p.obs3d_cam[a] < 0 || p.obs3d_cam[a] >= p.n_cam) return PTZ_EINVAL;
    if (p.n_obs3d > 0) c.has3d = 1;
    cam_hist.assign(p.n_cam, 0);
    for (int64_t a = 0; a < p.n_obs; ++a) {
      if (p.obs_cam[a] < 0 || p.obs_cam[a] >= p.n_cam || p.obs_ray[a] < 0 || p.obs_ray[a] >= p.n_ray) return PTZ_EINVAL;
      if (a > 0 && p.obs_ray[a] < p.obs_ray[a - 1]) return PTZ_EINVAL;
      ++cam_hist[p.obs_cam[a]];
    }
    for (int k = 0; k < p.n_cam; ++k) c.pre_max_cam_obs = std::max(c.pre_max_cam_obs, cam_hist[k]);
    c.pre_max_cam = std::max(c.pre_max_cam, p.n_cam);
  }
  // fy becomes a live column with annotation residuals; PTZRayFxfyDist has it anyway
  c.NC = type == PTZ_BA_PTZRayFxfyDist ? 6 : ((type == PTZ_BA_PTZRay) ? 4 : (c.disp ? 8 : 5)) + c.has3d;
  c.CBS = c.disp ? CAMBLK_DISP + 1 : CAMBLK + 1; c.CDS = c.disp ? CAMBLK_DISP + 1 : CANDBLK + 1;  // Dims<TYPE>::CBS / CDS
  return PTZ_OK;
}

// Pair lists on the device (k_pairs) unless the round-2 kernels are asked for, the per-camera bitmaps do not fit in LDS, or
// PTZ_BA_GPU_STRUCT=0 (the host builder: 2.1 of its 3.6 ms per 170-view problem are these lists)
int32_t choose_pair_builder(CreateCtx& c)
{
  c.pairs_lds = sizeof(unsigned) * ((size_t)c.pre_max_cam * ((c.pre_max_cam_obs + 31) / 32) + 5 * (size_t)c.pre_max_cam + 8);
  const bool too_wide = c.pairs_lds > 150 * 1024 || c.pre_max_cam_obs > 65535;
  if (c.views && too_wide) return PTZ_ELIMIT;  // (a view is built on the device or not at all)
  c.gpu_pairs = c.views || (!env_flag("PTZ_BA_SCHUR_W", false) && !too_wide && env_flag("PTZ_BA_GPU_STRUCT", true));
  // PTZ_BA_GPU_STRUCT_CHECK=1 (tests): the host builds its lists as well and the device's must equal them word for word
  c.pairs_check = c.gpu_pairs && getenv("PTZ_BA_GPU_STRUCT_CHECK") != nullptr;
  return PTZ_OK;
}

// A view's scene: extents of the WHOLE rig (the real counts are the device's to find, and nothing is read back to size an array):
// pairs of the candidates, the rig's entries, at most max(runs per workgroup, pairs of a camera) runs per camera
int32_t bound_view_scene(ptz_ba_batch* b, const CreateCtx& c, int i, SceneDev& s)
{
  const ptz_rig_view& v = c.views[i];
  const int64_t pair_bound = (int64_t)v.n_cam * (v.n_cam - 1) / 2;
  const int64_t run_bound = (int64_t)v.n_cam * std::max(schur_threads_of(c.type), v.n_cam);
  if ((int64_t)b->total_ent + v.rig->ent_bound > 0x7fffffff || (int64_t)b->total_pair + pair_bound > 0x7fffffff ||
      (int64_t)b->total_run + run_bound > 0x7fffffff) return PTZ_ELIMIT;
  s.run_off = b->total_run; s.n_pair = 0;
  b->total_run += (int)run_bound; b->total_pair += (int)pair_bound; b->total_ent += (int)v.rig->ent_bound;
  for (int k = 0; k < v.n_cam; ++k) {
    b->max_cam_obs = std::max(b->max_cam_obs, v.rig->img_obs[v.cam_image[k]]);
    b->max_cam_ent = std::max(b->max_cam_ent, v.rig->img_ent[v.cam_image[k]]);
  }
  b->max_cam_pair = std::max(b->max_cam_pair, v.n_cam - 1);
  b->max_cam_run = std::max(b->max_cam_run, std::max(schur_threads_of(c.type), v.n_cam - 1));
  return PTZ_OK;
}

// One wave of scenes on the host threads; their entry lists go into the batch-wide array in one resize and a parallel copy
int32_t build_wave_entries(ptz_ba_batch* b, CreateCtx& c, int first, int wn, std::vector<PairBuild>& wave)
{
  build_scene_wave(c.problems, first, wn, c.n_threads, c.h, b->ray_perm.data(), wave, c.gpu_pairs && !c.pairs_check);
  std::vector<size_t> ent_at(wn);
  size_t at = c.h_ent.size();
  bool wave_ok = true;
  for (int k = 0; k < wn; ++k) { ent_at[k] = at; at += wave[k].ent.size(); wave_ok &= wave[k].err == PTZ_OK; }
  if (!wave_ok || at > 0x7fffffff) return PTZ_EINVAL;
  c.h_ent.resize(at);
  run_strided(std::min(c.n_threads, wn), [&](int t0, int step) {
    for (int k = t0; k < wn; k += step) {
      if (!wave[k].ent.empty()) memcpy(c.h_ent.data() + ent_at[k], wave[k].ent.data(), sizeof(unsigned) * wave[k].ent.size());
      std::vector<unsigned>().swap(wave[k].ent);
    }
  });
  return PTZ_OK;
}

// A packed scene: its pair lists appended to the batch's, entry positions made batch-wide
int32_t append_scene_pairs(ptz_ba_batch* b, CreateCtx& c, const PairBuild& pb, SceneDev& s)
{
  if (pb.err != PTZ_OK || (int64_t)b->total_ent + pb.n_ent > 0x7fffffff) return PTZ_EINVAL;
  c.h_pci.insert(c.h_pci.end(), pb.pci.begin(), pb.pci.end());
  c.h_pcj.insert(c.h_pcj.end(), pb.pcj.begin(), pb.pcj.end());
  c.h_pbrow.insert(c.h_pbrow.end(), pb.pbrow.begin(), pb.pbrow.end());
  for (int v : pb.pptr) c.h_pptr.push_back(b->total_ent + v);
  for (const uint2& r : pb.runs) c.h_runs.push_back(make_uint2(r.x + (unsigned)b->total_ent, r.y));
  c.h_prun.insert(c.h_prun.end(), pb.prun.begin(), pb.prun.end());
  s.run_off = b->total_run; s.n_pair = pb.n_pair;
  b->total_run += (int)pb.runs.size(); b->total_ent += (int)pb.n_ent; b->total_pair += pb.n_pair;
  b->max_cam_run = std::max(b->max_cam_run, pb.max_cam_run); b->max_cam_obs = std::max(b->max_cam_obs, pb.max_cam_obs);
  b->max_cam_ent = std::max(b->max_cam_ent, pb.max_cam_ent); b->max_cam_pair = std::max(b->max_cam_pair, pb.max_cam_pair);
  return PTZ_OK;
}

// Shared intrinsics groups of scene i (ids are arbitrary integers; members in ascending camera order; groups in order of their
// first member); a camera alone in its group needs nothing.  And the cameras' flags: which of a group counts, which carries the
// displacement block.  `total_grp`: the groups of the scenes before this one.
void scene_groups(ptz_ba_batch* b, CreateCtx& c, int i, SceneDev& s, int total_grp)
{
  const ptz_ba_problem& p = c.problems[i];
  s.grp_off = total_grp; s.n_grp = 0;
  std::vector<int> first(p.n_cam);
  for (int k = 0; k < p.n_cam; ++k) {
    first[k] = k;
    if (p.ic_of_cam)
      for (int m = 0; m < k; ++m)
        if (p.ic_of_cam[m] == p.ic_of_cam[k]) { first[k] = m; break; }
  }
  for (int k = 0; k < p.n_cam; ++k) b->first_of_group.push_back(b->total_cam + first[k]);
  std::vector<char> counted(p.n_cam, 0);  // group (by first member) already has its counting camera
  bool disp_counted = false;
  const int* camptr_s = c.h.camptr.data() + c.h.cam_base[i] + i;  // filled by build_pairs for this scene (views: no camera has residuals as far as the flags are concerned)
  for (int k = 0; k < p.n_cam; ++k) {
    const bool has_res = camptr_s[k + 1] > camptr_s[k];
    unsigned char flag = 0;
    if (has_res && !counted[first[k]]) { flag = 1; counted[first[k]] = 1; }
    if (c.disp && has_res && !disp_counted) { flag |= 2; disp_counted = true; }
    c.h_camflag.push_back(flag);
  }
  c.h_grpptr.push_back((int)c.h_grpmem.size());
  for (int k = 0; k < p.n_cam; ++k) {
    if (first[k] != k) continue;
    int members = 0;
    for (int m = k; m < p.n_cam; ++m) members += first[m] == k;
    if (members < 2) continue;
    for (int m = k; m < p.n_cam; ++m) if (first[m] == k) c.h_grpmem.push_back(m);
    c.h_grpptr.push_back((int)c.h_grpmem.size());
    c.h_grpcls.push_back(0);
    ++s.n_grp;
    c.any_shared = true;
  }
  if (c.disp) {  // the displacement block is one parameter of the whole problem: a group of all cameras, over the d slots
    for (int m = 0; m < p.n_cam; ++m) c.h_grpmem.push_back(m);
    c.h_grpptr.push_back((int)c.h_grpmem.size());
    c.h_grpcls.push_back(1);
    ++s.n_grp;
    c.any_shared = true;
  }
  b->max_grp = std::max(b->max_grp, s.n_grp);
}

// The scenes' places in the batch-wide arrays (SceneDev), the 2D-3D arrays, and per scene: the rig's bounds (views) or the host-built
// observation and pair lists (packed problems: built a wave of scenes at a time on up to 16 host threads, PTZ_BA_HOST_THREADS --
// the observation-side arrays are written in place, the pair lists appended here), then its intrinsics groups
int32_t create_layout(ptz_ba_batch* b, CreateCtx& c)
{
  const int n = c.n, NC = c.NC, has3d = c.has3d;
  const bool vm = c.views != nullptr;
  c.h.set_bases(n, c.problems);
  if (c.h.obs_base[n] > 0x7fffffff) return PTZ_EINVAL;
  if (!vm) { c.h.resize_all(n); b->ray_perm.resize(c.h.ray_base[n]); }
  else c.h.camptr.assign(c.h.cam_base[n] + n, 0);  // (read by the per-camera flags: see scene_groups)
  c.n_threads = env_int("PTZ_BA_HOST_THREADS", (int)std::min<unsigned>(16u, std::max(1u, std::thread::hardware_concurrency())), 1);
  const int wave_scenes = 4 * c.n_threads;
  PTZ_TRY(choose_pair_builder(c));
  std::vector<PairBuild> wave;
  int wave_first = 0, total_grp = 0;
  for (int i = 0; i < n; ++i) {
    const ptz_ba_problem& p = c.problems[i];
    SceneDev s;
    s.n_cam = p.n_cam; s.n_ray = p.n_ray; s.n_obs = (int)p.n_obs;
    s.cam_off = b->total_cam; s.ray_off = b->total_ray; s.obs_off = b->total_obs;
    s.pair_off = b->total_pair; s.ent_off = b->total_ent; s.part_off = b->total_chunk;
    s.n_chunk = (p.n_ray + b->ray_block - 1) / b->ray_block; s.n_wave = (p.n_ray + 63) / 64;
    s.n = NC * p.n_cam + 6 * has3d; s.idx = i;
    s.o3_off = b->total_o3; s.n_o3 = p.n_obs3d;
    for (int a = 0; a < p.n_obs3d; ++a) {
      c.h_o3uv.push_back(make_float2(p.obs3d_uv[2 * a], p.obs3d_uv[2 * a + 1]));
      c.h_o3cam.push_back(p.obs3d_cam[a]);
      for (int k = 0; k < 3; ++k) c.h_o3xyz.push_back(p.obs3d_xyz[3 * a + k]);
    }
    b->total_o3 += p.n_obs3d;
    if (vm) PTZ_TRY(bound_view_scene(b, c, i, s));
    else {
      const double tsb = now_ms();
      if (i >= wave_first + (int)wave.size()) {
        wave_first = i;
        PTZ_TRY(build_wave_entries(b, c, i, std::min(n - i, wave_scenes), wave));
      }
      PTZ_TRY(append_scene_pairs(b, c, wave[i - wave_first], s));
      c.ts_ent += now_ms() - tsb;
      wave[i - wave_first] = PairBuild();  // release this scene's lists
    }
    scene_groups(b, c, i, s, total_grp);
    total_grp += s.n_grp;
    b->total_cam += p.n_cam; b->total_ray += p.n_ray; b->total_obs += (int)p.n_obs; b->total_chunk += s.n_wave + 1;
    b->max_cam = std::max(b->max_cam, p.n_cam); b->max_ray = std::max(b->max_ray, p.n_ray);
    b->max_chunk = std::max(b->max_chunk, s.n_chunk); b->max_pair = std::max(b->max_pair, s.n_pair);
    b->max_n = std::max(b->max_n, s.n);
    b->scenes.push_back(s);
  }
  return PTZ_OK;
}

// ---- k_pairs' arguments, shared by the view stage (arrays at the rigs' bounds, nothing read back to size them) and the
// device-pairs stage (arrays sized exactly, from the totals it reads back)
void pairs_inputs(const ptz_ba_batch* b, PairsDev& pa)
{
  const Dev& d = b->d;
  memset(&pa, 0, sizeof(pa));
  pa.scene = d.scene; pa.obs_cam = d.obs_cam; pa.obs_ray = d.obs_ray; pa.ray_ptr = d.ray_ptr; pa.cam_ptr = d.cam_ptr; pa.cam_obs = d.cam_obs;
  pa.wpos = d.wpos;
  pa.max_runs = schur_threads_of(b->type);
}
// the pair, entry and run arrays, from the batch's totals as they stand
int32_t alloc_pair_arrays(ptz_ba_batch* b, PairsDev& pa)
{
  const size_t n = (size_t)b->n_scene, pairs = (size_t)b->total_pair, cams = (size_t)b->total_cam;
  PTZ_TRY(b->alloc(&pa.pci, pairs)); PTZ_TRY(b->alloc(&pa.pcj, pairs)); PTZ_TRY(b->alloc(&pa.pbrow, pairs));
  PTZ_TRY(b->alloc(&pa.pptr, pairs + n)); PTZ_TRY(b->alloc(&pa.prun, pairs + n));
  PTZ_TRY(b->alloc(&pa.campair, cams + n)); PTZ_TRY(b->alloc(&pa.camrun, cams + n));
  PTZ_TRY(b->alloc(&pa.runs, (size_t)b->total_run));
  return b->alloc(&pa.ent, (size_t)b->total_ent);
}
void publish_pairs(const PairsDev& pa, Dev& d)
{
  d.pair_ci = pa.pci; d.pair_cj = pa.pcj; d.pair_brow = pa.pbrow; d.pair_ptr = pa.pptr; d.pair_run = pa.prun;
  d.cam_pair = pa.campair; d.cam_run = pa.camrun; d.run_rec = pa.runs; d.ent = pa.ent;
}
// a scene's six totals as k_pair_scan leaves them: pairs, entries, runs, and the most pairs, entries, runs of one camera
void widen_pair_maxima(ptz_ba_batch* b, const int* t)
{
  b->max_pair = std::max(b->max_pair, t[0]);
  b->max_cam_pair = std::max(b->max_cam_pair, t[3]); b->max_cam_ent = std::max(b->max_cam_ent, t[4]); b->max_cam_run = std::max(b->max_cam_run, t[5]);
}

// ---- views: what the device is given of them
struct ViewInputs {
  std::vector<ViewDev> hv; std::vector<int> map, camimg, chunkoff;
  size_t trk_total = 0, chunk_total = 0;  // chunk_total: [chunks of 256 rays][cameras] counters of the views (k_view_hist), bounds from the rigs' track counts
  int max_trk = 0; bool block_sort = false;  // block_sort: one launch sorts a view's tracks (k_view_sort); else the batch-wide sort
};
int32_t view_inputs(const ptz_ba_batch* b, const CreateCtx& c, ViewInputs& vi)
{
  const int n = c.n;
  vi.hv.resize(n);
  int64_t view_key_top = 0;  // largest (longest candidate track bound) * cameras + cameras of the views: what the sort keys must hold
  for (int i = 0; i < n; ++i) {
    const ptz_rig* rg = c.views[i].rig;
    if (rg->device != b->device) return PTZ_EINVAL;
    ViewDev& v = vi.hv[i];
    v.trk_ptr = rg->d_trk_ptr; v.trk_img = rg->d_trk_img; v.trk_uv = rg->d_trk_uv;
    v.n_track = rg->n_track; v.n_img = rg->n_img; v.n_cam = c.views[i].n_cam;
    v.map_off = (int)vi.map.size(); v.trk_off = (int)vi.trk_total;
    v.n_ray = 0; v.n_obs = 0; v.max_len = 0;
    vi.map.insert(vi.map.end(), (size_t)rg->n_img, -1);
    for (int k = 0; k < v.n_cam; ++k) { vi.map[v.map_off + c.views[i].cam_image[k]] = k; vi.camimg.push_back(c.views[i].cam_image[k]); }
    vi.trk_total += (size_t)rg->n_track;
    vi.max_trk = std::max(vi.max_trk, rg->n_track);
    // the sort key of the internal ray order holds (longest - length) * cameras + first camera in 22 bits, the track in 24.  What
    // k_view_keys puts there is below (the view's longest candidate track) * cameras, and a candidate track is no longer than the
    // rig's longest track or the number of candidate images -- NOT the rig's mean length: one long track in a wide view would
    // otherwise spill into the bits of the view number, and the batch-wide sort would silently be a different order.
    // That bound belongs to the BATCH-WIDE sort (k_view_keys, taken when a rig has more than 16 384 tracks or on request);
    // the one-launch sort (k_view_sort) keeps a 32-bit key of its own per view, whose padding value 2 << bits(top) must fit: top < 2^29.
    view_key_top = std::max(view_key_top, (int64_t)std::min(rg->max_track_len, v.n_cam) * v.n_cam + v.n_cam);
    if (rg->n_track >= (1 << 24)) return PTZ_ELIMIT;
  }
  vi.block_sort = vi.max_trk <= 16384 && env_flag("PTZ_BA_VIEW_BLOCK_SORT", true);
  if (view_key_top >= (vi.block_sort ? ((int64_t)1 << 29) : ((int64_t)1 << 22))) return PTZ_ELIMIT;
  vi.chunkoff.resize(n);
  for (int i = 0; i < n; ++i) {
    vi.chunkoff[i] = (int)vi.chunk_total;
    vi.chunk_total += (size_t)((c.views[i].rig->n_track + 255) / 256) * c.views[i].n_cam;
    if (vi.chunk_total > 0x7fffffffu) return PTZ_ELIMIT;
  }
  return PTZ_OK;
}

// the views' internal ray order: one launch (a workgroup per view sorts its tracks) when every view fits, else the batch-wide sort
int32_t enqueue_view_sort(ptz_ba_batch* b, const ViewInputs& vi, const ViewBuild& vb, unsigned long long* key_out, int* val_out)
{
  const int n = b->n_scene;
  hipStream_t st = b->io;
  if (vi.block_sort) {
    (void)once_per_device(CAPS_VIEW_SORT, b->device, [] { (void)hipFuncSetAttribute((const void*)k_view_sort<16>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024); return true; });
    if (vi.max_trk <= 4096) hipLaunchKernelGGL(k_view_sort<4>, dim3(n), dim3(1024), sizeof(rocprim::block_radix_sort<unsigned, 1024, 4, int>::storage_type), st, vb, val_out);
    else hipLaunchKernelGGL(k_view_sort<16>, dim3(n), dim3(1024), sizeof(rocprim::block_radix_sort<unsigned, 1024, 16, int>::storage_type), st, vb, val_out);
    return PTZ_OK;
  }
  hipLaunchKernelGGL(k_view_keys, dim3((vi.max_trk + 255) / 256, n), dim3(256), 0, st, vb);
  unsigned end_bit = 47;
  while ((1u << (end_bit - 47)) < (unsigned)n) ++end_bit;
  size_t tmp_bytes = 0;
  // (the low 24 bits of a key are the track number and the keys are generated in (view, track) order: a STABLE sort on the bits
  //  above them gives the same order in four digit passes instead of seven)
  const unsigned begin_bit = 24;
  if (rocprim::radix_sort_pairs(nullptr, tmp_bytes, vb.key_in, key_out, vb.val_in, val_out, vi.trk_total, begin_bit, end_bit, st) != hipSuccess) return PTZ_ENODEVICE;
  char* tmp = nullptr;
  PTZ_TRY(b->alloc(&tmp, tmp_bytes + 256));
  if (rocprim::radix_sort_pairs((void*)tmp, tmp_bytes, vb.key_in, key_out, vb.val_in, val_out, vi.trk_total, begin_bit, end_bit, st) != hipSuccess) return PTZ_ENODEVICE;
  return PTZ_OK;
}

// The packed problems of the views, on the device (ptz_view_kernels.h): observations in the library's order, ray and camera lists,
// camera pairs (k_pairs as for any batch); one read-back at the end (counts, pair totals, the error word, tile adjacency), nothing
// in between.  `tc1`: when the stage began (PTZ_BA_DEBUG_TIMING).
int32_t create_view_structure(ptz_ba_batch* b, CreateCtx& c, double tc1)
{
  const int n = c.n;
  Dev& d = b->d;
  const int nt_e = chol_padded_order(b->max_n) / CHOL_NB;
  ViewInputs vi;
  PTZ_TRY(view_inputs(b, c, vi));
  const ViewDev* dviews_c = nullptr;
  const int *d_map = nullptr, *d_camimg = nullptr, *d_chunkoff = nullptr;
  StagedUpload up;
  up.add(b->scenes, &d.scene); up.add(vi.hv, &dviews_c);
  up.add(vi.map, &d_map); up.add(vi.camimg, &d_camimg); up.add(vi.chunkoff, &d_chunkoff);
  PTZ_TRY(up.commit(b, /*wait=*/false));
  ViewBuild vb;
  memset(&vb, 0, sizeof(vb));
  vb.views = const_cast<ViewDev*>(dviews_c); vb.scene = const_cast<SceneDev*>(d.scene);
  vb.cam_of_image = d_map; vb.cam_image = d_camimg; vb.chunk_off = d_chunkoff;
  if (b->max_cam <= VIEW_LDS_CAMS) PTZ_TRY(b->alloc(&vb.chunk_cnt, vi.chunk_total));  // (unused by the wide path)
  unsigned long long* key_out = nullptr;  // the batch-wide sort's outputs; val_out: the tracks of every view in ray order
  int* val_out = nullptr;
  const size_t trk = vi.trk_total, rays = (size_t)b->total_ray, cams = (size_t)b->total_cam, obs = (size_t)b->total_obs;
  PTZ_TRY(b->alloc(&vb.t_len, trk)); PTZ_TRY(b->alloc(&vb.t_first, trk)); PTZ_TRY(b->alloc(&vb.t_ext, trk));
  PTZ_TRY(b->alloc(&vb.key_in, trk)); PTZ_TRY(b->alloc(&vb.val_in, trk)); PTZ_TRY(b->alloc(&key_out, trk)); PTZ_TRY(b->alloc(&val_out, trk));
  PTZ_TRY(b->alloc(&vb.ray_trk, rays)); PTZ_TRY(b->alloc(&vb.ray_len, rays)); PTZ_TRY(b->alloc(&vb.cam_cnt, cams));
  PTZ_TRY(b->alloc(&vb.obs_uv, obs)); PTZ_TRY(b->alloc(&vb.obs_cam, obs)); PTZ_TRY(b->alloc(&vb.obs_ray, obs));
  PTZ_TRY(b->alloc(&vb.ray_ptr, rays + n)); PTZ_TRY(b->alloc(&vb.cam_ptr, cams + n));
  PTZ_TRY(b->alloc(&vb.cam_obs, obs)); PTZ_TRY(b->alloc(&vb.wpos, obs)); PTZ_TRY(b->alloc(&vb.cam_ray, obs));
  PTZ_TRY(b->alloc(&vb.cam_uv, obs)); PTZ_TRY(b->alloc(&vb.ray_w, rays)); PTZ_TRY(b->alloc(&vb.ray_perm, rays));
  d.obs_uv = vb.obs_uv; d.obs_cam = vb.obs_cam; d.obs_ray = vb.obs_ray; d.ray_ptr = vb.ray_ptr; d.cam_ptr = vb.cam_ptr; d.cam_obs = vb.cam_obs;
  d.wpos = vb.wpos; d.cam_ray = vb.cam_ray; d.cam_uv = vb.cam_uv; d.ray_w = vb.ray_w; b->d_ray_perm = vb.ray_perm;
  hipStream_t st = b->io;
  const dim3 gtrk((vi.max_trk + 255) / 256, n);
  const double tv0 = now_ms();
  hipLaunchKernelGGL(k_view_tracks, gtrk, dim3(256), 0, st, vb);
  hipLaunchKernelGGL(k_view_scan, dim3(n), dim3(1024), 0, st, vb);
  PTZ_TRY(enqueue_view_sort(b, vi, vb, key_out, val_out));
  const double tva = now_ms();
  hipLaunchKernelGGL(k_view_rays, gtrk, dim3(256), 0, st, vb, (const int*)val_out);
  hipLaunchKernelGGL(k_view_rayscan, dim3(n), dim3(1024), 0, st, vb, b->ray_block);
  // (PTZ_BA_DEBUG_VIEW_WIDE=1: the path of views wider than VIEW_LDS_CAMS for any view -- tests: the same lists)
  const bool view_wide = b->max_cam > VIEW_LDS_CAMS || env_flag("PTZ_BA_DEBUG_VIEW_WIDE", false);
  if (!view_wide) {  // camera-major lists by counting: chunk histograms, running sums, placement
    hipLaunchKernelGGL(k_view_hist, gtrk, dim3(256), sizeof(int) * (size_t)b->max_cam, st, vb);
    hipLaunchKernelGGL(k_view_chunkscan, dim3(n), dim3(1024), 0, st, vb);
    hipLaunchKernelGGL(k_view_place, gtrk, dim3(256), sizeof(unsigned long long) * 4 * (size_t)b->max_cam, st, vb);
  }
  else {
    hipLaunchKernelGGL(k_view_obs, gtrk, dim3(256), 0, st, vb);
    hipLaunchKernelGGL(k_view_camscan, dim3(n), dim3(1024), 0, st, vb);
    hipLaunchKernelGGL(k_view_camlists_wide, dim3(b->max_cam, n), dim3(256), 0, st, vb);
  }
  const double tvb = now_ms();
  // camera pairs, entry lists, runs: into arrays of the bounds' extents (no sizing read-back)
  PairsDev pa;
  pairs_inputs(b, pa);
  int *d_cnt = nullptr, *d_off3 = nullptr, *d_tot = nullptr;
  unsigned char* d_adj = nullptr;
  PTZ_TRY(b->alloc(&d_cnt, (size_t)3 * b->total_cam)); PTZ_TRY(b->alloc(&d_off3, (size_t)3 * b->total_cam));
  PTZ_TRY(b->alloc(&d_tot, (size_t)6 * n + 1));
  int* d_err = d_tot + 6 * n;
  PTZ_TRY(b->alloc(&d_adj, (size_t)n * nt_e * nt_e));
  pa.cam_cnt = d_cnt; pa.cam_off3 = d_off3; pa.scene_tot = d_tot; pa.err = d_err;
  PTZ_TRY(alloc_pair_arrays(b, pa));
  (void)once_per_device(CAPS_PAIRS, b->device, raise_pairs_caps);
  const double tvc = now_ms();
  if (hipMemsetAsync(d_err, 0, sizeof(int), st) != hipSuccess) return PTZ_ENODEVICE;
  hipLaunchKernelGGL(k_pairs<false>, dim3(b->max_cam, n), dim3(256), c.pairs_lds, st, pa);
  hipLaunchKernelGGL(k_pair_scan, dim3((n + 63) / 64), dim3(64), 0, st, d.scene, n, (const int*)d_cnt, d_off3, d_tot);
  hipLaunchKernelGGL(k_view_pairs_patch, dim3((n + 63) / 64), dim3(64), 0, st, vb.scene, n, (const int*)d_tot);
  hipLaunchKernelGGL(k_pairs<true>, dim3(b->max_cam, n), dim3(256), c.pairs_lds, st, pa);
  hipLaunchKernelGGL(k_view_adjacency, dim3(n), dim3(256), 0, st, d.scene, (const int*)pa.pci, (const int*)pa.pcj, c.NC, nt_e, d_adj);
  publish_pairs(pa, d);
  // the one read-back: the views' counts, the pair totals, the error word, the tile adjacency
  const double tvd = now_ms();
  std::vector<int> h_tot((size_t)6 * n + 1);
  c.h_adj.resize((size_t)n * nt_e * nt_e);
  hipError_t e = hipMemcpyAsync(vi.hv.data(), dviews_c, sizeof(ViewDev) * n, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(h_tot.data(), d_tot, sizeof(int) * (6 * n + 1), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(c.h_adj.data(), d_adj, c.h_adj.size(), hipMemcpyDeviceToHost, st);
  const double tv1 = now_ms();
  if (e == hipSuccess) e = stream_wait(st);
  if (c.dbg_t) fprintf(stderr, "[ptz_ba_create] views: allocations + upload %.3f ms, build enqueued in %.3f ms, waited %.3f ms for it | tracks..sort %.3f, rays..place %.3f, pair arrays %.3f, memset + pairs launches %.3f, copies back %.3f\n", tv0 - tc1, tv1 - tv0, now_ms() - tv1,
                       tva - tv0, tvb - tva, tvc - tvb, tvd - tvc, tv1 - tvd);
  b->release_staged();
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) { (void)hipGetLastError(); return PTZ_ENODEVICE; }
  if (h_tot[(size_t)6 * n]) return PTZ_EINVAL;  // an image twice in one track (tracks.cc:77)
  b->max_pair = 0; b->max_cam_pair = 0; b->max_cam_ent = 0; b->max_cam_run = 0;
  for (int i = 0; i < n; ++i) {
    if (vi.hv[i].n_obs <= 0 || vi.hv[i].n_ray <= 0) return PTZ_ENOOBS;  // no candidate observation: not a problem (:517); its own code, so that callers can tell it from a malformed view
    SceneDev& sd = b->scenes[i];
    const int* t = h_tot.data() + 6 * (size_t)i;
    sd.n_ray = vi.hv[i].n_ray; sd.n_obs = vi.hv[i].n_obs;
    sd.n_wave = (sd.n_ray + 63) / 64; sd.n_chunk = (sd.n_ray + b->ray_block - 1) / b->ray_block; sd.n_pair = t[0];
    widen_pair_maxima(b, t);
  }
  return PTZ_OK;
}

// packed problems: the host structure, in one staged upload
int32_t create_upload_structure(ptz_ba_batch* b, CreateCtx& c)
{
  Dev& d = b->d;
  StagedUpload up;
  up.add(b->scenes, &d.scene);
  up.add(c.h.uv, &d.obs_uv); up.add(c.h.cam, &d.obs_cam); up.add(c.h.ray, &d.obs_ray);
  up.add(c.h.rayptr, &d.ray_ptr); up.add(c.h.camptr, &d.cam_ptr);
  up.add(c.h.camobs, &d.cam_obs); up.add(c.h.wpos, &d.wpos); up.add(c.h.camray, &d.cam_ray); up.add(c.h.camuv, &d.cam_uv);
  up.add(c.h_pci, &d.pair_ci); up.add(c.h_pcj, &d.pair_cj); up.add(c.h_pbrow, &d.pair_brow); up.add(c.h_pptr, &d.pair_ptr);
  up.add(c.h.campair, &d.cam_pair); up.add(c.h.camrun, &d.cam_run);
  up.add(c.h_runs, &d.run_rec); up.add(c.h_prun, &d.pair_run); up.add(c.h_ent, &d.ent); up.add(c.h.w, &d.ray_w);
  up.add(c.h_o3uv, &d.o3_uv); up.add(c.h_o3xyz, &d.o3_xyz); up.add(c.h_o3cam, &d.o3_cam); up.add(b->ray_perm, &b->d_ray_perm);
  return up.commit(b);
}

// PTZ_BA_GPU_STRUCT_CHECK: what the host builder found, kept aside before the device's totals replace it
struct HostPairTotals { int pair, run, max_cam_pair, max_cam_ent, max_cam_run; std::vector<SceneDev> scenes; };
int32_t check_pairs_against_host(ptz_ba_batch* b, const CreateCtx& c, const PairsDev& pa, const HostPairTotals& chk)
{
  const int n = c.n;
  long bad = 0;
  if (chk.pair != b->total_pair || chk.run != b->total_run || chk.max_cam_pair != b->max_cam_pair || chk.max_cam_ent != b->max_cam_ent || chk.max_cam_run != b->max_cam_run) ++bad;
  for (int i = 0; i < n && !bad; ++i)
    if (chk.scenes[i].n_pair != b->scenes[i].n_pair || chk.scenes[i].pair_off != b->scenes[i].pair_off || chk.scenes[i].run_off != b->scenes[i].run_off) ++bad;
  auto cmp = [&](const void* dev, const void* host, size_t bytes, const char* name) {
    std::vector<unsigned char> tmp(bytes + 1);
    if (bytes && (hipMemcpyAsync(tmp.data(), dev, bytes, hipMemcpyDeviceToHost, b->io) != hipSuccess || stream_wait(b->io) != hipSuccess)) { ++bad; return; }
    if (bytes && memcmp(tmp.data(), host, bytes) != 0) { ++bad; fprintf(stderr, "[ptz_ba_create] device-built %s differs from the host builder's\n", name); }
  };
  if (!bad) {
    cmp(pa.pci, c.h_pci.data(), sizeof(int) * c.h_pci.size(), "pair_ci"); cmp(pa.pcj, c.h_pcj.data(), sizeof(int) * c.h_pcj.size(), "pair_cj");
    cmp(pa.pbrow, c.h_pbrow.data(), sizeof(int) * c.h_pbrow.size(), "pair_brow"); cmp(pa.pptr, c.h_pptr.data(), sizeof(int) * c.h_pptr.size(), "pair_ptr");
    cmp(pa.prun, c.h_prun.data(), sizeof(int) * c.h_prun.size(), "pair_run");
    cmp(pa.campair, c.h.campair.data(), sizeof(int) * c.h.campair.size(), "cam_pair"); cmp(pa.camrun, c.h.camrun.data(), sizeof(int) * c.h.camrun.size(), "cam_run");
    cmp(pa.runs, c.h_runs.data(), sizeof(uint2) * c.h_runs.size(), "run_rec"); cmp(pa.ent, c.h_ent.data(), sizeof(unsigned) * c.h_ent.size(), "ent");
  }
  else fprintf(stderr, "[ptz_ba_create] device-built pair totals differ from the host builder's\n");
  return bad ? PTZ_EINVAL : PTZ_OK;
}

// packed problems: camera pairs, entry lists and runs on the device (k_pairs) -- count, scan, read the totals back (the arrays are
// sized exactly), write; then the pairs' cameras come back for the tile structure
int32_t create_device_pairs(ptz_ba_batch* b, CreateCtx& c)
{
  const int n = c.n;
  Dev& d = b->d;
  PairsDev pa;
  pairs_inputs(b, pa);
  int *d_cnt = nullptr, *d_off3 = nullptr, *d_tot = nullptr, *d_err = nullptr;
  PTZ_TRY(b->alloc(&d_cnt, (size_t)3 * b->total_cam)); PTZ_TRY(b->alloc(&d_off3, (size_t)3 * b->total_cam));
  PTZ_TRY(b->alloc(&d_tot, (size_t)6 * n)); PTZ_TRY(b->alloc(&d_err, 1));
  pa.cam_cnt = d_cnt; pa.cam_off3 = d_off3; pa.scene_tot = d_tot; pa.err = d_err;
  (void)once_per_device(CAPS_PAIRS, b->device, raise_pairs_caps);
  if (hipMemsetAsync(d_err, 0, sizeof(int), b->io) != hipSuccess) return PTZ_ENODEVICE;
  hipLaunchKernelGGL(k_pairs<false>, dim3(b->max_cam, n), dim3(256), c.pairs_lds, b->io, pa);
  hipLaunchKernelGGL(k_pair_scan, dim3((n + 63) / 64), dim3(64), 0, b->io, d.scene, n, (const int*)d_cnt, d_off3, d_tot);
  std::vector<int> h_tot((size_t)6 * n + 1);
  hipError_t e = hipMemcpyAsync(h_tot.data(), d_tot, sizeof(int) * 6 * n, hipMemcpyDeviceToHost, b->io);
  if (e == hipSuccess) e = hipMemcpyAsync(h_tot.data() + 6 * n, d_err, sizeof(int), hipMemcpyDeviceToHost, b->io);
  if (e == hipSuccess) e = stream_wait(b->io);
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) { (void)hipGetLastError(); return PTZ_ENODEVICE; }
  if (h_tot[(size_t)6 * n]) return PTZ_EINVAL;  // an image twice in one track (tracks.cc:77)
  const HostPairTotals chk = {b->total_pair, b->total_run, b->max_cam_pair, b->max_cam_ent, b->max_cam_run,
                              c.pairs_check ? b->scenes : std::vector<SceneDev>()};
  if (c.pairs_check) { b->max_cam_pair = 0; b->max_cam_ent = 0; b->max_cam_run = 0; }
  b->total_pair = 0; b->total_run = 0; b->max_pair = 0;
  for (int i = 0; i < n; ++i) {
    SceneDev& sd = b->scenes[i];
    const int* t = h_tot.data() + 6 * (size_t)i;
    const int64_t ne = (i + 1 < n ? b->scenes[i + 1].ent_off : b->total_ent) - sd.ent_off;  // (the host's count of the scene's entries, from the track lengths)
    if (t[1] != ne || (int64_t)b->total_pair + t[0] > 0x7fffffff || (int64_t)b->total_run + t[2] > 0x7fffffff) return PTZ_EINVAL;
    sd.n_pair = t[0]; sd.pair_off = b->total_pair; sd.run_off = b->total_run;
    b->total_pair += t[0]; b->total_run += t[2];
    widen_pair_maxima(b, t);
  }
  if (copy_on(b->io, const_cast<SceneDev*>(d.scene), b->scenes.data(), sizeof(SceneDev) * n, hipMemcpyHostToDevice) != hipSuccess) return PTZ_ENODEVICE;
  PTZ_TRY(alloc_pair_arrays(b, pa));
  hipLaunchKernelGGL(k_pairs<true>, dim3(b->max_cam, n), dim3(256), c.pairs_lds, b->io, pa);
  publish_pairs(pa, d);
  if (c.pairs_check) PTZ_TRY(check_pairs_against_host(b, c, pa, chk));
  c.h_pci.resize(b->total_pair); c.h_pcj.resize(b->total_pair);
  e = b->total_pair ? hipMemcpyAsync(c.h_pci.data(), pa.pci, sizeof(int) * b->total_pair, hipMemcpyDeviceToHost, b->io) : hipSuccess;
  if (e == hipSuccess && b->total_pair) e = hipMemcpyAsync(c.h_pcj.data(), pa.pcj, sizeof(int) * b->total_pair, hipMemcpyDeviceToHost, b->io);
  if (e == hipSuccess) e = stream_wait(b->io);
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) { (void)hipGetLastError(); return PTZ_ENODEVICE; }
  return PTZ_OK;
}

// solver state -- parameters, linearisation, LM control -- and the reduced camera systems (the zero fills go on `io`, behind the structure)
int32_t alloc_solver_state(ptz_ba_batch* b, const CreateCtx& c)
{
  const int n = c.n, NC = c.NC, CBS = c.CBS, CDS = c.CDS, type = c.type;
  const bool disp = c.disp;
  Dev& d = b->d;
  d.tlw_stride = (size_t)n * 6;
  const size_t cams = (size_t)b->total_cam, rays = (size_t)b->total_ray, o3 = (size_t)b->total_o3;
  // T_l_w and the 2D-3D term
  PTZ_TRY(b->alloc(&d.tlw_x, 2 * d.tlw_stride)); PTZ_TRY(b->alloc(&b->tlw0, d.tlw_stride));
  d.tlwblk_stride = (size_t)n * TLWBLK;
  PTZ_TRY(b->alloc(&d.tlwblk, 2 * d.tlwblk_stride)); PTZ_TRY(b->alloc(&d.tlwcand, (size_t)n * TLWBLK));
  PTZ_TRY(b->alloc(&d.scale_t, (size_t)n * 6)); PTZ_TRY(b->alloc(&d.diag_t, (size_t)n * 6)); PTZ_TRY(b->alloc(&d.Ut, (size_t)n * 36));
  PTZ_TRY(b->alloc(&d.gt, (size_t)n * 6)); PTZ_TRY(b->alloc(&d.dt, (size_t)n * 6));
  PTZ_TRY(b->alloc(&d.Jc3, o3 * 2 * NC)); PTZ_TRY(b->alloc(&d.Jt3, o3 * 12)); PTZ_TRY(b->alloc(&d.r3, o3 * 2));
  if (hipMemsetAsync(b->tlw0, 0, sizeof(double) * d.tlw_stride, b->io) != hipSuccess) return PTZ_ENODEVICE;
  // parameters: both halves of the double-buffered state, and the initial one
  d.cam_stride = cams * 15; d.ray_stride = rays * 3;
  PTZ_TRY(b->alloc(&d.cam_x, 2 * d.cam_stride)); PTZ_TRY(b->alloc(&d.ray_x, 2 * d.ray_stride)); PTZ_TRY(b->alloc(&b->cam0, d.cam_stride));
  if (disp) {
    d.dsp_stride = cams * 3;
    PTZ_TRY(b->alloc(&d.dsp_x, 2 * d.dsp_stride)); PTZ_TRY(b->alloc(&b->dsp0, d.dsp_stride));
    if (hipMemsetAsync(b->dsp0, 0, sizeof(double) * d.dsp_stride, b->io) != hipSuccess) return PTZ_ENODEVICE;  // :655
  }
  PTZ_TRY(b->alloc(&b->ray0, d.ray_stride));
  // camera side of the linearisation
  d.camblk_stride = (cams * CBS + 2 + 1) & ~(size_t)1;
  PTZ_TRY(b->alloc(&d.camblk, 2 * d.camblk_stride)); PTZ_TRY(b->alloc(&d.candblk, cams * CDS + 2));
  PTZ_TRY(b->alloc(&d.scale_c, cams * NC)); PTZ_TRY(b->alloc(&d.scale_r, rays * 3));
  PTZ_TRY(b->alloc(&d.U, 2 * cams * NC * NC)); PTZ_TRY(b->alloc(&d.gc, 2 * cams * NC)); PTZ_TRY(b->alloc(&d.costc, 2 * cams));
  d.lin_cams = b->total_cam;
  PTZ_TRY(b->alloc(&d.diag_c, 2 * cams * NC)); PTZ_TRY(b->alloc(&d.dc, cams * NC)); PTZ_TRY(b->alloc(&d.dct, cams * (NC | 1) + 4));
  // ray side (two halves each: k_eval leaves the ray-side linearisation of its candidate in the half that LmState.cur does not select)
  d.V_stride = rays * 6; d.gr_stride = rays * 3; d.rayrec_stride = rays * 8; d.plin_stride = (size_t)b->total_chunk * 2;
  PTZ_TRY(b->alloc(&d.V, 2 * d.V_stride)); PTZ_TRY(b->alloc(&d.gr, 2 * d.gr_stride)); PTZ_TRY(b->alloc(&d.diag_r, rays * 3));
  PTZ_TRY(b->alloc(&d.E, rays * EZS));  // the rays' records, as EZS / 2 planes of 16-byte pieces (e_piece)
  d.e_stride = rays;
  d.shared = c.any_shared ? 1 : 0;
  if (c.any_shared) {
    PTZ_TRY(upload(b, c.h_grpptr, &d.grp_ptr));
    PTZ_TRY(upload(b, c.h_grpmem, &d.grp_mem));
    PTZ_TRY(upload(b, c.h_camflag, &d.cam_flag));
    if (disp) PTZ_TRY(upload(b, c.h_grpcls, &d.grp_cls));
    PTZ_TRY(b->alloc(&d.gfold, (size_t)b->total_cam * NC));
  }
  // W = Jc^T Jr rows are not materialised by the solver (k_schur rebuilds them from the rays); ptz_ba_batch_linearize allocates
  // them when a caller asks for them, PTZ_BA_SCHUR_W=1 brings round 2's kernels back for A/B measurements
  b->schur_w = env_flag("PTZ_BA_SCHUR_W", false);
  if (b->schur_w) PTZ_TRY(b->alloc(&d.W, (size_t)b->total_obs * (disp ? 24 : type == PTZ_BA_PTZRayFxfyDist ? 18 : 16)));  // room for the widest row stride
  PTZ_TRY(b->alloc(&d.rayrec, 2 * d.rayrec_stride)); PTZ_TRY(b->alloc(&d.partial, (size_t)b->total_chunk * 4)); PTZ_TRY(b->alloc(&d.partial_lin, 2 * d.plin_stride));
  d.ray_block = b->ray_block;
  // LM control
  PTZ_TRY(b->alloc(&d.camstep, cams * 2)); PTZ_TRY(b->alloc(&d.cam_gmax, 2 * cams)); PTZ_TRY(b->alloc(&d.tail_cnt, (size_t)2 * n));
  PTZ_TRY(b->alloc(&d.lm, (size_t)n)); PTZ_TRY(b->alloc(&d.active, (size_t)n)); PTZ_TRY(b->alloc(&d.ray_fail, (size_t)n));
  // reduced camera systems
  d.chol.count = n; d.chol.np = chol_padded_order(b->max_n);
  PTZ_TRY(b->alloc(&d.chol.A, (size_t)n * d.chol.np * d.chol.np));
  // the one-launch-per-column factorisation (a few scenes, or the last few active scenes of a large batch) publishes its
  // finished L tiles in a second matrix, indexed by launch slot: up to CHOL_CHAIN_SLOTS slots per scene group
  const int groups = std::max(1, std::min(b->n_group_hint(n), n));
  const size_t slots = (size_t)std::min(n, CHOL_CHAIN_SLOTS) * groups;
  PTZ_TRY(b->alloc(&d.chol.L, slots * d.chol.np * d.chol.np));
  if (hipMemsetAsync(d.chol.L, 0, sizeof(double) * slots * d.chol.np * d.chol.np, b->io) != hipSuccess) return PTZ_ENODEVICE;
  PTZ_TRY(b->alloc(&b->d_act, (size_t)n));
  const size_t ctl_ints = chol_chain_ctl_ints(d.chol.np) * groups;
  PTZ_TRY(b->alloc(&d.chol.chain_ctl, ctl_ints));
  if (hipMemsetAsync(d.chol.chain_ctl, 0, sizeof(int) * ctl_ints, b->io) != hipSuccess) return PTZ_ENODEVICE;
  const size_t diag_tiles = (size_t)n * (d.chol.np / CHOL_NB);
  PTZ_TRY(b->alloc(&d.chol.Ldiag, diag_tiles * CHOL_NB * CHOL_NB)); PTZ_TRY(b->alloc(&d.chol.Dinv, diag_tiles * 4 * 16 * 16));
  PTZ_TRY(b->alloc(&d.chol.Linv, diag_tiles * CHOL_NB * CHOL_NB)); PTZ_TRY(b->alloc(&d.chol.fail, (size_t)n));
  d.chol.active = d.active;
  return b->alloc(&d.yc, (size_t)n * d.chol.np);
}

// Tile mask of scene i's reduced camera system, before any reordering: cameras that share a track couple their tiles, the T_l_w
// block and the rhs row couple to everything.  Views: marked on the device by the same rule (k_view_adjacency).  Returns the first
// dense tile row.
int scene_tile_mask(const ptz_ba_batch* b, const CreateCtx& c, int i, int nt, unsigned char* m0)
{
  const SceneDev& sd = b->scenes[i];
  const int NC = c.NC;
  auto tile_lo = [&](int cam) { return (cam * NC) / CHOL_NB; };
  auto tile_hi = [&](int cam) { return (cam * NC + NC - 1) / CHOL_NB; };
  if (c.views) memcpy(m0, c.h_adj.data() + (size_t)i * nt * nt, (size_t)nt * nt);
  else {
    memset(m0, 0, (size_t)nt * nt);
    for (int k = 0; k < sd.n_cam; ++k)
      for (int a = tile_lo(k); a <= tile_hi(k); ++a)
        for (int e = tile_lo(k); e <= a; ++e) m0[a * nt + e] = 1;
    for (int p = 0; p < sd.n_pair; ++p) {
      const int ci = c.h_pci[sd.pair_off + p], cj = c.h_pcj[sd.pair_off + p];
      for (int a = tile_lo(ci); a <= tile_hi(ci); ++a)
        for (int e = tile_lo(cj); e <= tile_hi(cj); ++e) {
          if (a >= e) m0[a * nt + e] = 1; else m0[e * nt + a] = 1;
        }
    }
  }
  // shared intrinsics: the fold puts a dense row / column at every group's representative (its last camera)
  if (c.any_shared) {
    const int* gp = c.h_grpptr.data() + sd.grp_off + i;
    for (int g = 0; g < sd.n_grp; ++g) {
      const int rep = c.h_grpmem[gp[g + 1] - 1];
      for (int a = tile_lo(rep); a <= tile_hi(rep); ++a) {
        for (int e = 0; e <= a; ++e) m0[a * nt + e] = 1;
        for (int r = a; r < nt; ++r) m0[r * nt + a] = 1;
      }
    }
  }
  // dense rows: the global block (if any) and the rhs row, index n_cam * NC .. n
  const int first_dense = (sd.n_cam * NC) / CHOL_NB;
  for (int a = first_dense; a < nt; ++a)
    for (int e = 0; e <= a; ++e) m0[a * nt + e] = 1;
  return first_dense;
}

// The systems' orders and their tile structure, elimination order, step schedule and back-substitution lists: ONE upload.
// The tiles are eliminated in the order plan_dissection picks (arcs of a ring side by side, separators last) when that shortens
// the dependent chain of the factorisation; Dev::tperm carries the order to the kernels, CholBatch::sched the steps.
int32_t create_tile_plan(ptz_ba_batch* b, const CreateCtx& c)
{
  const int n = c.n;
  Dev& d = b->d;
  StagedUpload up;
  std::vector<int> hn(n);
  for (int i = 0; i < n; ++i) hn[i] = b->scenes[i].n;
  up.add(hn, &d.chol.n);
  std::vector<unsigned char> hm;
  std::vector<int> h_tperm, h_sched, h_groups; std::vector<BsItem> h_items;
  if (!getenv("PTZ_BA_DENSE_CHOL")) {
    const int nt = d.chol.np / CHOL_NB;
    bool dissect = true, nested = true;
    if (const char* e = getenv("PTZ_BA_ORDER")) { dissect = strcmp(e, "natural") != 0; nested = strcmp(e, "flat") != 0; }
    hm.assign((size_t)n * nt * nt, 0);
    h_tperm.resize((size_t)n * nt); h_sched.resize((size_t)n * nt * CHOL_STEP_COLS);
    int max_steps = 0; bool any_plan = false;
    std::vector<unsigned char> m0((size_t)nt * nt);
    for (int i = 0; i < n; ++i) {
      const int first_dense = scene_tile_mask(b, c, i, nt, m0.data());
      int* perm = h_tperm.data() + (size_t)i * nt;
      int* sched = h_sched.data() + (size_t)i * nt * CHOL_STEP_COLS;
      int lane_a = 0, lane_b = 0;
      const bool planned = dissect && b->scenes[i].n_grp == 0 && plan_dissection(nt, first_dense, m0.data(), perm, &lane_a, &lane_b, nested);
      if (!planned) for (int t = 0; t < nt; ++t) perm[t] = t;
      if (planned) any_plan = true;
      const int steps = fill_and_schedule(nt, m0.data(), planned ? perm : nullptr, hm.data() + (size_t)i * nt * nt, sched);
      max_steps = std::max(max_steps, steps);
      if ((int)b->sched_kmin.size() < steps) b->sched_kmin.resize(steps, nt);
      for (int st = 0; st < steps; ++st) b->sched_kmin[st] = std::min(b->sched_kmin[st], sched[CHOL_STEP_COLS * st]);  // (slot 0 of a step holds its smallest column)
      if (c.dbg_t && i == 0) fprintf(stderr, "[ptz_ba_create] scene 0: %d tiles, elimination %s: lanes %d + %d, %d steps\n", nt, planned ? "dissected" : "natural", lane_a, lane_b, steps);
    }
    up.add(hm, &d.chol.tmask);
    if (any_plan) {
      up.add(h_tperm, &d.tperm);  // (d.chol.xperm = d.tperm once the upload has placed it)
      up.add(h_sched, &d.chol.sched);
      d.chol.n_steps = max_steps;
      d.chol.sched_kmin = b->sched_kmin.data();
    }
    // the back-substitution's work list, per scene (the kernel would otherwise make it itself, every launch: ~6 us of one wave)
    const int mg = chol_backsolve_max_groups(d.chol.np);
    const char* e = getenv("PTZ_BA_BACKSOLVE_HOST_LIST");  // 0: the kernel makes the list itself (tests: the same list, the same bits)
    // (mg <= 1024: chol_backsolve_kernel keeps the kinds of the host list's groups in a fixed array of that many)
    if ((!e || atoi(e) != 0) && mg <= 1024 && sizeof(double) * ((size_t)d.chol.np + 1024) + sizeof(BsItem) * 4 * (size_t)mg <= 150 * 1024) {  // (the kernel's own list form applies)
      h_items.resize((size_t)n * 4 * mg);
      h_groups.resize(n);
      // a few systems: the two arcs of a dissected system on a workgroup each (chol_backsolve_arcs); PTZ_BA_BACKSOLVE_SPLIT=0: one workgroup
      const char* es = getenv("PTZ_BA_BACKSOLVE_SPLIT");
      const bool want_split = any_plan && n <= 8 && nt <= 64 && !(es && atoi(es) == 0);
      for (int i = 0; i < n; ++i) {
        bool split = false;
        h_groups[i] = chol_backsolve_plan(d.chol.np, b->scenes[i].n, hm.data() + (size_t)i * nt * nt,
                                          any_plan ? h_sched.data() + (size_t)i * nt * CHOL_STEP_COLS : nullptr, max_steps, h_items.data() + (size_t)i * 4 * mg,
                                          want_split, &split);
        if (split) d.chol.bs_split = 1;
      }
      up.add(h_items, &d.chol.bs_items);
      up.add(h_groups, &d.chol.bs_groups);
    }
    // tiles outside the structure are never written again: zero everything once (the block may be a recycled one)
    if (hipMemsetAsync(d.chol.A, 0, sizeof(double) * (size_t)n * d.chol.np * d.chol.np, b->io) != hipSuccess) return PTZ_ENODEVICE;
  }
  PTZ_TRY(up.commit(b, /*wait=*/false));  // (the hand-over event at the end of create ends it)
  d.chol.xperm = d.tperm;
  return PTZ_OK;
}

// The solver's options, the knobs of the pass pipeline, the scene groups with their streams and control blocks, the launch shapes
int32_t create_pipeline(ptz_ba_batch* b, const CreateCtx& c)
{
  const int n = c.n;
  const ptz_lm_options& o = c.o;
  Dev& d = b->d;
  d.cam_x0 = b->cam0; d.ray_x0 = b->ray0;
  d.opt.max_num_iterations = o.max_num_iterations; d.opt.max_consecutive_invalid = o.max_num_consecutive_invalid_steps;
  d.opt.jacobi_scaling = o.jacobi_scaling; d.opt.min_relative_decrease = o.min_relative_decrease;
  d.opt.initial_radius = o.initial_trust_region_radius; d.opt.max_radius = o.max_trust_region_radius; d.opt.min_radius = o.min_trust_region_radius;
  d.opt.min_lm_diagonal = o.min_lm_diagonal; d.opt.max_lm_diagonal = o.max_lm_diagonal;
  d.opt.function_tolerance = o.function_tolerance; d.opt.gradient_tolerance = o.gradient_tolerance; d.opt.parameter_tolerance = o.parameter_tolerance;
  // Two independently pipelined groups for batches: the groups drift out of phase, so the latency-bound block-column chain of
  // one overlaps the throughput kernels of the other (measured on the 256-scene C2 batch: 35.0k -> 36.8k LM it/s; four groups
  // 36.2k, six slower than one).  Small batches stay in one group.
  b->n_group = b->n_group_hint(n);
  b->lookahead = env_flag("PTZ_BA_LOOKAHEAD", n >= 8);  // look-ahead pays for mid-size batches; a single scene is better off with fewer launches
  // batches: left-looking column updates (half the tile traffic, no trailing-update launches); a few scenes: right-looking,
  // whose updates of one column step spread over many workgroups instead of looping inside one (measured: 256 scenes
  // 141.9 -> 137.8 ms, single scene 16.4 -> 19.4 ms with the left-looking form)
  b->left_looking = env_flag("PTZ_BA_CHOL_LEFT", n >= 8);
  // (small batches -- the view batches of the incremental pipeline converge in two or three passes -- run two ahead: every pass
  //  enqueued beyond the last real one is a dozen empty launches; large batches, whose passes last milliseconds, keep three)
  b->ahead = env_int("PTZ_BA_AHEAD", n <= 32 ? 2 : 3, 1);
  // compacted (item, slot) launches deal their workgroups over the XCDs by the device's live count (ptz_xcd_map.h); 0: by the grid
  d.xcd_live = d.chol.xcd_live = env_flag("PTZ_BA_XCD_LIVE", true);
  d.debug_stall = env_int("PTZ_BA_DEBUG_STALL", d.debug_stall, 0);
  d.chol.chain_spin_limit = env_int("PTZ_BA_DEBUG_CHAIN_SPIN", d.chol.chain_spin_limit, 0);  // tests: hand-overs that time out
  b->use_graph = env_flag("PTZ_BA_GRAPH", b->use_graph);
  b->ctl_groups = std::max(1, std::min(b->n_group, n));
  if (b->alloc(&b->d_ctl, (size_t)4 * b->ctl_groups) != PTZ_OK ||
      ptzpool::pinned_acquire(sizeof(int) * 4 * b->ctl_groups, (void**)&b->h_ctl) != hipSuccess ||
      hipHostGetDevicePointer((void**)&b->h_ctl_dev, b->h_ctl, 0) != hipSuccess)
    return PTZ_ENODEVICE;
  make_groups(b);
  b->stream = b->streams.empty() ? nullptr : b->streams[0];
  if (b->stream == nullptr || ptzpool::event_acquire(b->device, true, &b->ev0) != hipSuccess ||
      ptzpool::event_acquire(b->device, true, &b->ev1) != hipSuccess)
    return PTZ_ENODEVICE;
  // ---- the launch-shape ladder (PassShape): the full size, then compacted shapes
  const int NC = c.NC, CBS = c.CBS, CDS = c.CDS;
  // kernels that stage camera tables need > 64 KiB of dynamic LDS for large rigs
  // Rigs whose camera tables do not fit in LDS (the 160 KiB hold ~340 cameras) read them from global memory instead: the
  // reference has no cap on the number of views (ptzray_optimizer.cc:799-885)
  b->gtab = env_flag("PTZ_BA_GLOBAL_TABLES", sizeof(double) * ((size_t)b->max_cam * (CBS + CDS + (NC | 1)) + 16 + 18) + (size_t)OBS_PREFETCH_BYTES * 256 > 160 * 1024);
  b->compaction = env_flag("PTZ_BA_COMPACT", true);
  b->exact_fit = env_flag("PTZ_BA_EXACT_FIT", true);
  auto make_shape = [&](int slots, bool compact) {
    PassShape sh;
    sh.slots = slots; sh.compact = compact;
    sh.ray_block = ray_block_for(slots);
    sh.small_blocks = sh.ray_block <= 256;
    // one launch per factorisation (chol_chain_kernel) or per step (chol_col_step_kernel) for a few systems; up to CHOL_CHAIN_SLOTS when
    // the one-launch form takes them (chol_chain_fits)
    sh.fused = (slots <= 8 || chol_chain_fits(slots, b->d.chol.np)) && env_flag("PTZ_BA_CHOL_FUSED", true);
    // a few scenes: LM control and the camera update ride in the tails / prologue of k_eval and k_lin_cam (three launches less per pass)
    sh.fuse_ctl = slots <= 8 && sh.small_blocks && !b->gtab && env_flag("PTZ_BA_FUSE_CTL", true);
    sh.eval_lanes = (sh.fuse_ctl && sh.ray_block <= 128 && env_int("PTZ_BA_EVAL_LANES", 4, 1) == 4) ? 4 : 1;  // (tests: the same bits either way)
    sh.max_chunk = (b->max_ray + sh.ray_block - 1) / sh.ray_block;
    const size_t obs_lds = sh.small_blocks ? (size_t)OBS_PREFETCH_BYTES * sh.ray_block : 0;
    if (b->gtab) { sh.eval_smem = sizeof(double) * 16 + obs_lds + 16; sh.lin_smem = obs_lds + 16; }
    else {
      sh.eval_smem = sizeof(double) * ((size_t)b->max_cam * (CBS + CDS + (NC | 1)) + 16 + 18) + obs_lds;
      sh.lin_smem = sizeof(double) * ((size_t)b->max_cam * CBS + 6) + obs_lds;
    }
    return sh;
  };
  b->shapes.clear();
  b->shapes.push_back(make_shape(n, false));  // (its ray_block is the batch's: ray_block_for(n))
  // (two slots: the last rigs of a large batch get the one-launch factorisation, chol_chain_kernel; a batch of up to eight keeps
  //  its single shape -- a second one costs it a k_compact launch per pass)
  for (int sl = n > 8 ? 2 : 8; sl < n; sl *= 4) b->shapes.push_back(make_shape(sl, true));
  return PTZ_OK;
}

// Which Schur kernel, where its T table lives, and the limits of what LDS holds
int32_t create_schur_limits(ptz_ba_batch* b, const CreateCtx& c)
{
  const int NC = c.NC, type = c.type;
  // k_schur keeps a camera's T_a rows in LDS (up to ~1700 observations of one view); beyond that the table goes to global
  // memory.  What remains is the 16-bit position inside the camera-pair entry records: 65535 observations per view.
  if (b->max_cam_obs > 65535) return PTZ_ELIMIT;
  // (also when a view has more runs than a workgroup has threads -- more pairs than that: the several rounds k_schur then needs
  // cannot reuse the table's LDS space for their sums)
  const int NW2d = NC - ((c.has3d && type != PTZ_BA_PTZRayFxfyDist) ? 1 : 0);  // Dims<TYPE>::NW
  // PTZRay: the factored rows of k_schur_f (8 doubles per observation instead of 15, and no copy of the entry list: four
  // workgroups per compute unit for views of up to ~560 observations, three beyond, and the LDS table holds views of ~2000
  // observations); PTZ_BA_SCHUR_F=0 keeps k_schur (A/B measurements)
  b->schur_f = type == PTZ_BA_PTZRay && !b->schur_w && env_flag("PTZ_BA_SCHUR_F", true);
  const int frow = b->schur_f ? SCHUR_F_ROW : 0;
  b->d.e_fold = b->schur_f ? 1 : 0;
  for (auto& dgp : b->dg) dgp.e_fold = b->d.e_fold;
  // k_schur stages a camera's entry list in LDS; k_schur_f reads its runs from global memory
  b->schur_lds_ent = b->schur_f ? 0 : b->max_cam_ent;
  b->d.schur_ent_cap = b->schur_lds_ent;
  for (auto& dgp : b->dg) dgp.schur_ent_cap = b->schur_lds_ent;
  // PTZ_BA_SCHUR_WG4=0: k_schur_f's launches ask for more LDS than a quarter of a compute unit's, which holds the same binary
  // at three workgroups per compute unit (A/B measurements: what the occupancy gives, apart from the restructured loads)
  b->schur_wg4 = env_flag("PTZ_BA_SCHUR_WG4", true);
  b->schur_tg = schur_lds_bytes(b->max_cam_obs, NC, b->d.chol.np, b->schur_w, schur_threads_of(type), NW2d, b->schur_lds_ent, frow) > 160 * 1024 ||
                (!b->schur_w && b->max_cam_run > schur_threads_of(type));
  // a view with more pair entries than the LDS copy of its list holds (~60 000)
  if (!b->schur_w && schur_lds_bytes(0, NC, b->d.chol.np, false, schur_threads_of(type), NW2d, b->schur_lds_ent, frow) > 160 * 1024) return PTZ_ELIMIT;
  b->schur_tg = env_flag("PTZ_BA_SCHUR_GLOBAL_T", b->schur_tg);
  if (b->schur_tg) {
    PTZ_TRY(b->alloc(&b->d.Tbuf, (size_t)b->total_obs * ((NC * 3 + 3) | 1)));
    for (auto& dgp : b->dg) dgp.Tbuf = b->d.Tbuf;
  }
  if (b->shapes[0].eval_smem > 160 * 1024 || b->shapes[0].lin_smem > 160 * 1024) return PTZ_ELIMIT;
  if (c.dbg_t && b->schur_f && !b->schur_tg) {  // PTZ_BA_DEBUG_TIMING: the residency the runtime reports for the batch's k_schur_f launches
    const size_t smem = schur_launch_lds(b, NC, NW2d, b->d.chol.np, schur_threads_of(type));
    int wg = 0;
    const hipError_t e = c.has3d ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&wg, k_schur_f<4, false>, 256, smem)
                                 : hipOccupancyMaxActiveBlocksPerMultiprocessor(&wg, k_schur_f<0, false>, 256, smem);
    fprintf(stderr, "[ptz_ba] k_schur_f: %zu bytes of LDS for views of up to %d observations, %d workgroups per compute unit%s\n", smem, b->max_cam_obs,
            wg, e == hipSuccess ? "" : " (occupancy query failed)");
  }
  return PTZ_OK;
}

// dynamic LDS caps of the pass kernels, at the hardware limit
bool raise_pass_caps()
{
  bool attr_ok = true;
  auto raise_cap = [&](const void* fn) {
    hipFuncAttributes fa;
    if (hipFuncGetAttributes(&fa, fn) != hipSuccess) { attr_ok = false; return; }
    const int cap = 160 * 1024 - (int)fa.sharedSizeBytes;  // the statically declared part counts against the same 160 KB
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, cap) != hipSuccess) attr_ok = false;
  };
#define PTZ_SET_ATTR(T)                                                                                     \
  raise_cap((const void*)k_schur<T, false>); raise_cap((const void*)k_schur<T, true>);                      \
  raise_cap((const void*)k_schur_w<T, false>); raise_cap((const void*)k_schur_w<T, true>);                  \
  raise_cap((const void*)k_eval<T, true, false>); raise_cap((const void*)k_eval<T, false, false>);          \
  raise_cap((const void*)k_lin_ray<T, true, false>); raise_cap((const void*)k_lin_ray<T, false, false>);
  raise_cap((const void*)k_eval<0, true, false, true>); raise_cap((const void*)k_eval<1, true, false, true>); raise_cap((const void*)k_eval<2, true, false, true>);
  raise_cap((const void*)k_eval<0, true, false, true, 4>); raise_cap((const void*)k_eval<1, true, false, true, 4>); raise_cap((const void*)k_eval<2, true, false, true, 4>);
  raise_cap((const void*)k_schur_f<0, false>); raise_cap((const void*)k_schur_f<0, true>);
  raise_cap((const void*)k_schur_f<4, false>); raise_cap((const void*)k_schur_f<4, true>);
  PTZ_SET_ATTR(0) PTZ_SET_ATTR(1) PTZ_SET_ATTR(2) PTZ_SET_ATTR(3) PTZ_SET_ATTR(4) PTZ_SET_ATTR(5) PTZ_SET_ATTR(6) PTZ_SET_ATTR(7)
#undef PTZ_SET_ATTR
  return attr_ok;
}
}  // namespace

// views == nullptr: the n packed problems.  Else: the packed problems of n views of resident rigs, built on the device
// (ptz_view_kernels.h) -- the structure arrays then have the extents of the WHOLE rigs (nothing is read back to size them),
// each scene's real counts live in its SceneDev.
static int32_t create_impl(int32_t n, const ptz_ba_problem* problems, const ptz_rig_view* views, int32_t view_type, const ptz_lm_options* opt,
                           ptz_ba_batch** out)
{
  *out = nullptr;
  const double tc0 = now_ms();
  CreateCtx c;
  PTZ_TRY(create_validate(n, problems, views, view_type, opt, c));
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= c.o.device_id) return PTZ_ENODEVICE;
  PTZ_DEVICE_GUARD(c.o.device_id);
  BatchOwner owner(new ptz_ba_batch());  // from here on every return destroys what has been built
  ptz_ba_batch* b = owner.get();
  b->has3d = c.has3d; b->views_mode = views != nullptr;
  b->n_scene = n; b->type = c.type; b->nc = c.NC; b->opt = c.o; b->device = c.o.device_id;
  if (ptzpool::stream_acquire(b->device, &b->io) != hipSuccess) return PTZ_ENODEVICE;
  b->ray_block = ray_block_for(n);
  PTZ_TRY(create_layout(b, c));
  const double tc1 = now_ms();
  memset(&b->d, 0, sizeof(b->d)); b->d.n_scene = n;
  if (views) PTZ_TRY(create_view_structure(b, c, tc1));
  else {
    PTZ_TRY(create_upload_structure(b, c));
    if (c.gpu_pairs) PTZ_TRY(create_device_pairs(b, c));
  }
  PTZ_TRY(alloc_solver_state(b, c));
  const double tc2 = now_ms();
  PTZ_TRY(create_tile_plan(b, c));
  PTZ_TRY(create_pipeline(b, c));
  PTZ_TRY(create_schur_limits(b, c));
  if (!once_per_device(CAPS_PASS, b->device, raise_pass_caps)) { (void)hipGetLastError(); return PTZ_ENODEVICE; }
  // The zero fills and the staged upload are still in flight on `io`: the batch's first stream waits for them ON THE DEVICE (every
  // later entry point works on that stream or behind it), the host does not -- it goes on to the caller's set_state / solve while
  // the device finishes the structure.  (The staging blocks are released behind the next host-side wait: solve, destroy.)
  if (ptzpool::event_acquire(b->device, false, &b->create_ev) != hipSuccess || hipEventRecord(b->create_ev, b->io) != hipSuccess ||
      hipStreamWaitEvent(b->stream, b->create_ev, 0) != hipSuccess) {
    (void)hipGetLastError(); return PTZ_ENODEVICE;
  }
  if (c.dbg_t) fprintf(stderr, "[ptz_ba_create] host structure %.2f ms (pair entries %.2f), uploads + allocations %.2f ms, mask + rest %.2f ms\n", tc1 - tc0, c.ts_ent, tc2 - tc1, now_ms() - tc2);
  *out = owner.release();
  return PTZ_OK;
}

// the ray order of a batch built from views lives on the device: fetched when a host-side entry point needs it
static int32_t ensure_host_ray_perm(ptz_ba_batch* b)
{
  if (!b->ray_perm.empty() || !b->d_ray_perm) return PTZ_OK;
  b->ray_perm.resize((size_t)b->total_ray);
  if (copy_on(b->stream, b->ray_perm.data(), b->d_ray_perm, sizeof(int) * b->ray_perm.size(), hipMemcpyDeviceToHost) != hipSuccess) return PTZ_ENODEVICE;
  return PTZ_OK;
}

int32_t ptz_ba_batch_set_state(ptz_ba_batch* b, const double* cam, const double* ray, const double* tlw)
{
  if (!b || !cam || !ray) return PTZ_EINVAL;
  PTZ_DEVICE_GUARD(b->device);
  if (int32_t rcp = ensure_host_ray_perm(b)) return rcp;
  // cameras (a shared block starting from its first camera's values), rays in the library's order and T_l_w are put together in
  // ONE pinned block, sent with three asynchronous copies and waited for ONCE (three staged copies with a wait each cost the
  // lock-step PTZ-IBA 0.4 ms per bundle adjustment); batches whose state is larger than the staging limit copy array by array
  const size_t nc = (size_t)15 * b->total_cam, nr = (size_t)3 * b->total_ray, nt = (size_t)6 * b->n_scene;
  const size_t bytes = sizeof(double) * (nc + nr + nt);
  void* pin = nullptr;
  std::vector<double> heap;
  double* st = nullptr;
  if (bytes <= ((size_t)32 << 20) && ptzpool::pinned_acquire(bytes, &pin) == hipSuccess) st = static_cast<double*>(pin);
  else { (void)hipGetLastError(); heap.resize(nc + nr + nt); st = heap.data(); }
  double *c = st, *r = st + nc, *t = st + nc + nr;
  memcpy(c, cam, sizeof(double) * nc);
  if (b->d.shared) {
    // a shared block starts from its first camera's values (intrinsics_param_.insert, ptzray_optimizer.cc:645-650)
    for (int i = 0; i < b->total_cam; ++i) {
      const int f = b->first_of_group[i];
      if (f == i) continue;
      for (int k = 0; k < 15; ++k)
        if (k < 4 || k >= 10) c[15 * (size_t)i + k] = c[15 * (size_t)f + k];
    }
  }
  for (const SceneDev& sd : b->scenes)
    for (int j = 0; j < sd.n_ray; ++j) {
      const double* src = ray + 3 * ((size_t)sd.ray_off + b->ray_perm[sd.ray_off + j]);
      double* dst = r + 3 * ((size_t)sd.ray_off + j);
      dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
    }
  if (tlw) memcpy(t, tlw, sizeof(double) * nt);
  else memset(t, 0, sizeof(double) * nt);
  hipError_t e = hipMemcpyAsync(b->cam0, c, sizeof(double) * nc, hipMemcpyHostToDevice, b->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(b->ray0, r, sizeof(double) * nr, hipMemcpyHostToDevice, b->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(b->tlw0, t, sizeof(double) * nt, hipMemcpyHostToDevice, b->stream);
  if (e == hipSuccess) e = stream_wait(b->stream);
  ptzpool::pinned_release(pin);
  PTZ_HIP_TRY(e);
  b->has_state = true;
  return PTZ_OK;
}

int32_t ptz_ba_batch_solve(ptz_ba_batch* b, ptz_lm_summary* summaries)
{
  if (!b || !b->has_state) return PTZ_EINVAL;
  clear_stale_error(__func__);
  PTZ_DEVICE_GUARD(b->device);
  switch (b->type + 4 * b->has3d) {  // Dims<TYPE>
    case 0: return solve_impl<0>(b, summaries);
    case 1: return solve_impl<1>(b, summaries);
    case 2: return solve_impl<2>(b, summaries);
    case 3: return solve_impl<3>(b, summaries);
    case 4: return solve_impl<4>(b, summaries);
    case 5: return solve_impl<5>(b, summaries);
    case 6: return solve_impl<6>(b, summaries);
    default: return solve_impl<7>(b, summaries);
  }
}

int32_t ptz_ba_batch_get_state(ptz_ba_batch* b, double* cam, double* ray, double* tlw)
{
  if (!b) return PTZ_EINVAL;
  PTZ_DEVICE_GUARD(b->device);
  // The current half of every scene's double-buffered state is gathered ON THE DEVICE, in the caller's order (the library
  // numbers a scene's rays by track length, ray_perm), and comes back in one copy per array: round 2 issued two small
  // synchronous copies per scene (6 ms for 64 rigs, 30 ms for the 1000 scenes of C4).
  const size_t nc = (size_t)b->total_cam * 15, nr = (size_t)b->total_ray * 3, nt = (size_t)b->n_scene * 6;
  void* stage = nullptr;
  if (ptzpool::dev_acquire(b->device, sizeof(double) * (nc + nr + nt), &stage) != hipSuccess) return PTZ_ENOMEM;
  double* s_cam = static_cast<double*>(stage);
  double* s_tlw = s_cam + nc;
  double* s_ray = s_tlw + nt;  // (last: a caller that does not want the rays does not pay for their copy)
  hipLaunchKernelGGL(k_gather_state, dim3(std::max(1, (std::max(b->max_cam * 15, b->max_ray) + 255) / 256), b->n_scene), dim3(256), 0, b->stream, b->d,
                     b->d_ray_perm, s_cam, s_ray, s_tlw);
  // the gathered state comes back in ONE copy into a pinned block (the kernel and the copy are ordered on the batch's stream: one
  // wait), from where the caller's arrays are filled
  const size_t bytes = sizeof(double) * (nc + nt + (ray ? nr : 0));
  void* pin = nullptr;
  hipError_t e = hipSuccess;
  if (bytes <= ((size_t)32 << 20) && ptzpool::pinned_acquire(bytes, &pin) == hipSuccess) {
    e = hipMemcpyAsync(pin, stage, bytes, hipMemcpyDeviceToHost, b->stream);
    if (e == hipSuccess) e = stream_wait(b->stream);
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) {
      const double* p = static_cast<const double*>(pin);
      if (cam) memcpy(cam, p, sizeof(double) * nc);
      if (tlw) memcpy(tlw, p + nc, sizeof(double) * nt);
      if (ray) memcpy(ray, p + nc + nt, sizeof(double) * nr);
    }
    ptzpool::pinned_release(pin);
  }
  else {
    (void)hipGetLastError();
    e = stream_wait(b->stream);
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess && cam) e = copy_on(b->stream, cam, s_cam, sizeof(double) * nc, hipMemcpyDeviceToHost);
    if (e == hipSuccess && ray) e = copy_on(b->stream, ray, s_ray, sizeof(double) * nr, hipMemcpyDeviceToHost);
    if (e == hipSuccess && tlw) e = copy_on(b->stream, tlw, s_tlw, sizeof(double) * nt, hipMemcpyDeviceToHost);
  }
  ptzpool::dev_release(b->device, stage);
  if (e != hipSuccess) { (void)hipGetLastError(); return PTZ_ENODEVICE; }
  return PTZ_OK;
}

namespace {
// the anchors of a batch covariance: gauge_cam checked against each problem's cameras (NULL: camera 0 everywhere)
bool ba_cov_gauges(const ptz_ba_batch* b, const int32_t* gauge_cam, std::vector<int>& gauge)
{
  gauge.assign(b->n_scene, 0);
  for (int i = 0; gauge_cam && i < b->n_scene; ++i) {
    if (gauge_cam[i] < 0 || gauge_cam[i] >= b->scenes[i].n_cam) return false;
    gauge[i] = gauge_cam[i];
  }
  return true;
}

// What ptz_ba_cov.hip is given of a batch, for both covariances: the scenes' real extents and state halves (k_ba_cov_pack) on the
// device and on the host, BaCovIn (with_geo: BaGeoIn too) from the batch's resident structure.  Owns the device scene array.
struct BaCovPrep {
  int32_t rc = PTZ_OK;  // PTZ_OK, or why there is nothing to run
  std::vector<BaCovScene> hs;
  BaCovIn in;
  BaGeoIn geo{};
  BaCovPrep(ptz_ba_batch* b, bool with_geo) : device(b->device)
  {
    const Dev& d = b->d;
    if (ptzpool::dev_acquire(device, sizeof(BaCovScene) * b->n_scene, &dsc) != hipSuccess) { rc = PTZ_ENOMEM; return; }
    // before the first solve the state is the one last set (cam0 / ray0 / tlw0); afterwards the current half of every scene
    const bool initial = b->n_solves == 0;
    hipLaunchKernelGGL(k_ba_cov_pack, dim3((b->n_scene + 63) / 64), dim3(64), 0, b->stream, d, initial ? 1 : 0, static_cast<BaCovScene*>(dsc));
    hs.resize(b->n_scene);
    if (copy_on(b->stream, hs.data(), dsc, sizeof(BaCovScene) * b->n_scene, hipMemcpyDeviceToHost) != hipSuccess || hipGetLastError() != hipSuccess) { rc = PTZ_ENODEVICE; return; }
    in.n_scene = b->n_scene; in.type = b->type; in.device = device;
    in.scene = static_cast<const BaCovScene*>(dsc);
    in.obs_uv = d.obs_uv; in.obs_cam = d.obs_cam; in.ray_ptr = d.ray_ptr; in.cam_ptr = d.cam_ptr; in.cam_obs = d.cam_obs;
    in.pair_cj = d.pair_cj; in.pair_ptr = d.pair_ptr; in.cam_pair = d.cam_pair; in.ent = d.ent; in.ray_w = d.ray_w;
    in.cam_x = initial ? b->cam0 : d.cam_x; in.ray_x = initial ? b->ray0 : d.ray_x;
    in.cam_stride = initial ? 0 : d.cam_stride; in.ray_stride = initial ? 0 : d.ray_stride;
    if (!with_geo) return;
    geo.o3_uv = d.o3_uv; geo.o3_xyz = d.o3_xyz; geo.o3_cam = d.o3_cam;
    geo.tlw_x = initial ? b->tlw0 : d.tlw_x; geo.tlw_stride = initial ? 0 : d.tlw_stride;
  }
  ~BaCovPrep() { ptzpool::dev_release(device, dsc); }
  BaCovPrep(const BaCovPrep&) = delete;

 private:
  int device;
  void* dsc = nullptr;
};
}  // namespace

int32_t ptz_ba_cov_dim(int32_t factor_type)
{
  const int nf = ba_cov_dim(factor_type);
  return nf < 0 ? PTZ_EUNSUPPORTED : nf;
}

int32_t ptz_ba_batch_covariance(ptz_ba_batch* b, const int32_t* gauge_cam, double pixel_sigma, double* cov, double* sigma0, int32_t* status,
                                double* device_ms)
{
  if (!b || !b->has_state || !cov || !sigma0 || !status) return PTZ_EINVAL;
  if (!(pixel_sigma >= 0.0) || !std::isfinite(pixel_sigma)) return PTZ_EINVAL;
  // PTZRayDistDisp, 2D-3D annotations and shared intrinsics couple the cameras through blocks this reduced system does not carry
  if (ba_cov_dim(b->type) < 0 || b->has3d || b->d.shared) return PTZ_EUNSUPPORTED;
  std::vector<int> gauge;
  if (!ba_cov_gauges(b, gauge_cam, gauge)) return PTZ_EINVAL;
  clear_stale_error(__func__);
  PTZ_DEVICE_GUARD(b->device);
  BaCovPrep prep(b, false);
  if (prep.rc) return prep.rc;
  return ba_cov_run(prep.in, prep.hs.data(), gauge.data(), pixel_sigma, b->stream, cov, sigma0, status, device_ms);
}

int32_t ptz_ba_covariance(const ptz_ba_problem* p, const double* cam, const double* ray, int32_t gauge_cam, double pixel_sigma,
                          const ptz_lm_options* opt, double* cov, double* sigma0, int32_t* status)
{
  if (!p || !cam || !ray || !cov || !sigma0 || !status) return PTZ_EINVAL;
  if (!(pixel_sigma >= 0.0) || !std::isfinite(pixel_sigma)) return PTZ_EINVAL;
  if (ba_cov_dim(p->factor_type) < 0 || p->n_obs3d > 0 || p->ic_of_cam) return PTZ_EUNSUPPORTED;
  if (gauge_cam < 0 || gauge_cam >= p->n_cam) return PTZ_EINVAL;
  ptz_ba_batch* b = nullptr;
  PTZ_TRY(ptz_ba_batch_create(1, p, opt, &b));
  BatchOwner owner(b);
  PTZ_TRY(ptz_ba_batch_set_state(b, cam, ray, nullptr));
  return ptz_ba_batch_covariance(b, &gauge_cam, pixel_sigma, cov, sigma0, status, nullptr);
}

int32_t ptz_ba_geo_cov_dim(int32_t factor_type)
{
  const int nf = ba_geo_cov_dim(factor_type);
  return nf < 0 ? PTZ_EUNSUPPORTED : nf;
}

int32_t ptz_ba_batch_covariance_georef(ptz_ba_batch* b, const int32_t* gauge_cam, double pixel_sigma, double annotation_sigma, double* cov,
                                       double* cov_centre, double* sigma0, int32_t* status, double* device_ms)
{
  if (!b || !b->has_state || !cov || !cov_centre || !sigma0 || !status) return PTZ_EINVAL;
  if (!(pixel_sigma >= 0.0) || !std::isfinite(pixel_sigma) || !(annotation_sigma >= 0.0) || !std::isfinite(annotation_sigma)) return PTZ_EINVAL;
  // PTZRayFxfyDist, PTZRayDistDisp and shared intrinsics are not what the georeferencing stage solves
  if (ba_geo_cov_dim(b->type) < 0 || b->d.shared) return PTZ_EUNSUPPORTED;
  std::vector<int> gauge;
  if (!ba_cov_gauges(b, gauge_cam, gauge)) return PTZ_EINVAL;
  if (!b->has3d) {  // no problem of the batch carries an annotation: every one is short of constraints, nothing to compute
    for (int i = 0; i < b->n_scene; ++i) status[i] = kBaCovDof;
    if (device_ms) *device_ms = 0.0;
    return PTZ_OK;
  }
  clear_stale_error(__func__);
  PTZ_DEVICE_GUARD(b->device);
  BaCovPrep prep(b, true);
  if (prep.rc) return prep.rc;
  return ba_geo_cov_run(prep.in, prep.geo, prep.hs.data(), gauge.data(), pixel_sigma, annotation_sigma, b->stream, cov, cov_centre, sigma0, status,
                        device_ms);
}

int32_t ptz_ba_covariance_georef(const ptz_ba_problem* p, const double* cam, const double* ray, const double* tlw, int32_t gauge_cam,
                                 double pixel_sigma, double annotation_sigma, const ptz_lm_options* opt, double* cov, double* cov_centre,
                                 double* sigma0, int32_t* status)
{
  if (!p || !cam || !ray || !tlw || !cov || !cov_centre || !sigma0 || !status) return PTZ_EINVAL;
  if (!(pixel_sigma >= 0.0) || !std::isfinite(pixel_sigma) || !(annotation_sigma >= 0.0) || !std::isfinite(annotation_sigma)) return PTZ_EINVAL;
  if (ba_geo_cov_dim(p->factor_type) < 0 || p->ic_of_cam) return PTZ_EUNSUPPORTED;
  if (gauge_cam < 0 || gauge_cam >= p->n_cam) return PTZ_EINVAL;
  ptz_ba_batch* b = nullptr;
  PTZ_TRY(ptz_ba_batch_create(1, p, opt, &b));
  BatchOwner owner(b);
  PTZ_TRY(ptz_ba_batch_set_state(b, cam, ray, tlw));
  return ptz_ba_batch_covariance_georef(b, &gauge_cam, pixel_sigma, annotation_sigma, cov, cov_centre, sigma0, status, nullptr);
}

namespace {
// the residual report / the selection on it at the batch's current state: the checks the two entry points share, then ptz_ba_resid.hip
int32_t ba_resid_call(ptz_ba_batch* b, const BaResidOut& out, double* device_ms)
{
  // PTZRayDistDisp carries a displacement block, shared intrinsics one state per group: not what these kernels read
  if (ba_cov_dim(b->type) < 0 || b->d.shared) return PTZ_EUNSUPPORTED;
  clear_stale_error(__func__);
  PTZ_DEVICE_GUARD(b->device);
  BaCovPrep prep(b, b->has3d != 0);
  if (prep.rc) return prep.rc;
  return ba_resid_run(prep.in, prep.geo, prep.hs.data(), b->d_ray_perm, b->stream, out, device_ms);
}
}  // namespace

int32_t ptz_ba_batch_residuals(ptz_ba_batch* b, double* err_px, double* ray_max, int32_t* ray_worst, double* view_rms, double* view_max,
                               int32_t* view_count, double* rms, double* median, double* err3d_px, double* rms3d, double* device_ms)
{
  if (!b || !b->has_state) return PTZ_EINVAL;
  if (!err_px && !ray_max && !ray_worst && !view_rms && !view_max && !view_count && !rms && !median && !err3d_px && !rms3d) return PTZ_EINVAL;
  BaResidOut out;
  out.err_px = err_px; out.ray_max = ray_max; out.ray_worst = ray_worst; out.view_rms = view_rms; out.view_max = view_max;
  out.view_count = view_count; out.rms = rms; out.median = median; out.err3d_px = err3d_px; out.rms3d = rms3d;
  return ba_resid_call(b, out, device_ms);
}

int32_t ptz_ba_batch_trim_select(ptz_ba_batch* b, double trim_px, double k_sigma, uint8_t* reject, double* threshold, int32_t* n_reject,
                                 double* device_ms)
{
  if (!b || !b->has_state) return PTZ_EINVAL;
  if (!reject && !threshold && !n_reject) return PTZ_EINVAL;
  BaResidOut out;
  out.select = true;
  out.rule = TrimRule{trim_px, k_sigma, 2};
  if (!trim_rule_valid(out.rule)) return PTZ_EINVAL;
  out.reject = reject; out.threshold = threshold; out.n_reject = n_reject;
  return ba_resid_call(b, out, device_ms);
}

int32_t ptz_ba_batch_set_disp(ptz_ba_batch* b, const double* disp)
{
  if (!b || !disp) return PTZ_EINVAL;
  if (b->type != PTZ_BA_PTZRayDistDisp) return PTZ_EUNSUPPORTED;
  PTZ_DEVICE_GUARD(b->device);
  std::vector<double> v((size_t)3 * b->total_cam);  // every camera carries a copy of its scene's block
  for (const SceneDev& sd : b->scenes)
    for (int c = 0; c < sd.n_cam; ++c)
      for (int k = 0; k < 3; ++k) v[3 * ((size_t)sd.cam_off + c) + k] = disp[3 * (size_t)sd.idx + k];
  PTZ_HIP_TRY(copy_on(b->stream, b->dsp0, v.data(), sizeof(double) * v.size(), hipMemcpyHostToDevice));
  return PTZ_OK;
}

int32_t ptz_ba_batch_get_disp(ptz_ba_batch* b, double* disp)
{
  if (!b || !disp) return PTZ_EINVAL;
  if (b->type != PTZ_BA_PTZRayDistDisp) return PTZ_EUNSUPPORTED;
  PTZ_DEVICE_GUARD(b->device);
  std::vector<LmState> h(b->n_scene);
  PTZ_HIP_TRY(copy_on(b->stream, h.data(), b->d.lm, sizeof(LmState) * b->n_scene, hipMemcpyDeviceToHost));
  for (int i = 0; i < b->n_scene; ++i)  // camera 0's copy (all copies of a scene are equal)
    PTZ_HIP_TRY(copy_on(b->stream, disp + 3 * (size_t)i, b->d.dsp_x + h[i].cur * b->d.dsp_stride + 3 * (size_t)b->scenes[i].cam_off,
                          sizeof(double) * 3, hipMemcpyDeviceToHost));
  return PTZ_OK;
}

int32_t ptz_ba_batch_last_solve_ms(const ptz_ba_batch* b, double* ms)
{
  if (!b || !ms) return PTZ_EINVAL;
  *ms = b->last_ms;
  return PTZ_OK;
}

int32_t ptz_ba_batch_set_profiling(ptz_ba_batch* b, int32_t enable)
{
  if (!b) return PTZ_EINVAL;
  b->profiling = enable != 0;
  for (int i = 0; i < PTZ_PROF_SLOTS; ++i) { b->prof_ms[i] = 0; b->prof_n[i] = 0; }
  return PTZ_OK;
}

int32_t ptz_ba_batch_get_profile(const ptz_ba_batch* b, double* ms_per_slot, int64_t* launches_per_slot, const char** slot_names)
{
  if (!b) return PTZ_EINVAL;
  for (int i = 0; i < PTZ_PROF_SLOTS; ++i) {
    if (ms_per_slot) ms_per_slot[i] = b->prof_ms[i];
    if (launches_per_slot) launches_per_slot[i] = b->prof_n[i];
    if (slot_names) slot_names[i] = kSlotNames[i];
  }
  return PTZ_OK;
}

int32_t ptz_ba_batch_pix2ray(ptz_ba_batch* b)
{
  if (!b || !b->has_state) return PTZ_EINVAL;
  clear_stale_error(__func__);
  PTZ_DEVICE_GUARD(b->device);
  hipLaunchKernelGGL(k_pix2ray, dim3(b->shapes[0].max_chunk, b->n_scene), dim3(b->shapes[0].ray_block), 0, b->stream, b->d, b->cam0, b->ray0);
  PTZ_HIP_TRY(stream_wait(b->stream));
  PTZ_HIP_TRY(hipGetLastError());
  return PTZ_OK;
}

int32_t ptz_ba_batch_linearize(ptz_ba_batch* b, int32_t index, double* cost, double* g_c, double* U, double* g_r, double* V, double* W)
{
  clear_stale_error(__func__);
  if (!b || !b->has_state || index < 0 || index >= b->n_scene) return PTZ_EINVAL;
  PTZ_DEVICE_GUARD(b->device);
  if (int32_t rcp = ensure_host_ray_perm(b)) return rcp;
  if (W && !b->d.W) {  // the rows exist only for this call's callers (the solver does not materialise them)
    const bool disp = b->type == PTZ_BA_PTZRayDistDisp;
    const int rcw = b->alloc(&b->d.W, (size_t)b->total_obs * (disp ? 24 : b->type == PTZ_BA_PTZRayFxfyDist ? 18 : 16));
    if (rcw) return rcw;
  }
  const Dev& d = b->d;
  const int NC = b->nc;
  hipStream_t st = b->stream;
  PTZ_HIP_TRY(hipMemcpyAsync(d.cam_x, b->cam0, sizeof(double) * 15 * b->total_cam, hipMemcpyDeviceToDevice, st));
  PTZ_HIP_TRY(hipMemcpyAsync(d.ray_x, b->ray0, sizeof(double) * 3 * b->total_ray, hipMemcpyDeviceToDevice, st));
  hipLaunchKernelGGL(k_reset, dim3((b->n_scene + 63) / 64), dim3(64), 0, st, d);
  hipLaunchKernelGGL(k_fill, dim3(((size_t)b->total_cam * NC + 255) / 256), dim3(256), 0, st, d.scale_c, (size_t)b->total_cam * NC, 1.0);
  hipLaunchKernelGGL(k_fill, dim3(((size_t)b->total_ray * 3 + 255) / 256), dim3(256), 0, st, d.scale_r, (size_t)b->total_ray * 3, 1.0);
  PTZ_HIP_TRY(hipMemcpyAsync(d.tlw_x, b->tlw0, sizeof(double) * 6 * b->n_scene, hipMemcpyDeviceToDevice, st));
  PTZ_HIP_TRY(hipMemcpyAsync(d.tlw_x + d.tlw_stride, b->tlw0, sizeof(double) * 6 * b->n_scene, hipMemcpyDeviceToDevice, st));
  hipLaunchKernelGGL(k_fill, dim3((6 * b->n_scene + 255) / 256), dim3(256), 0, st, d.scale_t, (size_t)6 * b->n_scene, 1.0);
  if (d.dsp_x) PTZ_HIP_TRY(hipMemcpyAsync(d.dsp_x, b->dsp0, sizeof(double) * d.dsp_stride, hipMemcpyDeviceToDevice, st));
  switch (b->type + 4 * b->has3d) {  // Dims<TYPE>
    case 0: enqueue_linearize<0>(b); break;
    case 1: enqueue_linearize<1>(b); break;
    case 2: enqueue_linearize<2>(b); break;
    case 3: enqueue_linearize<3>(b); break;
    case 4: enqueue_linearize<4>(b); break;
    case 5: enqueue_linearize<5>(b); break;
    case 6: enqueue_linearize<6>(b); break;
    default: enqueue_linearize<7>(b); break;
  }
  PTZ_HIP_TRY(stream_wait(st));
  PTZ_HIP_TRY(hipGetLastError());
  const SceneDev& s = b->scenes[index];
  if (cost) {
    std::vector<double> c(s.n_cam);
    PTZ_HIP_TRY(copy_on(b->stream, c.data(), d.costc + s.cam_off, sizeof(double) * s.n_cam, hipMemcpyDeviceToHost));
    double t = 0;
    for (double v : c) t += v;
    *cost = t;
  }
  if (g_c) PTZ_HIP_TRY(copy_on(b->stream, g_c, d.gc + (size_t)s.cam_off * NC, sizeof(double) * NC * s.n_cam, hipMemcpyDeviceToHost));
  if (U) PTZ_HIP_TRY(copy_on(b->stream, U, d.U + (size_t)s.cam_off * NC * NC, sizeof(double) * NC * NC * s.n_cam, hipMemcpyDeviceToHost));
  const int* perm = b->ray_perm.data() + s.ray_off;  // internal ray j -> the caller's ray index
  if (g_r) {
    std::vector<double> g3((size_t)s.n_ray * 3);
    PTZ_HIP_TRY(copy_on(b->stream, g3.data(), d.gr + (size_t)s.ray_off * 3, sizeof(double) * 3 * s.n_ray, hipMemcpyDeviceToHost));
    for (int j = 0; j < s.n_ray; ++j)
      for (int k = 0; k < 3; ++k) g_r[(size_t)perm[j] * 3 + k] = g3[(size_t)j * 3 + k];
  }
  if (V) {
    std::vector<double> v6((size_t)s.n_ray * 6);
    PTZ_HIP_TRY(copy_on(b->stream, v6.data(), d.V + (size_t)s.ray_off * 6, sizeof(double) * 6 * s.n_ray, hipMemcpyDeviceToHost));
    for (int j = 0; j < s.n_ray; ++j) {
      const double* p = &v6[(size_t)j * 6];
      double* q = V + (size_t)perm[j] * 9;
      q[0] = p[0]; q[1] = p[1]; q[2] = p[3]; q[3] = p[1]; q[4] = p[2]; q[5] = p[4]; q[6] = p[3]; q[7] = p[4]; q[8] = p[5];
    }
  }
  if (W) {  // rows are stored camera-major; return them in observation order
    const int NW = b->type == PTZ_BA_PTZRayFxfyDist ? 6 : NC - b->has3d;  // W carries the 2D-2D columns only (PTZRayDistDisp: 8)
    const int ws = (NW * 3 + 1) & ~1;        // Dims<TYPE>::WS
    std::vector<double> rows((size_t)s.n_obs * ws);
    std::vector<int> wp(s.n_obs);
    PTZ_HIP_TRY(copy_on(b->stream, rows.data(), d.W + (size_t)s.obs_off * ws, sizeof(double) * ws * s.n_obs, hipMemcpyDeviceToHost));
    PTZ_HIP_TRY(copy_on(b->stream, wp.data(), d.wpos + s.obs_off, sizeof(int) * s.n_obs, hipMemcpyDeviceToHost));
    // internal observation order is (internal ray, order inside the track); the caller's is (caller's ray, same inner order)
    std::vector<int> rp(s.n_ray + 1);
    PTZ_HIP_TRY(copy_on(b->stream, rp.data(), d.ray_ptr + s.ray_off + s.idx, sizeof(int) * (s.n_ray + 1), hipMemcpyDeviceToHost));
    std::vector<int> ext_first(s.n_ray + 1, 0);
    for (int j = 0; j < s.n_ray; ++j) ext_first[perm[j] + 1] = rp[j + 1] - rp[j];
    for (int r = 0; r < s.n_ray; ++r) ext_first[r + 1] += ext_first[r];
    for (int j = 0; j < s.n_ray; ++j)
      for (int a = rp[j]; a < rp[j + 1]; ++a) {
        const int a_int = a - s.obs_off, a_ext = ext_first[perm[j]] + (a - rp[j]);
        memcpy(W + (size_t)a_ext * NW * 3, &rows[(size_t)(wp[a_int] - s.obs_off) * ws], sizeof(double) * NW * 3);
      }
  }
  return PTZ_OK;
}

int32_t ptz_rig_create(int32_t n_img, int32_t n_track, const int64_t* trk_ptr, const int32_t* trk_img, const float* trk_uv, int32_t device_id,
                       ptz_rig** out)
{
  if (n_img <= 0 || n_track <= 0 || !trk_ptr || !trk_img || !trk_uv || !out) return PTZ_EINVAL;
  *out = nullptr;
  const int64_t nv = trk_ptr[n_track];
  if (trk_ptr[0] != 0 || nv <= 0 || nv > 0x7fffffff) return PTZ_EINVAL;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device_id) return PTZ_ENODEVICE;
  ptz_rig* r = new ptz_rig();
  r->device = device_id; r->n_img = n_img; r->n_track = n_track; r->n_view = nv;
  r->img_obs.assign(n_img, 0); r->img_ent.assign(n_img, 0);
  std::vector<int> ptr32(n_track + 1);
  for (int t = 0; t <= n_track; ++t) ptr32[t] = (int)trk_ptr[t];
  for (int t = 0; t < n_track; ++t) {
    const int64_t L = trk_ptr[t + 1] - trk_ptr[t];
    if (L <= 0) { delete r; return PTZ_EINVAL; }
    r->ent_bound += L * (L - 1) / 2;
    r->max_track_len = (int)std::max<int64_t>(r->max_track_len, L);
    for (int64_t e = trk_ptr[t]; e < trk_ptr[t + 1]; ++e) {
      const int im = trk_img[e];
      if (im < 0 || im >= n_img || (e > trk_ptr[t] && im <= trk_img[e - 1])) { delete r; return PTZ_EINVAL; }  // images ascend inside a track
      ++r->img_obs[im];
      r->img_ent[im] += (int)(e - trk_ptr[t]);  // pairs in which this view is the higher camera
    }
  }
  if (r->ent_bound > 0x7fffffff) { delete r; return PTZ_ELIMIT; }
  PTZ_DEVICE_GUARD(device_id);
  hipStream_t st = nullptr;
  if (ptzpool::stream_acquire(device_id, &st) != hipSuccess) { delete r; return PTZ_ENODEVICE; }
  auto up = [&](const void* src, size_t bytes, const void** dst) -> bool {
    void* q = nullptr;
    if (ptzpool::dev_acquire(device_id, bytes, &q) != hipSuccess) return false;
    r->allocs.push_back(q);
    *dst = q;
    return copy_on(st, q, src, bytes, hipMemcpyHostToDevice) == hipSuccess;
  };
  const bool ok = up(ptr32.data(), sizeof(int) * ptr32.size(), (const void**)&r->d_trk_ptr) && up(trk_img, sizeof(int) * (size_t)nv, (const void**)&r->d_trk_img) &&
                  up(trk_uv, sizeof(float) * 2 * (size_t)nv, (const void**)&r->d_trk_uv);
  ptzpool::stream_release(device_id, st);
  if (!ok) { ptz_rig_destroy(r); return PTZ_ENODEVICE; }
  *out = r;
  return PTZ_OK;
}

void ptz_rig_destroy(ptz_rig* r)
{
  if (!r) return;
  DeviceGuard guard(r->device);
  for (void* p : r->allocs) ptzpool::dev_release(r->device, p);
  delete r;
}

int32_t ptz_ba_batch_set_state_pix2ray(ptz_ba_batch* b, const double* cam, const double* rkinv)
{
  if (!b || !cam || !rkinv) return PTZ_EINVAL;
  PTZ_DEVICE_GUARD(b->device);
  clear_stale_error(__func__);
  // cameras and their R^-1 K^-1 in one pinned block, two copies, the ray kernel behind them, one wait
  const size_t nc = (size_t)15 * b->total_cam, nk = (size_t)9 * b->total_cam;
  void* pin = nullptr;
  std::vector<double> heap;
  double* stg = nullptr;
  if (ptzpool::pinned_acquire(sizeof(double) * (nc + nk), &pin) == hipSuccess) stg = static_cast<double*>(pin);
  else { (void)hipGetLastError(); heap.resize(nc + nk); stg = heap.data(); }
  memcpy(stg, cam, sizeof(double) * nc);
  memcpy(stg + nc, rkinv, sizeof(double) * nk);
  // (no wait: the solve that follows runs on the same stream; the staging block lives until that solve's wait, the R^-1 K^-1 block
  //  until the batch goes)
  if (!b->rkinv_dev && b->alloc(&b->rkinv_dev, nk) != PTZ_OK) { if (pin) ptzpool::pinned_release(pin); return PTZ_ENOMEM; }
  double* dk = b->rkinv_dev;  // (one block per batch, reused by later calls: they are ordered on the batch's stream)
  hipError_t e = hipMemcpyAsync(b->cam0, stg, sizeof(double) * nc, hipMemcpyHostToDevice, b->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(dk, stg + nc, sizeof(double) * nk, hipMemcpyHostToDevice, b->stream);
  if (e == hipSuccess) e = hipMemsetAsync(b->tlw0, 0, sizeof(double) * 6 * b->n_scene, b->stream);
  if (e == hipSuccess)
    hipLaunchKernelGGL(k_view_pix2ray, dim3((b->max_ray + 255) / 256, b->n_scene), dim3(256), 0, b->stream, b->d, (const double*)b->cam0, (const double*)dk, b->ray0);
  if (e == hipSuccess && pin) b->staged_pinned.push_back(pin);  // (in flight)
  else { (void)stream_wait(b->stream); if (pin) ptzpool::pinned_release(pin); }  // pageable staging or a refused copy: nothing may still read it
  if (e == hipSuccess) e = hipGetLastError();
  PTZ_HIP_TRY(e);
  b->has_state = true;
  return PTZ_OK;
}

int32_t ptz_debug_batch_initial_rays(ptz_ba_batch* b, double* ray)
{
  if (!b || !ray || !b->has_state) return PTZ_EINVAL;
  PTZ_DEVICE_GUARD(b->device);
  if (int32_t rcp = ensure_host_ray_perm(b)) return rcp;
  std::vector<double> r((size_t)3 * b->total_ray);
  if (copy_on(b->stream, r.data(), b->ray0, sizeof(double) * r.size(), hipMemcpyDeviceToHost) != hipSuccess) return PTZ_ENODEVICE;
  for (const SceneDev& sd : b->scenes)
    for (int j = 0; j < sd.n_ray; ++j)
      for (int k = 0; k < 3; ++k) ray[3 * ((size_t)sd.ray_off + b->ray_perm[sd.ray_off + j]) + k] = r[3 * ((size_t)sd.ray_off + j) + k];
  return PTZ_OK;
}

int32_t ptz_debug_batch_structure_hash(ptz_ba_batch* b, uint64_t* hash)
{
  if (!b || !hash) return PTZ_EINVAL;
  PTZ_DEVICE_GUARD(b->device);
  const Dev& d = b->d;
  uint64_t h = FNV_BASIS;
  auto mix = [&](const void* ptr, size_t bytes) { fnv_mix(h, ptr, bytes); };
  std::vector<unsigned char> buf;
  auto fetch = [&](const void* dev, size_t bytes) -> const unsigned char* {
    buf.resize(bytes + 8);
    if (bytes && copy_on(b->stream, buf.data(), dev, bytes, hipMemcpyDeviceToHost) != hipSuccess) return nullptr;
    return buf.data();
  };
  // every scene's arrays over their real extents, positions made scene-relative (a batch built from views keeps gaps between scenes)
  std::vector<SceneDev> sc(b->n_scene);
  if (copy_on(b->stream, sc.data(), d.scene, sizeof(SceneDev) * b->n_scene, hipMemcpyDeviceToHost) != hipSuccess) return PTZ_ENODEVICE;
  for (int i = 0; i < b->n_scene; ++i) {
    const SceneDev& s = sc[i];
    const int counts[6] = {s.n_cam, s.n_ray, s.n_obs, s.n_pair, s.n_wave, s.n};
    mix(counts, sizeof(counts));
    auto plain = [&](const void* base, size_t elem, size_t first, size_t count) { const unsigned char* p = fetch((const char*)base + elem * first, elem * count); if (p) mix(p, elem * count); return p != nullptr; };
    auto rel = [&](const int* base, size_t first, size_t count, int minus) {
      const unsigned char* p = fetch(base + first, sizeof(int) * count);
      if (!p) return false;
      std::vector<int> v(count);
      memcpy(v.data(), p, sizeof(int) * count);
      for (int& x : v) x -= minus;
      mix(v.data(), sizeof(int) * count);
      return true;
    };
    bool ok = plain(d.obs_uv, sizeof(float2), s.obs_off, s.n_obs) && plain(d.obs_cam, 4, s.obs_off, s.n_obs) && plain(d.obs_ray, 4, s.obs_off, s.n_obs);
    ok = ok && rel(d.ray_ptr, (size_t)s.ray_off + s.idx, (size_t)s.n_ray + 1, s.obs_off) && rel(d.cam_ptr, (size_t)s.cam_off + s.idx, (size_t)s.n_cam + 1, s.obs_off);
    ok = ok && rel(d.cam_obs, s.obs_off, s.n_obs, s.obs_off) && rel(d.wpos, s.obs_off, s.n_obs, s.obs_off) && rel(d.cam_ray, s.obs_off, s.n_obs, s.ray_off);
    ok = ok && plain(d.cam_uv, sizeof(float2), s.obs_off, s.n_obs) && plain(d.ray_w, 8, s.ray_off, s.n_ray) && plain(b->d_ray_perm, 4, s.ray_off, s.n_ray);
    ok = ok && plain(d.pair_ci, 4, s.pair_off, s.n_pair) && plain(d.pair_cj, 4, s.pair_off, s.n_pair) && rel(d.pair_brow, s.pair_off, s.n_pair, s.obs_off);
    ok = ok && rel(d.pair_ptr, (size_t)s.pair_off + s.idx, (size_t)s.n_pair + 1, s.ent_off) && plain(d.pair_run, 4, (size_t)s.pair_off + s.idx, (size_t)s.n_pair + 1);
    ok = ok && plain(d.cam_pair, 4, (size_t)s.cam_off + s.idx, (size_t)s.n_cam + 1) && plain(d.cam_run, 4, (size_t)s.cam_off + s.idx, (size_t)s.n_cam + 1);
    if (!ok) return PTZ_ENODEVICE;
    // entries and runs: extents from the scene's own last offsets
    std::vector<int> last(2);
    if (copy_on(b->stream, &last[0], d.pair_ptr + s.pair_off + s.idx + s.n_pair, 4, hipMemcpyDeviceToHost) != hipSuccess) return PTZ_ENODEVICE;
    if (copy_on(b->stream, &last[1], d.cam_run + s.cam_off + s.idx + s.n_cam, 4, hipMemcpyDeviceToHost) != hipSuccess) return PTZ_ENODEVICE;
    const int n_ent = last[0] - s.ent_off, n_run = last[1];
    if (!plain(d.ent, 4, s.ent_off, (size_t)std::max(n_ent, 0))) return PTZ_ENODEVICE;
    {
      const unsigned char* p = fetch(d.run_rec + s.run_off, sizeof(uint2) * (size_t)std::max(n_run, 0));
      if (!p) return PTZ_ENODEVICE;
      std::vector<uint2> v((size_t)std::max(n_run, 0));
      memcpy(v.data(), p, sizeof(uint2) * v.size());
      for (uint2& x : v) x.x -= (unsigned)s.ent_off;
      mix(v.data(), sizeof(uint2) * v.size());
    }
    const int tail[2] = {n_ent, n_run};
    mix(tail, sizeof(tail));
  }
  *hash = h;
  return PTZ_OK;
}

extern "C++" {
namespace {
template <int TYPE>
int32_t reduced_system_impl(ptz_ba_batch* b, int index, const double* scale_c, const double* scale_r, bool poison, double* S, double* rhs,
                            double* diag_c, int32_t* info)
{
  constexpr int NC = Dims<TYPE>::NC;
  const Dev& d = b->d;
  const SceneDev& s = b->scenes[index];
  const size_t np = d.chol.np, nt = np / CHOL_NB;
  // ---- the solver's prologue (solve_impl) with the caller's Jacobi scales where k_jacobi_scale would write its own
  begin_solve(b);
  hipStream_t s0 = b->stream;
  enqueue_solve_init<TYPE>(b);
  if (scale_c) PTZ_HIP_TRY(copy_on(s0, d.scale_c + (size_t)s.cam_off * NC, scale_c, sizeof(double) * NC * s.n_cam, hipMemcpyHostToDevice));
  if (scale_r) {
    const int* perm = b->ray_perm.data() + s.ray_off;  // internal ray j -> the caller's ray index
    std::vector<double> sr((size_t)s.n_ray * 3);
    for (int j = 0; j < s.n_ray; ++j)
      for (int k = 0; k < 3; ++k) sr[(size_t)j * 3 + k] = scale_r[(size_t)perm[j] * 3 + k];
    PTZ_HIP_TRY(copy_on(s0, d.scale_r + (size_t)s.ray_off * 3, sr.data(), sizeof(double) * sr.size(), hipMemcpyHostToDevice));
  }
  enqueue_linearize<TYPE>(b);
  enqueue_open_first_step<TYPE>(b);
  // ---- the first pass of the scene's group up to the system, in shape 0 at its full extent
  int g = 0;
  while (g + 1 < (int)b->dg.size() && index >= b->group_first[g] + b->group_count[g]) ++g;
  PassShape sh = b->shapes[0];
  sh.slots = b->group_count[g];
  sh.path_slots = sh.slots;
  sh.compact = false;
  const Dev dp = pass_dev<TYPE>(b, b->dg[g], sh);
  double* A_dev = d.chol.A + (size_t)index * np * np;
  if (poison) PTZ_HIP_TRY(hipMemsetAsync(A_dev, 0xFF, sizeof(double) * np * np, s0));
  const SchurLaunch sl = enqueue_reduced_system<TYPE>(b, dp, sh);
  {
    const hipError_t we = stream_wait(s0);
    b->release_staged();
    PTZ_HIP_TRY(we);
    PTZ_HIP_TRY(hipGetLastError());
  }
  b->prof_collect();
  // ---- read back
  LmState lm;
  int active = 0;
  PTZ_HIP_TRY(copy_on(s0, &lm, d.lm + index, sizeof(LmState), hipMemcpyDeviceToHost));
  PTZ_HIP_TRY(copy_on(s0, &active, d.active + index, sizeof(int), hipMemcpyDeviceToHost));
  if (!active) return PTZ_EINVAL;  // the scene ended at iteration zero (gradient tolerance): no step was opened, no system built
  std::vector<double> A(np * np);
  PTZ_HIP_TRY(copy_on(s0, A.data(), A_dev, sizeof(double) * np * np, hipMemcpyDeviceToHost));
  std::vector<unsigned char> mask(nt * nt, 1);  // (PTZ_BA_DENSE_CHOL: no mask, every tile is cleared and read)
  if (d.chol.tmask) PTZ_HIP_TRY(copy_on(s0, mask.data(), d.chol.tmask + (size_t)index * nt * nt, nt * nt, hipMemcpyDeviceToHost));
  std::vector<int> tperm(nt);
  for (size_t t = 0; t < nt; ++t) tperm[t] = (int)t;
  if (d.tperm) PTZ_HIP_TRY(copy_on(s0, tperm.data(), d.tperm + (size_t)index * nt, sizeof(int) * nt, hipMemcpyDeviceToHost));
  int reordered = 0;
  for (size_t t = 0; t < nt; ++t) reordered |= tperm[t] != (int)t;
  const int n = s.n;
  auto col = [&](int c) { return (size_t)tperm[c / CHOL_NB] * CHOL_NB + c % CHOL_NB; };  // sys_col()
  for (int r = 0; r < n; ++r)
    for (int c = 0; c <= r; ++c) {
      const size_t pr = col(r), pc = col(c), hi = std::max(pr, pc), lo = std::min(pr, pc);
      const double v = mask[(hi / CHOL_NB) * nt + lo / CHOL_NB] ? A[hi * np + lo] : 0.0;
      S[(size_t)r * n + c] = v;
      S[(size_t)c * n + r] = v;
    }
  // the right-hand side is row n of the padded system where it stands (its tile, the first dense one, keeps its place in every
  // order: plan_dissection), its columns follow the order
  for (int c = 0; c < n; ++c) rhs[c] = A[(size_t)n * np + col(c)];
  if (diag_c)
    PTZ_HIP_TRY(copy_on(s0, diag_c, d.diag_c + ((size_t)lm.cur * d.lin_cams + s.cam_off) * NC, sizeof(double) * NC * s.n_cam, hipMemcpyDeviceToHost));
  if (info) {
    info[0] = sl.kernel; info[1] = b->schur_tg ? 1 : 0; info[2] = (int)np; info[3] = (int)nt; info[4] = reordered;
    info[5] = b->max_cam_obs; info[6] = b->max_cam_run; info[7] = sl.threads;
  }
  return PTZ_OK;
}
}  // namespace
}  // extern "C++"

int32_t ptz_debug_batch_reduced_system(ptz_ba_batch* b, int32_t index, const double* scale_c, const double* scale_r, int32_t flags, double* S,
                                       double* rhs, double* diag_c, int32_t* info)
{
  if (!b || !b->has_state || index < 0 || index >= b->n_scene || !S || !rhs) return PTZ_EINVAL;
  if (b->type < PTZ_BA_PTZRay || b->type > PTZ_BA_PTZRayFxfyDist || b->has3d || b->d.shared) return PTZ_EUNSUPPORTED;
  clear_stale_error(__func__);
  PTZ_DEVICE_GUARD(b->device);
  if (int32_t rcp = ensure_host_ray_perm(b)) return rcp;
  const bool poison = (flags & 1) != 0;
  switch (b->type) {
    case 0: return reduced_system_impl<0>(b, index, scale_c, scale_r, poison, S, rhs, diag_c, info);
    case 1: return reduced_system_impl<1>(b, index, scale_c, scale_r, poison, S, rhs, diag_c, info);
    default: return reduced_system_impl<2>(b, index, scale_c, scale_r, poison, S, rhs, diag_c, info);
  }
}

void ptz_trim_cache(void) { ptzpool::trim(); }

// a batch for one solve: create, set the state (and the displacement block), solve, read the result back over the caller's arrays
static int32_t solve_in_place(int32_t n, const ptz_ba_problem* problems, const ptz_lm_options* opt, double* cam, double* ray, double* tlw,
                              double* disp, ptz_lm_summary* summaries)
{
  ptz_ba_batch* b = nullptr;
  PTZ_TRY(ptz_ba_batch_create(n, problems, opt, &b));
  BatchOwner owner(b);
  PTZ_TRY(ptz_ba_batch_set_state(b, cam, ray, tlw));
  if (disp) PTZ_TRY(ptz_ba_batch_set_disp(b, disp));
  PTZ_TRY(ptz_ba_batch_solve(b, summaries));
  PTZ_TRY(ptz_ba_batch_get_state(b, cam, ray, tlw));
  return disp ? ptz_ba_batch_get_disp(b, disp) : PTZ_OK;
}

int32_t ptz_ba_solve(const ptz_ba_problem* p, double* cam, double* ray, double* tlw, const ptz_lm_options* opt, ptz_lm_summary* summary)
{
  if (!p || !cam || !ray) return PTZ_EINVAL;
  const bool dbg = getenv("PTZ_BA_DEBUG_TIMING") != nullptr;
  const double t0 = now_ms();
  ptz_ba_batch* b = nullptr;
  int rc = ptz_ba_batch_create(1, p, opt, &b);
  if (rc) return rc;
  BatchOwner owner(b);
  const double t1 = now_ms();
  rc = ptz_ba_batch_set_state(b, cam, ray, tlw);
  const double t2 = now_ms();
  if (!rc) rc = ptz_ba_batch_solve(b, summary);
  const double t3 = now_ms();
  if (!rc) rc = ptz_ba_batch_get_state(b, cam, ray, tlw);
  const double t4 = now_ms();
  owner.reset();
  if (dbg) fprintf(stderr, "[ptz_ba_solve] n_cam %d n_obs %lld: create %.2f set_state %.2f solve %.2f get_state %.2f destroy %.2f ms\n", p->n_cam,
                   (long long)p->n_obs, t1 - t0, t2 - t1, t3 - t2, t4 - t3, now_ms() - t4);
  return rc;
}

int32_t ptz_ba_solve_disp(const ptz_ba_problem* p, double* cam, double* ray, double* tlw, double* disp, const ptz_lm_options* opt,
                          ptz_lm_summary* summary)
{
  if (!p || !cam || !ray) return PTZ_EINVAL;
  if (p->factor_type != PTZ_BA_PTZRayDistDisp) return PTZ_EUNSUPPORTED;
  return solve_in_place(1, p, opt, cam, ray, tlw, disp, summary);
}

// Many scenes over several devices of one node, from one process: scenes are dealt longest-first to the least loaded device
// (they never interact -- run_ptzba_synthetic.sh:4-13 runs them as separate processes), every device gets one host thread
// that creates, solves and reads back its own batch, and the results are scattered back into the caller's arrays.  No
// collective: there is nothing to exchange.
int32_t ptz_ba_solve_sharded(int32_t n, const ptz_ba_problem* problems, double* cam, double* ray, double* tlw,
                             const int32_t* device_ids, int32_t n_devices, const ptz_lm_options* opt, ptz_lm_summary* summaries)
{
  if (n <= 0 || !problems || !cam || !ray || !device_ids || n_devices <= 0) return PTZ_EINVAL;
  ptz_lm_options base;
  if (opt) base = *opt; else ptz_lm_options_default(&base);
  std::vector<size_t> cam_off(n + 1, 0), ray_off(n + 1, 0);
  for (int i = 0; i < n; ++i) {
    if (problems[i].n_cam <= 0 || problems[i].n_ray <= 0) return PTZ_EINVAL;
    cam_off[i + 1] = cam_off[i] + (size_t)problems[i].n_cam;
    ray_off[i + 1] = ray_off[i] + (size_t)problems[i].n_ray;
  }
  // longest-first greedy assignment by observation count
  std::vector<int> order(n);
  for (int i = 0; i < n; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int bq) { return problems[a].n_obs > problems[bq].n_obs; });
  std::vector<std::vector<int>> shard(n_devices);
  std::vector<int64_t> load(n_devices, 0);
  for (int i : order) {
    int best = 0;
    for (int dv = 1; dv < n_devices; ++dv) if (load[dv] < load[best]) best = dv;
    shard[best].push_back(i);
    load[best] += problems[i].n_obs;
  }
  std::vector<int> rcs(n_devices, PTZ_OK);
  auto run = [&](int dv) {
    std::vector<int>& ids = shard[dv];
    if (ids.empty()) return;
    std::sort(ids.begin(), ids.end());  // problem order inside the shard
    std::vector<ptz_ba_problem> probs;
    std::vector<double> c, r, t;
    for (int i : ids) {
      probs.push_back(problems[i]);
      c.insert(c.end(), cam + 15 * cam_off[i], cam + 15 * cam_off[i + 1]);
      r.insert(r.end(), ray + 3 * ray_off[i], ray + 3 * ray_off[i + 1]);
      if (tlw) t.insert(t.end(), tlw + 6 * (size_t)i, tlw + 6 * (size_t)(i + 1));
    }
    ptz_lm_options o = base;
    o.device_id = device_ids[dv];
    std::vector<ptz_lm_summary> summ(ids.size());
    rcs[dv] = solve_in_place((int32_t)ids.size(), probs.data(), &o, c.data(), r.data(), tlw ? t.data() : nullptr, nullptr, summ.data());
    if (rcs[dv]) return;
    size_t co = 0, ro = 0;
    for (size_t k = 0; k < ids.size(); ++k) {
      const int i = ids[k];
      const size_t nc = (size_t)problems[i].n_cam, nr = (size_t)problems[i].n_ray;
      memcpy(cam + 15 * cam_off[i], c.data() + 15 * co, sizeof(double) * 15 * nc);
      memcpy(ray + 3 * ray_off[i], r.data() + 3 * ro, sizeof(double) * 3 * nr);
      if (tlw) memcpy(tlw + 6 * (size_t)i, t.data() + 6 * k, sizeof(double) * 6);
      if (summaries) summaries[i] = summ[k];
      co += nc; ro += nr;
    }
  };
  std::vector<std::thread> th;
  for (int dv = 1; dv < n_devices; ++dv) th.emplace_back(run, dv);
  run(0);
  for (auto& x : th) x.join();
  for (int rc : rcs) if (rc) return rc;
  return PTZ_OK;
}

// Diagnostic (not part of the drop-in boundary, used by tools/probes/probe_host_structure.py): the host-side structure stage of
// ptz_ba_batch_create -- build_pairs of every problem on `n_threads` threads, into scratch arrays -- without touching a device.
int32_t ptz_debug_host_structure(int32_t n, const ptz_ba_problem* problems, int32_t n_threads, int32_t reps, double* ms_per_rep, uint64_t* hash_out)
{
  if (n <= 0 || !problems || n_threads <= 0 || reps <= 0 || !ms_per_rep) return PTZ_EINVAL;
  const auto t0 = std::chrono::steady_clock::now();
  for (int rep = 0; rep < reps; ++rep) {
    HostObs a;
    a.set_bases(n, problems);
    a.resize_all(n);
    std::vector<int> perm(a.ray_base[n]);
    std::vector<PairBuild> wave;
    build_scene_wave(problems, 0, n, n_threads, a, perm.data(), wave, /*pairs_on_device=*/false);
    for (int k = 0; k < n; ++k) if (wave[k].err != PTZ_OK) return wave[k].err;
    if (hash_out && rep == 0) {  // FNV-1a over everything the stage produces, in a fixed order
      uint64_t h = FNV_BASIS;
      auto mix = [&](const void* ptr, size_t bytes) { fnv_mix(h, ptr, bytes); };
      const size_t to = a.obs_base[n];
      mix(a.uv.data(), sizeof(float2) * to); mix(a.camuv.data(), sizeof(float2) * to); mix(a.cam.data(), 4 * to); mix(a.ray.data(), 4 * to);
      mix(a.camobs.data(), 4 * to); mix(a.camray.data(), 4 * to); mix(a.wpos.data(), 4 * to);
      mix(a.rayptr.data(), 4 * a.rayptr.size()); mix(a.camptr.data(), 4 * a.camptr.size()); mix(a.campair.data(), 4 * a.campair.size()); mix(a.camrun.data(), 4 * a.camrun.size());
      mix(perm.data(), 4 * perm.size()); mix(a.w.data(), 8 * a.w.size());
      for (int k = 0; k < n; ++k) {
        const PairBuild& pb = wave[k];
        mix(pb.pci.data(), 4 * pb.pci.size()); mix(pb.pcj.data(), 4 * pb.pcj.size()); mix(pb.pptr.data(), 4 * pb.pptr.size()); mix(pb.pbrow.data(), 4 * pb.pbrow.size());
        mix(pb.ent.data(), 4 * pb.ent.size()); mix(pb.runs.data(), 8 * pb.runs.size()); mix(pb.prun.data(), 4 * pb.prun.size());
        const int64_t v[7] = {pb.n_ent, pb.n_pair, pb.max_cam_obs, pb.max_cam_ent, pb.max_cam_pair, pb.max_cam_run, pb.err};
        mix(v, sizeof(v));
      }
      *hash_out = h;
    }
  }
  *ms_per_rep = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / reps;
  return PTZ_OK;
}

}  // extern "C"
