// ptz_relocalizer.hip -- the resident serving loop of the online half: what joins the device entry points.  References stay on the
// device (their descriptor set is the caller's, their cameras and rotation matrices are uploaded once); a run takes a set of query
// images through
//   0. (ptz_relocalizer_run_shortlisted) the vote pass that picks a query's references, read by the host   ptz_desc_shortlist_device
//      (ptz_relocalizer_run_tracked) the overlap lists and pair homographies of the prior cameras            ptz_reloc_prior_pairs_device
//      -- then the guided matcher under those homographies stands IN PLACE of stages 1 and 2, the prior enters the solve's initial
//      camera after stage 3, and stage 4 is forced on (the lone-candidate finding of ptz_reloc_prior.h)
//      (ptz_relocalizer_run_landmarks) nothing: the run's pairs are (map, query q), one per query -- stage 1 matches every query
//      against the landmark map's one image, stage 2 does not exist, and stage 3 is ptz_landmark_assemble_device
//      (ptz_relocalizer_run_landmarks_tracked) the landmark view of the prior cameras                        ptz_landmark_visible
//      -- then the guided matcher over the pairs (view image q, query q) under identity H stands in place of stage 1, its idx_a is
//      lifted from view-local to landmark indices in front of the landmark assembly, the prior enters the solve's initial camera,
//      and stage 4 is forced on, as in the tracked run
//      (ptz_relocalizer_run_landmarks_shortlisted) the vote pass over the map's home set, then the view of    ptz_landmark_shortlist_device
//      the landmarks whose home is on a query's list, both from device arrays                          ptz_landmark_view_from_homes_device
//      -- then the DENSE matcher of stage 1 runs over the pairs (view image q, query q), its idx_a is lifted as in the tracked
//      landmark run, and nothing else differs from the landmark run: no prior, no forced gate
//   1. the matcher over the run's pairs: every (reference, query) pair, or the shortlisted ones             ptz_desc_match_pairs
//   2. optionally the gate on all pairs and the guided pass      ptz_match_gate_run_device, ptz_desc_match_pairs_guided_device
//   3. the assembly                                              ptz_reloc_assemble_device
//   4. optionally the gate on the assembled queries              ptz_match_gate_run_device, or after ptz_relocalizer_set_gate_model(r, 1, ..)
//                                                                ptz_rotfocal_gate_run_device (cam_ref / cam_cur as stage 3 left them)
//   5. the solve or the trimmed solve                            ptz_krt_solve_batch_device, ptz_krt_solve_batch_trimmed_device
//   6. optionally the covariance                                 ptz_krt_covariance_batch_device
// with every array between them on the device.  Nothing here computes: the stages are the library's own entry points, composed as
// run_ptz_reloc and MatchDescriptors compose their host forms, so with max_refs = 1 a query's outputs are the bits of that path.
// The kernels of this file turn the gate's kept offsets into what the host code derives from its mask: a pair's `found` after
// the min_inliers rule, a mask that is zero for a query that does not pass and, in a tracked run, accepted = 0 for such a query.
#include <cmath>
#include <optional>
#include <vector>

#include "ptz_common.h"
#include "ptz_desc_set.h"
#include "ptz_host_batch.h"
#include "ptz_landmark_map.h"

namespace ptz {
namespace {

// found[p] = 1 iff the gate kept matches of pair p (a model and at least max(min_inliers, 4) mask-1 matches), else 0
__global__ void k_reloc_found(int n_pair, const int64_t* __restrict__ gate_ptr, int32_t* __restrict__ found)
{
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p < n_pair) found[p] = gate_ptr[p + 1] > gate_ptr[p] ? 1 : 0;
}

// the mask bytes of a query the gate did not pass are whatever an earlier run left: zero them (one wave per query)
__global__ void k_reloc_universe(int n_query, const int64_t* __restrict__ match_ptr, const int64_t* __restrict__ gate_ptr,
                                 uint8_t* __restrict__ mask)
{
  const int q = blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE;
  if (q >= n_query || gate_ptr[q + 1] > gate_ptr[q]) return;
  for (int64_t i = match_ptr[q] + threadIdx.x % WAVE; i < match_ptr[q + 1]; i += WAVE) mask[i] = 0;
}

// a tracked run: a query the gate kept nothing of is LOST, whatever the solve on no matches answers (an empty query converges where it
// stands): its accepted is 0, the caller's signal to fall back
__global__ void k_reloc_lost(int n_query, const int64_t* __restrict__ gate_ptr, int32_t* __restrict__ accepted)
{
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q < n_query && gate_ptr[q + 1] <= gate_ptr[q]) accepted[q] = 0;
}

// a landmark run over a view (from a prior or from homes): the matcher's idx_a is local to the view image of its pair (= its
// query); the assembly wants landmarks.
// One wave per query; an index outside the view becomes -1, which neither votes nor is kept.
__global__ void k_reloc_lift(int n_query, const int64_t* __restrict__ match_ptr, const int32_t* __restrict__ idx_a,
                             const int64_t* __restrict__ vis_ptr, const int32_t* __restrict__ vis_lm, int32_t* __restrict__ lifted)
{
  const int q = blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE;
  if (q >= n_query) return;
  const int64_t v0 = vis_ptr[q], nv = vis_ptr[q + 1] - v0;
  for (int64_t i = match_ptr[q] + threadIdx.x % WAVE; i < match_ptr[q + 1]; i += WAVE) {
    const int32_t a = idx_a[i];
    lifted[i] = a >= 0 && a < nv ? vis_lm[v0 + a] : -1;
  }
}

struct Events {  // the stamps around stages 3 .. 6 on the resident stream (the temporaries of stages 0 and 2 bring their own)
  int dev;
  hipEvent_t e[5] = {};
  explicit Events(int d) : dev(d) {}
  ~Events() { for (hipEvent_t x : e) ptzpool::event_release(dev, true, x); }
  hipError_t make() { for (hipEvent_t& x : e) { const hipError_t r = ptzpool::event_acquire(dev, true, &x); if (r != hipSuccess) return r; } return hipSuccess; }
  double ms(int a, int b) const { float t = 0; (void)hipEventElapsedTime(&t, e[a], e[b]); return t; }
};

}  // namespace
}  // namespace ptz

struct ptz_relocalizer {
  int device = 0;
  int32_t n_ref = 0;
  const ptz_desc_set* refs = nullptr;
  char* d_const = nullptr;  // [ref_cams | ref_R]
  double *d_cams = nullptr, *d_R = nullptr;
  hipStream_t st = nullptr;
  ptz_match_gate* gate = nullptr;  // grows with the runs: pairs, matches, matches of one pair
  int32_t gate_pairs = 0, gate_pm = 0;
  int64_t gate_matches = 0;
  ptz_rotfocal_gate* rf_gate = nullptr;  // the rotation-and-focal gate of stage 4 (gate_model = 1): grows likewise
  int32_t rf_pairs = 0;
  int64_t rf_matches = 0;
  int32_t gate_model = 0, gate_iters = 128;  // ptz_relocalizer_set_gate_model: the model of stage 4 in the runs that follow
  ptz_desc_matches* table = nullptr;  // the last run's match table of its pairs (the guided one, if that pass ran)
  ptz_landmark_view* view = nullptr;  // the last run's landmark view, if it was a tracked or a shortlisted landmark run
  std::vector<int32_t> pair_ref;      // the last run's pair list: the reference of each pair,
  std::vector<int64_t> query_ptr;     // and each query's range of it
  // the last run's block: the assembled matches stay until the next run
  char* blk = nullptr;
  int32_t n_query = 0;
  int64_t kept = 0;
  size_t o_optr = 0, o_oa = 0, o_ob = 0, o_osrc = 0, o_model = 0, o_found = 0;
  bool has_models = false;  // the last run gated its assembled queries with gate_model = 1
};

extern "C" void ptz_reloc_options_default(ptz_reloc_options* o)
{
  if (!o) return;
  memset(o, 0, sizeof(*o));
  ptz_desc_options_default(&o->match);
  o->ransac_thresh = 4.0;
  o->min_inliers = 6;
  o->gate_max_pair_matches = 2048;
  ptz_krt_trim_options_default(&o->trim_options);
  o->max_refs = 1;
  o->factor_type = PTZ_KRT_F;
  o->max_reproj_error = 100.0;
  ptz_lm_options_default(&o->lm);
}

extern "C" int32_t ptz_relocalizer_create(const ptz_desc_set* ref_set, const double* ref_cams, int32_t n_ref, int32_t device_id,
                                          ptz_relocalizer** out)
{
  using namespace ptz;
  if (!out) return PTZ_EINVAL;
  *out = nullptr;
  if (!ref_set || !ref_cams || n_ref < 1 || device_id < 0) return PTZ_EINVAL;
  clear_stale_error(__func__);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device_id) return PTZ_ENODEVICE;
  PTZ_DEVICE_GUARD(device_id);
  std::vector<double> R(9 * (size_t)n_ref);
  if (const int32_t rc = ptz_reloc_ref_rotations(n_ref, ref_cams, R.data())) return rc;
  ptz_relocalizer* r = new ptz_relocalizer();
  r->device = device_id; r->n_ref = n_ref; r->refs = ref_set;
  BlockLayout b;
  const size_t o_cams = b.take(sizeof(double) * 15 * n_ref), o_R = b.take(sizeof(double) * 9 * n_ref);
  hipError_t e = ptzpool::dev_acquire(device_id, b.total(), (void**)&r->d_const);
  if (e == hipSuccess) e = ptzpool::stream_acquire(device_id, &r->st);
  if (e == hipSuccess) {
    r->d_cams = (double*)(r->d_const + o_cams); r->d_R = (double*)(r->d_const + o_R);
    e = hipMemcpyAsync(r->d_cams, ref_cams, sizeof(double) * 15 * n_ref, hipMemcpyHostToDevice, r->st);
  }
  if (e == hipSuccess) e = hipMemcpyAsync(r->d_R, R.data(), sizeof(double) * 9 * n_ref, hipMemcpyHostToDevice, r->st);
  if (e == hipSuccess) e = stream_wait(r->st);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    ptz_relocalizer_destroy(r);
    return e == hipErrorOutOfMemory ? PTZ_ENOMEM : PTZ_ENODEVICE;
  }
  *out = r;
  return PTZ_OK;
}

extern "C" void ptz_relocalizer_destroy(ptz_relocalizer* r)
{
  if (!r) return;
  ptz::DeviceGuard guard(r->device);
  if (r->st) { (void)ptz::stream_wait(r->st); ptzpool::stream_release(r->device, r->st); }
  ptz_match_gate_destroy(r->gate);
  ptz_rotfocal_gate_destroy(r->rf_gate);
  ptz_desc_matches_destroy(r->table);
  ptz_landmark_view_destroy(r->view);
  ptzpool::dev_release(r->device, r->blk);
  ptzpool::dev_release(r->device, r->d_const);
  delete r;
}

static int32_t reloc_gate_for(ptz_relocalizer* r, int32_t pairs, int64_t matches, int32_t pm)
{
  if (r->gate && r->gate_pairs >= pairs && r->gate_matches >= matches && r->gate_pm >= pm) return PTZ_OK;
  ptz_match_gate_destroy(r->gate);
  r->gate = nullptr;
  r->gate_pairs = pairs > r->gate_pairs ? pairs : r->gate_pairs;
  r->gate_matches = matches > r->gate_matches ? matches : r->gate_matches;
  r->gate_pm = pm > r->gate_pm ? pm : r->gate_pm;
  return ptz_match_gate_create(r->gate_pairs, r->gate_matches, r->gate_pm, r->device, &r->gate);
}

static int32_t reloc_rf_gate_for(ptz_relocalizer* r, int32_t pairs, int64_t matches)
{
  if (r->rf_gate && r->rf_pairs >= pairs && r->rf_matches >= matches) return PTZ_OK;
  ptz_rotfocal_gate_destroy(r->rf_gate);
  r->rf_gate = nullptr;
  r->rf_pairs = pairs > r->rf_pairs ? pairs : r->rf_pairs;
  r->rf_matches = matches > r->rf_matches ? matches : r->rf_matches;
  return ptz_rotfocal_gate_create(r->rf_pairs, r->rf_matches, r->device, &r->rf_gate);
}

// the prior cameras of a tracked run and what it reports of its stage 0
struct RelocPrior {
  const double* cams;
  ptz_prior_options opt;
  ptz_prior_result* res;
};

// the prior cameras of a tracked landmark run and what it reports of its stage 0
struct RelocLmPrior {
  const double* cams;
  ptz_landmark_prior_options opt;
  ptz_landmark_view_result* res;
};

// the vote options of a shortlisted landmark run and what it reports of its stage 0
struct RelocLmShort {
  ptz_shortlist_options opt;
  ptz_shortlist_result* sl_res;
  ptz_landmark_view_result* res;
};

// all the runs: sl = pr = nullptr is ptz_relocalizer_run (every reference of every query), else stage 0 picks a query's references,
// by votes (sl) or by the overlap with its prior camera (pr); lmap: the landmark run, whose one pair per query is (map, query);
// lp (with lmap): the tracked landmark run, whose pair is (the query's view of the map, query); ls (with lmap): the shortlisted
// landmark run, the same pair with the view of the listed homes
static int32_t reloc_run(const char* who, ptz_relocalizer* r, const ptz_desc_set* query_set, int32_t n_query, const int32_t* query_wh,
                         const ptz_reloc_options* options, const ptz_shortlist_options* sl, ptz_reloc_result* res, ptz_shortlist_result* sl_res,
                         const RelocPrior* pr = nullptr, const ptz_landmark_map* lmap = nullptr, const RelocLmPrior* lp = nullptr,
                         const RelocLmShort* ls = nullptr)
{
  using namespace ptz;
  if (!r || !query_set || n_query < 0 || !res || (n_query > 0 && !query_wh)) return PTZ_EINVAL;
  ptz_reloc_options o;
  if (options) o = *options; else ptz_reloc_options_default(&o);
  if (lmap) o.max_refs = 1;  // one slot: the anchor
  if (lp) o.guided_radius = 0.0;  // (ignored: the radius is lp's)
  if (o.max_refs < 1 || o.min_inliers < 0 || !(o.guided_radius >= 0.0) || !std::isfinite(o.guided_radius) ||
      !(std::isfinite(o.ransac_thresh) && o.ransac_thresh > 0) || o.gate_max_pair_matches < 0 || o.gate_max_pair_matches > 4096 ||
      (o.guided_grid != 0 && o.guided_grid != 1))
    return PTZ_EINVAL;
  for (int q = 0; q < n_query; ++q)
    if (query_wh[2 * q] <= 0 || query_wh[2 * q + 1] <= 0) return PTZ_EINVAL;
  if (o.factor_type < PTZ_KRT_F || o.factor_type > PTZ_KRT_FxfyDist) return PTZ_EUNSUPPORTED;
  if (o.match.device_id != r->device || (o.lm.device_id != 0 && o.lm.device_id != r->device)) return PTZ_EINVAL;
  if (sl && (shortlist_options_check(*sl) || r->refs->n_img != r->n_ref || n_query > query_set->n_img)) return PTZ_EINVAL;
  if (pr && (prior_options_check(pr->opt) || r->refs->n_img != r->n_ref || n_query > query_set->n_img || (n_query > 0 && !pr->cams) ||
             prior_cams_check(n_query, pr->cams)))
    return PTZ_EINVAL;
  if (lmap && (lmap->device != r->device || lmap->n_ref != r->n_ref || !lmap->set || lmap->D != query_set->D || query_set->device != r->device ||
               n_query > query_set->n_img))
    return PTZ_EINVAL;
  if (lp && (!lmap || !(std::isfinite(lp->opt.radius_px) && lp->opt.radius_px > 0) || lp->opt.max_view_bytes < 1 || (n_query > 0 && !lp->cams) ||
             prior_cams_check(n_query, lp->cams)))
    return PTZ_EINVAL;
  if (ls && (!lmap || lp || shortlist_options_check(ls->opt))) return PTZ_EINVAL;
  if (lmap && o.guided_radius > 0.0) return PTZ_EUNSUPPORTED;  // no pair homography between a map and an image
  if (pr || lp) o.inlier_matches = 1;  // a lone admissible candidate passes the ratio test: the tracked run always gates the assembled query
  for (double& t : res->stage_ms) t = 0;
  if (sl_res) sl_res->shortlist_ms = 0;
  if (pr && pr->res) pr->res->prior_ms = 0;
  if (lp && lp->res) lp->res->view_ms = 0;
  if (ls && ls->sl_res) ls->sl_res->shortlist_ms = 0;
  if (ls && ls->res) ls->res->view_ms = 0;
  ptz_landmark_view_destroy(r->view);  // (whatever this run is, the last run's view goes)
  r->view = nullptr;
  if (n_query == 0) return PTZ_OK;
  const int32_t n_ref = r->n_ref, K = o.max_refs, listed = sl ? sl->max_refs : (pr ? pr->opt.max_refs : n_ref),
                per_query = listed < n_ref ? listed : n_ref;
  if ((int64_t)n_query * per_query > INT32_MAX || (int64_t)n_query * o.max_refs > INT32_MAX) return PTZ_ELIMIT;
  clear_stale_error(who);
  PTZ_DEVICE_GUARD(r->device);
  const size_t nq = (size_t)n_query;
  hipStream_t st = r->st;
  Events ev(r->device);
  PTZ_HIP_TRY(ev.make());
  // the pairs test image by test image, the references in ascending order: FindBestMatch's first-wins tie picks the lowest reference
  std::vector<int32_t> ia, ib;
  std::vector<int64_t> qptr(nq + 1, 0);
  // a downloaded stage 0 -> the pair list, query-major, a query's references in the list's (ascending) order
  const auto pairs_of = [&](const std::vector<int32_t>& list, const std::vector<int32_t>& n_short, size_t R) -> int32_t {
    for (size_t q = 0; q < nq; ++q) {
      const int32_t n = n_short[q];
      if (n < 0 || n > per_query) return PTZ_ENODEVICE;  // (a kernel that did not run)
      for (int32_t k = 0; k < n; ++k) {
        const int32_t ref = list[q * R + k];
        if (ref < 0 || ref >= n_ref) return PTZ_ENODEVICE;
        ia.push_back(ref);
        ib.push_back((int32_t)q);
      }
      qptr[q + 1] = (int64_t)ia.size();
    }
    return PTZ_OK;
  };
  std::optional<CallHeld> prior_held;  // a tracked run's stage 0 block: the pairs' H until the matcher has run, the priors until stage 3 has
  const double *d_prior_H = nullptr, *d_prior_cams = nullptr;
  if (pr) {
    // 0. the overlap lists and the H of every slot from the prior cameras; the host reads the lists and keeps their order
    const size_t R = (size_t)pr->opt.max_refs;
    std::vector<double> pR(9 * nq);
    if (const int32_t rc = ptz_reloc_ref_rotations(n_query, pr->cams, pR.data())) return rc;
    BlockLayout b;
    const size_t o_pc = b.take(sizeof(double) * 15 * nq), o_pR = b.take(sizeof(double) * 9 * nq), o_wh = b.take(sizeof(int32_t) * 2 * nq),
                 o_sl = b.take(sizeof(int32_t) * R * nq), o_ns = b.take(sizeof(int32_t) * nq), o_ov = b.take(sizeof(int32_t) * nq * n_ref),
                 o_Hs = b.take(sizeof(double) * 9 * R * nq), o_qp = b.take(sizeof(int64_t) * (nq + 1)),
                 o_H = b.take(sizeof(double) * 9 * (size_t)per_query * nq);
    std::vector<int32_t> list(R * nq), n_short(nq);
    CallHeld& t = prior_held.emplace(st);
    if (const int32_t rc = t.acquire(r->device, b.total())) return rc;
    char* const p = t.base;
    PTZ_HIP_TRY(hipMemcpyAsync(p + o_pc, pr->cams, sizeof(double) * 15 * nq, hipMemcpyHostToDevice, st));
    PTZ_HIP_TRY(hipMemcpyAsync(p + o_pR, pR.data(), sizeof(double) * 9 * nq, hipMemcpyHostToDevice, st));
    PTZ_HIP_TRY(hipMemcpyAsync(p + o_wh, query_wh, sizeof(int32_t) * 2 * nq, hipMemcpyHostToDevice, st));
    PTZ_HIP_TRY(hipEventRecord(t.ev[0], st));
    if (const int32_t rc = ptz_reloc_prior_pairs_device(n_ref, r->d_cams, r->d_R, n_query, (const double*)(p + o_pc), (const double*)(p + o_pR),
                                                        (const int32_t*)(p + o_wh), o.factor_type, &pr->opt, (int32_t*)(p + o_sl),
                                                        (int32_t*)(p + o_ns), (int32_t*)(p + o_ov), (double*)(p + o_Hs), st))
      return rc;
    PTZ_HIP_TRY(hipEventRecord(t.ev[1], st));
    PTZ_HIP_TRY(hipMemcpyAsync(list.data(), p + o_sl, sizeof(int32_t) * R * nq, hipMemcpyDeviceToHost, st));
    PTZ_HIP_TRY(hipMemcpyAsync(n_short.data(), p + o_ns, sizeof(int32_t) * nq, hipMemcpyDeviceToHost, st));
    if (pr->res && pr->res->overlap) PTZ_HIP_TRY(hipMemcpyAsync(pr->res->overlap, p + o_ov, sizeof(int32_t) * nq * n_ref, hipMemcpyDeviceToHost, st));
    PTZ_HIP_TRY(stream_wait(st));
    PTZ_HIP_TRY(hipGetLastError());
    if (const int32_t rc = pairs_of(list, n_short, R)) return rc;
    if (pr->res) {
      if (pr->res->shortlist) memcpy(pr->res->shortlist, list.data(), sizeof(int32_t) * R * nq);
      if (pr->res->n_short) memcpy(pr->res->n_short, n_short.data(), sizeof(int32_t) * nq);
      pr->res->prior_ms = t.elapsed_ms();
    }
    // the H of every pair of the list, gathered where the matcher reads it; the matcher runs on a stream of its own
    PTZ_HIP_TRY(hipMemcpyAsync(p + o_qp, qptr.data(), sizeof(int64_t) * (nq + 1), hipMemcpyHostToDevice, st));
    reloc_prior_enqueue_gather((int)ia.size(), n_query, (int)R, (const int64_t*)(p + o_qp), (const double*)(p + o_Hs), (double*)(p + o_H), st);
    PTZ_HIP_TRY(hipGetLastError());
    PTZ_HIP_TRY(stream_wait(st));
    d_prior_H = (const double*)(p + o_H);
    d_prior_cams = (const double*)(p + o_pc);
  }
  else if (sl) {
    // 0. the vote pass over the resident references; the host reads the lists and keeps their order
    const size_t R = (size_t)sl->max_refs;
    const int64_t ws = ptz_desc_shortlist_workspace_bytes(r->refs, query_set, n_query, sl);
    BlockLayout b;
    const size_t o_sl = b.take(sizeof(int32_t) * R * nq), o_ns = b.take(sizeof(int32_t) * nq), o_votes = b.take(sizeof(int32_t) * nq * n_ref),
                 o_ws = b.take((size_t)ws);
    std::vector<int32_t> list(R * nq), n_short(nq);
    CallHeld t(st);
    if (const int32_t rc = t.acquire(r->device, b.total())) return rc;
    char* const p = t.base;
    PTZ_HIP_TRY(hipEventRecord(t.ev[0], st));
    if (const int32_t rc = ptz_desc_shortlist_device(r->refs, query_set, n_query, nullptr, &o.match, sl, (int32_t*)(p + o_sl), (int32_t*)(p + o_ns),
                                                     (int32_t*)(p + o_votes), p + o_ws, ws, st))
      return rc;
    PTZ_HIP_TRY(hipEventRecord(t.ev[1], st));
    PTZ_HIP_TRY(hipMemcpyAsync(list.data(), p + o_sl, sizeof(int32_t) * R * nq, hipMemcpyDeviceToHost, st));
    PTZ_HIP_TRY(hipMemcpyAsync(n_short.data(), p + o_ns, sizeof(int32_t) * nq, hipMemcpyDeviceToHost, st));
    if (sl_res && sl_res->votes) PTZ_HIP_TRY(hipMemcpyAsync(sl_res->votes, p + o_votes, sizeof(int32_t) * nq * n_ref, hipMemcpyDeviceToHost, st));
    PTZ_HIP_TRY(stream_wait(st));
    PTZ_HIP_TRY(hipGetLastError());
    if (const int32_t rc = pairs_of(list, n_short, R)) return rc;
    if (sl_res) {
      if (sl_res->shortlist) memcpy(sl_res->shortlist, list.data(), sizeof(int32_t) * R * nq);
      if (sl_res->n_short) memcpy(sl_res->n_short, n_short.data(), sizeof(int32_t) * nq);
      sl_res->shortlist_ms = t.elapsed_ms();
    }
  }
  else if (lmap) {
    ia.assign(nq, 0);  // the map's set is one image
    ib.resize(nq);
    for (int q = 0; q < n_query; ++q) { ib[q] = q; qptr[q + 1] = q + 1; }
    if (lp) {
      // 0. the view of every query's prior: its visible landmarks and their descriptor rows as image q of a set of its own
      std::vector<double> pR(9 * nq);
      if (const int32_t rc = ptz_reloc_ref_rotations(n_query, lp->cams, pR.data())) return rc;
      if (const int32_t rc = ptz_landmark_visible(lmap, n_query, lp->cams, pR.data(), query_wh, o.factor_type, &lp->opt, &r->view)) return rc;
      for (int q = 0; q < n_query; ++q) ia[q] = q;
      res->stage_ms[0] = r->view->device_ms;
      if (lp->res) {
        lp->res->view_ms = r->view->device_ms;
        if (lp->res->n_visible)
          for (size_t q = 0; q < nq; ++q) lp->res->n_visible[q] = (int32_t)(r->view->vis_ptr[q + 1] - r->view->vis_ptr[q]);
      }
    }
    else if (ls) {
      // 0a. the vote pass over the map's home set; the lists stay on the device (sl_res downloads them for the caller)
      const size_t R = (size_t)ls->opt.max_refs;
      const int64_t ws = ptz_landmark_shortlist_workspace_bytes(lmap, query_set, n_query, &ls->opt);
      if (ws <= 0) return PTZ_ENOMEM;  // (a home set that could not be built)
      BlockLayout b;
      const size_t o_sl = b.take(sizeof(int32_t) * R * nq), o_ns = b.take(sizeof(int32_t) * nq), o_votes = b.take(sizeof(int32_t) * nq * n_ref),
                   o_ws = b.take((size_t)ws);
      CallHeld t(st);
      if (const int32_t rc = t.acquire(r->device, b.total())) return rc;
      char* const p = t.base;
      PTZ_HIP_TRY(hipEventRecord(t.ev[0], st));
      if (const int32_t rc = ptz_landmark_shortlist_device(lmap, query_set, n_query, nullptr, &o.match, &ls->opt, (int32_t*)(p + o_sl),
                                                           (int32_t*)(p + o_ns), (int32_t*)(p + o_votes), p + o_ws, ws, st))
        return rc;
      PTZ_HIP_TRY(hipEventRecord(t.ev[1], st));
      if (ls->sl_res) {
        ptz_shortlist_result* sr = ls->sl_res;
        if (sr->shortlist) PTZ_HIP_TRY(hipMemcpyAsync(sr->shortlist, p + o_sl, sizeof(int32_t) * R * nq, hipMemcpyDeviceToHost, st));
        if (sr->n_short) PTZ_HIP_TRY(hipMemcpyAsync(sr->n_short, p + o_ns, sizeof(int32_t) * nq, hipMemcpyDeviceToHost, st));
        if (sr->votes) PTZ_HIP_TRY(hipMemcpyAsync(sr->votes, p + o_votes, sizeof(int32_t) * nq * n_ref, hipMemcpyDeviceToHost, st));
      }
      // 0b. the view of the listed homes, on the same stream: image q of its set holds the landmarks query q is matched against
      ptz_landmark_prior_options vo;
      ptz_landmark_prior_options_default(&vo);
      if (const int32_t rc = ptz_landmark_view_from_homes_device(lmap, n_query, (int32_t)R, (const int32_t*)(p + o_sl), vo.max_view_bytes, st, &r->view))
        return rc;
      PTZ_HIP_TRY(hipGetLastError());
      for (int q = 0; q < n_query; ++q) ia[q] = q;
      if (ls->sl_res) ls->sl_res->shortlist_ms = t.elapsed_ms();
      if (ls->res) {
        ls->res->view_ms = r->view->device_ms;
        if (ls->res->n_visible)
          for (size_t q = 0; q < nq; ++q) ls->res->n_visible[q] = (int32_t)(r->view->vis_ptr[q + 1] - r->view->vis_ptr[q]);
      }
    }
  }
  else {
    ia.resize((size_t)n_query * n_ref);
    ib.resize(ia.size());
    for (int q = 0; q < n_query; ++q) {
      for (int k = 0; k < n_ref; ++k) { ia[(size_t)q * n_ref + k] = k; ib[(size_t)q * n_ref + k] = q; }
      qptr[q + 1] = (int64_t)(q + 1) * n_ref;
    }
  }
  const int32_t npair = (int32_t)ia.size();

  // 1. pass 1 over all pairs; a tracked run: the guided matcher under the predicted H, every pair found, in place of stages 1 and 2
  ptz_desc_matches_destroy(r->table);
  r->table = nullptr;
  ptz_desc_matches* m = nullptr;
  const auto guided = o.guided_grid ? ptz_desc_match_pairs_guided_grid_device : ptz_desc_match_pairs_guided_device;  // the same arrays
  struct Held { ptz_desc_matches*& m; ~Held() { ptz_desc_matches_destroy(m); } } held{m};
  if (pr) {
    if (const int32_t rc = guided(r->refs, query_set, npair, ia.data(), ib.data(), d_prior_H, nullptr, pr->opt.radius_px, &o.match, &m)) return rc;
    res->stage_ms[1] = ptz_desc_matches_device_ms(m);
  }
  else if (lp) {
    if (const int32_t rc = guided(r->view->set, query_set, npair, ia.data(), ib.data(), r->view->d_H, nullptr, lp->opt.radius_px, &o.match, &m)) return rc;
    res->stage_ms[1] = ptz_desc_matches_device_ms(m);
  }
  else {
    if (const int32_t rc = ptz_desc_match_pairs(ls ? r->view->set : (lmap ? lmap->set : r->refs), query_set, npair, ia.data(), ib.data(), &o.match, &m)) return rc;
    res->stage_ms[0] = ptz_desc_matches_device_ms(m);
  }
  int64_t nm = ptz_desc_matches_n_matches(m);
  if (nm > INT32_MAX) return PTZ_ELIMIT;
  const int64_t* d_ptr = nullptr;
  const int32_t* d_ia = nullptr;
  const float *d_ua = nullptr, *d_ub = nullptr;
  if (const int32_t rc = ptz_desc_matches_device_ptrs(m, &d_ptr, &d_ia, nullptr, nullptr, &d_ua, &d_ub)) return rc;
  if (nm > 0 && (!d_ua || !d_ub)) return PTZ_EINVAL;  // sets without key points

  // 2. the gate on all pairs, then the guided pass with its device H / found, as MatchDescriptors composes them
  if (!pr && o.guided_radius > 0.0 && npair > 0) {
    if (const int32_t rc = reloc_gate_for(r, npair, nm, o.gate_max_pair_matches)) return rc;
    const size_t nmx = (size_t)(nm > 0 ? nm : 1);
    BlockLayout b;
    const size_t o_H = b.take(sizeof(double) * 9 * npair), o_f = b.take(sizeof(int32_t) * npair), o_p = b.take(sizeof(int64_t) * ((size_t)npair + 1)),
                 o_a = b.take(sizeof(float) * 2 * nmx), o_b = b.take(sizeof(float) * 2 * nmx);
    CallHeld t(st);
    if (const int32_t rc = t.acquire(r->device, b.total())) return rc;
    char* const p = t.base;
    PTZ_HIP_TRY(hipEventRecord(t.ev[0], st));
    if (const int32_t rc = ptz_match_gate_run_device(r->gate, npair, d_ptr, d_ua, d_ub, o.ransac_thresh, o.min_inliers, (double*)(p + o_H),
                                                     (int32_t*)(p + o_f), nullptr, (int64_t*)(p + o_p), (float*)(p + o_a),
                                                     (float*)(p + o_b), nullptr, st))
      return rc;
    hipLaunchKernelGGL(k_reloc_found, dim3((npair + 255) / 256), dim3(256), 0, st, npair, (const int64_t*)(p + o_p), (int32_t*)(p + o_f));
    PTZ_HIP_TRY(hipGetLastError());
    PTZ_HIP_TRY(hipEventRecord(t.ev[1], st));
    PTZ_HIP_TRY(stream_wait(st));  // the guided call runs on a stream of its own
    ptz_desc_matches* g = nullptr;
    if (const int32_t rc = guided(r->refs, query_set, npair, ia.data(), ib.data(), (const double*)(p + o_H), (const int32_t*)(p + o_f),
                                  o.guided_radius, &o.match, &g))
      return rc;
    ptz_desc_matches_destroy(m);
    m = g;
    res->stage_ms[1] = t.elapsed_ms() + ptz_desc_matches_device_ms(m);
    nm = ptz_desc_matches_n_matches(m);
    if (nm > INT32_MAX) return PTZ_ELIMIT;
    if (const int32_t rc = ptz_desc_matches_device_ptrs(m, &d_ptr, nullptr, nullptr, nullptr, &d_ua, &d_ub)) return rc;
  }

  // the run's block
  const bool gated = o.inlier_matches != 0, trimming = o.trim != 0, cov = o.uncertainty != 0;
  const int nf = ptz_krt_free_dim(o.factor_type);
  const size_t nmx = (size_t)(nm > 0 ? nm : 1);
  const int64_t ws_asm = lmap ? ptz_landmark_assemble_workspace_bytes(n_query, nm) : ptz_reloc_assemble_workspace_bytes(n_query, nm);
  const int64_t ws_trim = trimming ? ptz_krt_trim_workspace_bytes(n_query, nm) : 0;
  BlockLayout b;
  const size_t o_pref = b.take(sizeof(int32_t) * npair), o_qptr = b.take(sizeof(int64_t) * (nq + 1)), o_wh = b.take(sizeof(int32_t) * 2 * nq),
               o_sel = b.take(sizeof(int32_t) * K * nq), o_nsel = b.take(sizeof(int32_t) * nq), o_optr = b.take(sizeof(int64_t) * (nq + 1)),
               o_oa = b.take(sizeof(float) * 2 * nmx), o_ob = b.take(sizeof(float) * 2 * nmx), o_osrc = b.take(sizeof(int32_t) * nmx),
               o_cref = b.take(sizeof(double) * 15 * nq), o_ccur = b.take(sizeof(double) * 15 * nq), o_ws = b.take((size_t)ws_asm),
               o_sum = b.take(sizeof(ptz_lm_summary) * nq), o_acc = b.take(sizeof(int32_t) * nq), o_H = b.take(sizeof(double) * 9 * nq),
               o_found = b.take(sizeof(int32_t) * nq), o_mask = b.take(nmx), o_gptr = b.take(sizeof(int64_t) * (nq + 1)),
               o_ga = b.take(sizeof(float) * 2 * nmx), o_gb = b.take(sizeof(float) * 2 * nmx), o_kept = b.take(nmx),
               o_rep = b.take(sizeof(ptz_krt_trim_report) * nq), o_wst = b.take((size_t)ws_trim), o_cov = b.take(sizeof(double) * nf * nf * nq),
               o_s0 = b.take(sizeof(double) * nq), o_cst = b.take(sizeof(int32_t) * nq), o_lift = b.take(lp || ls ? sizeof(int32_t) * nmx : 0),
               o_model = b.take(sizeof(double) * 10 * nq);
  ptzpool::dev_release(r->device, r->blk);
  r->blk = nullptr; r->n_query = 0; r->kept = 0; r->has_models = false;
  if (ptzpool::dev_acquire(r->device, b.total(), (void**)&r->blk) != hipSuccess) return PTZ_ENOMEM;
  char* d = r->blk;
  if (npair > 0) PTZ_HIP_TRY(hipMemcpyAsync(d + o_pref, ia.data(), sizeof(int32_t) * npair, hipMemcpyHostToDevice, st));
  PTZ_HIP_TRY(hipMemcpyAsync(d + o_qptr, qptr.data(), sizeof(int64_t) * (nq + 1), hipMemcpyHostToDevice, st));
  PTZ_HIP_TRY(hipMemcpyAsync(d + o_wh, query_wh, sizeof(int32_t) * 2 * nq, hipMemcpyHostToDevice, st));

  // 3. the assembly
  PTZ_HIP_TRY(hipEventRecord(ev.e[0], st));
  if (lmap) {  // the anchor takes slot 0 of sel (K = 1); n_sel is derived on the host
    if (lp || ls) {
      hipLaunchKernelGGL(k_reloc_lift, dim3((n_query + 3) / 4), dim3(256), 0, st, n_query, d_ptr, d_ia, r->view->d_vis_ptr, r->view->d_vis_lm,
                         (int32_t*)(d + o_lift));
      PTZ_HIP_TRY(hipGetLastError());
      d_ia = (const int32_t*)(d + o_lift);
    }
    if (const int32_t rc = ptz_landmark_assemble_device(lmap, n_query, nm, d_ptr, d_ia, d_ub, r->d_cams, r->d_R, (const int32_t*)(d + o_wh), o.factor_type,
                                                        (int32_t*)(d + o_sel), (int64_t*)(d + o_optr), (float*)(d + o_oa), (float*)(d + o_ob),
                                                        (int32_t*)(d + o_osrc), (double*)(d + o_cref), (double*)(d + o_ccur), d + o_ws, ws_asm, st))
      return rc;
  }
  else if (const int32_t rc = ptz_reloc_assemble_device(n_query, npair, nm, n_ref, d_ptr, d_ua, d_ub, (const int32_t*)(d + o_pref), (const int64_t*)(d + o_qptr),
                                                   r->d_cams, r->d_R, (const int32_t*)(d + o_wh), o.factor_type, K, (int32_t*)(d + o_sel),
                                                   (int32_t*)(d + o_nsel), (int64_t*)(d + o_optr), (float*)(d + o_oa), (float*)(d + o_ob),
                                                   (int32_t*)(d + o_osrc), (double*)(d + o_cref), (double*)(d + o_ccur), d + o_ws, ws_asm, st))
    return rc;
  if (pr || lp) {  // the solve starts from the prior's focal, rotation and distortion (one small launch, inside stage 3's stamp)
    reloc_prior_enqueue_cams(n_query, pr ? d_prior_cams : r->view->d_prior_cams, o.factor_type, (double*)(d + o_ccur), st);
    PTZ_HIP_TRY(hipGetLastError());
  }
  PTZ_HIP_TRY(hipEventRecord(ev.e[1], st));
  std::vector<int64_t> optr(nq + 1), gptr(nq + 1, 0);
  PTZ_HIP_TRY(hipMemcpyAsync(optr.data(), d + o_optr, sizeof(int64_t) * (nq + 1), hipMemcpyDeviceToHost, st));
  PTZ_HIP_TRY(stream_wait(st));  // the one word the host needs: the extent of the assembled arrays
  const int64_t kept = optr[nq];
  if (kept < 0 || kept > nm) return PTZ_ENODEVICE;
  const int64_t* a_ptr = (const int64_t*)(d + o_optr);
  const float *a_ref = (const float*)(d + o_oa), *a_cur = (const float*)(d + o_ob);
  const double* a_cref = (const double*)(d + o_cref);
  double* a_ccur = (double*)(d + o_ccur);
  ptz_lm_summary* d_sum = (ptz_lm_summary*)(d + o_sum);
  int32_t* d_acc = (int32_t*)(d + o_acc);
  uint8_t *d_mask = (uint8_t*)(d + o_mask), *d_kept = (uint8_t*)(d + o_kept);

  // 4. the gate on the assembled queries
  if (gated) {
    if (r->gate_model == 1) {  // the assembled query's own model: f and R between the (virtual) anchor and the query, no size limit
      if (const int32_t rc = reloc_rf_gate_for(r, n_query, nm)) return rc;
      PTZ_HIP_TRY(hipMemsetAsync(d + o_model, 0, sizeof(double) * 10 * nq, st));
      if (const int32_t rc = ptz_rotfocal_gate_run_device(r->rf_gate, n_query, a_ptr, a_ref, a_cur, a_cref, a_ccur, o.ransac_thresh, o.min_inliers,
                                                          r->gate_iters, (double*)(d + o_model), nullptr, (int32_t*)(d + o_found), d_mask,
                                                          (int64_t*)(d + o_gptr), (float*)(d + o_ga), (float*)(d + o_gb), nullptr, st))
        return rc;
    }
    else {
      if (const int32_t rc = reloc_gate_for(r, n_query, nm, o.gate_max_pair_matches)) return rc;
      if (const int32_t rc = ptz_match_gate_run_device(r->gate, n_query, a_ptr, a_ref, a_cur, o.ransac_thresh, o.min_inliers, (double*)(d + o_H),
                                                       (int32_t*)(d + o_found), d_mask, (int64_t*)(d + o_gptr), (float*)(d + o_ga),
                                                       (float*)(d + o_gb), nullptr, st))
        return rc;
    }
    hipLaunchKernelGGL(k_reloc_universe, dim3((n_query + 3) / 4), dim3(256), 0, st, n_query, a_ptr, (const int64_t*)(d + o_gptr), d_mask);
    PTZ_HIP_TRY(hipGetLastError());
    PTZ_HIP_TRY(hipMemcpyAsync(gptr.data(), d + o_gptr, sizeof(int64_t) * (nq + 1), hipMemcpyDeviceToHost, st));
  }
  PTZ_HIP_TRY(hipEventRecord(ev.e[2], st));

  // 5. the solve: on the gate's compacted CSR, or the trimming loop over the assembled arrays with the gate's set as its universe
  if (trimming) {
    PTZ_HIP_TRY(hipMemsetAsync(d + o_rep, 0, sizeof(ptz_krt_trim_report) * nq, st));
    if (const int32_t rc = ptz_krt_solve_batch_trimmed_device(n_query, kept, a_ptr, a_ref, a_cur, nullptr, nullptr, nullptr, a_cref, a_ccur, o.factor_type,
                                                              o.max_reproj_error, gated ? d_mask : nullptr, &o.trim_options, &o.lm, d_sum, d_acc,
                                                              d_kept, (ptz_krt_trim_report*)(d + o_rep), d + o_wst, ws_trim, st))
      return rc;
  }
  else if (const int32_t rc = gated ? ptz_krt_solve_batch_device(n_query, (const int64_t*)(d + o_gptr), (const float*)(d + o_ga), (const float*)(d + o_gb),
                                                                  nullptr, nullptr, nullptr, a_cref, a_ccur, o.factor_type, o.max_reproj_error, &o.lm,
                                                                  d_sum, d_acc, st)
                                    : ptz_krt_solve_batch_device(n_query, a_ptr, a_ref, a_cur, nullptr, nullptr, nullptr, a_cref, a_ccur, o.factor_type,
                                                                  o.max_reproj_error, &o.lm, d_sum, d_acc, st))
    return rc;
  if (pr || lp) {
    hipLaunchKernelGGL(k_reloc_lost, dim3((n_query + 255) / 256), dim3(256), 0, st, n_query, (const int64_t*)(d + o_gptr), d_acc);
    PTZ_HIP_TRY(hipGetLastError());
  }
  PTZ_HIP_TRY(hipEventRecord(ev.e[3], st));

  // 6. the covariance over the matches a query kept
  if (cov) {
    PTZ_HIP_TRY(hipMemsetAsync(d + o_cov, 0, sizeof(double) * nf * nf * nq, st));
    PTZ_HIP_TRY(hipMemsetAsync(d + o_s0, 0, sizeof(double) * nq, st));
    if (const int32_t rc = ptz_krt_covariance_batch_device(n_query, a_ptr, a_ref, a_cur, nullptr, nullptr, nullptr, a_cref, a_ccur, o.factor_type,
                                                           trimming ? d_kept : (gated ? d_mask : nullptr), d_acc, 0.0, (double*)(d + o_cov),
                                                           (double*)(d + o_s0), (int32_t*)(d + o_cst), st))
      return rc;
  }
  PTZ_HIP_TRY(hipEventRecord(ev.e[4], st));

  // only per-query results reach the host
  std::vector<int32_t> sel(res->sel_ref || (lmap && res->n_sel) ? (size_t)K * nq : 0);
  if (res->cam) PTZ_HIP_TRY(hipMemcpyAsync(res->cam, a_ccur, sizeof(double) * 15 * nq, hipMemcpyDeviceToHost, st));
  if (res->accepted) PTZ_HIP_TRY(hipMemcpyAsync(res->accepted, d_acc, sizeof(int32_t) * nq, hipMemcpyDeviceToHost, st));
  if (res->summaries) PTZ_HIP_TRY(hipMemcpyAsync(res->summaries, d_sum, sizeof(ptz_lm_summary) * nq, hipMemcpyDeviceToHost, st));
  if (!sel.empty()) PTZ_HIP_TRY(hipMemcpyAsync(sel.data(), d + o_sel, sizeof(int32_t) * K * nq, hipMemcpyDeviceToHost, st));
  if (res->n_sel && !lmap) PTZ_HIP_TRY(hipMemcpyAsync(res->n_sel, d + o_nsel, sizeof(int32_t) * nq, hipMemcpyDeviceToHost, st));
  if (res->trim_report && trimming) PTZ_HIP_TRY(hipMemcpyAsync(res->trim_report, d + o_rep, sizeof(ptz_krt_trim_report) * nq, hipMemcpyDeviceToHost, st));
  if (cov) {
    if (res->cov) PTZ_HIP_TRY(hipMemcpyAsync(res->cov, d + o_cov, sizeof(double) * nf * nf * nq, hipMemcpyDeviceToHost, st));
    if (res->sigma0) PTZ_HIP_TRY(hipMemcpyAsync(res->sigma0, d + o_s0, sizeof(double) * nq, hipMemcpyDeviceToHost, st));
    if (res->cov_status) PTZ_HIP_TRY(hipMemcpyAsync(res->cov_status, d + o_cst, sizeof(int32_t) * nq, hipMemcpyDeviceToHost, st));
  }
  PTZ_HIP_TRY(stream_wait(st));
  PTZ_HIP_TRY(hipGetLastError());
  for (size_t q = 0; q < nq; ++q) {
    if (res->n_matches) res->n_matches[q] = (int32_t)(optr[q + 1] - optr[q]);
    if (res->n_inliers) res->n_inliers[q] = (int32_t)(gated ? gptr[q + 1] - gptr[q] : optr[q + 1] - optr[q]);
    if (lmap) {  // sel holds reference images already
      const int32_t a = sel.empty() ? -1 : sel[q];
      if (res->sel_ref) res->sel_ref[q] = a >= 0 && a < n_ref ? a : -1;
      if (res->n_sel) res->n_sel[q] = a >= 0 && a < n_ref ? 1 : 0;
    }
    else if (res->sel_ref)
      for (int s = 0; s < K; ++s) { const int32_t p = sel[q * K + s]; res->sel_ref[q * K + s] = p < 0 || p >= npair ? -1 : ia[p]; }
  }
  res->stage_ms[2] = ev.ms(0, 1); res->stage_ms[3] = gated ? ev.ms(1, 2) : 0; res->stage_ms[4] = ev.ms(2, 3); res->stage_ms[5] = cov ? ev.ms(3, 4) : 0;
  r->n_query = n_query; r->kept = kept;
  r->table = m;  // (kept for ptz_relocalizer_table)
  m = nullptr;
  r->pair_ref.swap(ia);
  r->query_ptr.swap(qptr);
  r->o_optr = o_optr; r->o_oa = o_oa; r->o_ob = o_ob; r->o_osrc = o_osrc; r->o_model = o_model; r->o_found = o_found;
  r->has_models = gated && r->gate_model == 1;
  return PTZ_OK;
}

extern "C" int32_t ptz_relocalizer_run(ptz_relocalizer* r, const ptz_desc_set* query_set, int32_t n_query, const int32_t* query_wh,
                                       const ptz_reloc_options* options, ptz_reloc_result* res)
{
  return reloc_run(__func__, r, query_set, n_query, query_wh, options, nullptr, res, nullptr);
}

extern "C" int32_t ptz_relocalizer_run_shortlisted(ptz_relocalizer* r, const ptz_desc_set* query_set, int32_t n_query, const int32_t* query_wh,
                                                   const ptz_reloc_options* options, const ptz_shortlist_options* sl_opt, ptz_reloc_result* res,
                                                   ptz_shortlist_result* sl_res)
{
  ptz_shortlist_options s;
  ptz_shortlist_options_default(&s);
  if (sl_opt) s = *sl_opt;
  return reloc_run(__func__, r, query_set, n_query, query_wh, options, &s, res, sl_res);
}

extern "C" int32_t ptz_relocalizer_run_tracked(ptz_relocalizer* r, const ptz_desc_set* query_set, int32_t n_query, const int32_t* query_wh,
                                               const double* prior_cams, const ptz_reloc_options* options, const ptz_prior_options* prior_opt,
                                               ptz_reloc_result* res, ptz_prior_result* prior_res)
{
  RelocPrior p = {prior_cams, {}, prior_res};
  ptz_prior_options_default(&p.opt);
  if (prior_opt) p.opt = *prior_opt;
  return reloc_run(__func__, r, query_set, n_query, query_wh, options, nullptr, res, nullptr, &p);
}

extern "C" int32_t ptz_relocalizer_run_landmarks(ptz_relocalizer* r, const ptz_landmark_map* map, const ptz_desc_set* query_set, int32_t n_query,
                                                 const int32_t* query_wh, const ptz_reloc_options* options, ptz_reloc_result* res)
{
  if (!map) return PTZ_EINVAL;
  return reloc_run(__func__, r, query_set, n_query, query_wh, options, nullptr, res, nullptr, nullptr, map);
}

extern "C" int32_t ptz_relocalizer_run_landmarks_tracked(ptz_relocalizer* r, const ptz_landmark_map* map, const ptz_desc_set* query_set,
                                                         int32_t n_query, const int32_t* query_wh, const double* prior_cams,
                                                         const ptz_reloc_options* options, const ptz_landmark_prior_options* lp_opt,
                                                         ptz_reloc_result* res, ptz_landmark_view_result* view_res)
{
  if (!map) return PTZ_EINVAL;
  RelocLmPrior p = {prior_cams, {}, view_res};
  ptz_landmark_prior_options_default(&p.opt);
  if (lp_opt) p.opt = *lp_opt;
  return reloc_run(__func__, r, query_set, n_query, query_wh, options, nullptr, res, nullptr, nullptr, map, &p);
}

extern "C" int32_t ptz_relocalizer_run_landmarks_shortlisted(ptz_relocalizer* r, const ptz_landmark_map* map, const ptz_desc_set* query_set,
                                                             int32_t n_query, const int32_t* query_wh, const ptz_reloc_options* options,
                                                             const ptz_shortlist_options* sl_opt, ptz_reloc_result* res,
                                                             ptz_shortlist_result* sl_res, ptz_landmark_view_result* view_res)
{
  if (!map) return PTZ_EINVAL;
  RelocLmShort s = {{}, sl_res, view_res};
  ptz_shortlist_options_default(&s.opt);
  if (sl_opt) s.opt = *sl_opt;
  return reloc_run(__func__, r, query_set, n_query, query_wh, options, nullptr, res, nullptr, nullptr, map, nullptr, &s);
}

extern "C" int32_t ptz_relocalizer_view(const ptz_relocalizer* r, int64_t* n_visible, int64_t* vis_ptr, int32_t* vis_lm, float* vis_uv)
{
  if (!r || !r->view || r->n_query <= 0 || r->view->n_query != r->n_query) return PTZ_EINVAL;  // (a run that failed leaves no view to read)
  if (n_visible) *n_visible = ptz_landmark_view_n_visible(r->view);
  return ptz_landmark_view_download(r->view, vis_ptr, vis_lm, vis_uv);
}

extern "C" int32_t ptz_relocalizer_pairs(const ptz_relocalizer* r, int32_t* n_pair, int32_t* pair_ref, int64_t* query_ptr)
{
  if (!r || r->n_query <= 0) return PTZ_EINVAL;
  if (n_pair) *n_pair = (int32_t)r->pair_ref.size();
  if (pair_ref && !r->pair_ref.empty()) memcpy(pair_ref, r->pair_ref.data(), sizeof(int32_t) * r->pair_ref.size());
  if (query_ptr) memcpy(query_ptr, r->query_ptr.data(), sizeof(int64_t) * r->query_ptr.size());
  return PTZ_OK;
}

extern "C" int32_t ptz_relocalizer_set_gate_model(ptz_relocalizer* r, int32_t gate_model, int32_t gate_iters)
{
  if (!r || (gate_model != 0 && gate_model != 1) || gate_iters < 1 || gate_iters > 4096) return PTZ_EINVAL;
  r->gate_model = gate_model;
  r->gate_iters = gate_iters;
  return PTZ_OK;
}

extern "C" int32_t ptz_relocalizer_gate_models(const ptz_relocalizer* r, double* model, int32_t* found)
{
  using namespace ptz;
  if (!r || !r->blk || r->n_query <= 0 || !r->has_models) return PTZ_EINVAL;
  PTZ_DEVICE_GUARD(r->device);
  if (model) PTZ_HIP_TRY(hipMemcpyAsync(model, r->blk + r->o_model, sizeof(double) * 10 * (size_t)r->n_query, hipMemcpyDeviceToHost, r->st));
  if (found) PTZ_HIP_TRY(hipMemcpyAsync(found, r->blk + r->o_found, sizeof(int32_t) * (size_t)r->n_query, hipMemcpyDeviceToHost, r->st));
  PTZ_HIP_TRY(stream_wait(r->st));
  return PTZ_OK;
}

extern "C" const ptz_desc_matches* ptz_relocalizer_table(const ptz_relocalizer* r) { return r ? r->table : nullptr; }

extern "C" int64_t ptz_relocalizer_n_matches(const ptz_relocalizer* r) { return r ? r->kept : 0; }

extern "C" int32_t ptz_relocalizer_matches(const ptz_relocalizer* r, int64_t* match_ptr, float* uv_ref, float* uv_cur, int32_t* src)
{
  using namespace ptz;
  if (!r || !r->blk || r->n_query <= 0) return PTZ_EINVAL;
  PTZ_DEVICE_GUARD(r->device);
  if (match_ptr) PTZ_HIP_TRY(hipMemcpyAsync(match_ptr, r->blk + r->o_optr, sizeof(int64_t) * ((size_t)r->n_query + 1), hipMemcpyDeviceToHost, r->st));
  if (r->kept > 0) {
    if (uv_ref) PTZ_HIP_TRY(hipMemcpyAsync(uv_ref, r->blk + r->o_oa, sizeof(float) * 2 * r->kept, hipMemcpyDeviceToHost, r->st));
    if (uv_cur) PTZ_HIP_TRY(hipMemcpyAsync(uv_cur, r->blk + r->o_ob, sizeof(float) * 2 * r->kept, hipMemcpyDeviceToHost, r->st));
    if (src) PTZ_HIP_TRY(hipMemcpyAsync(src, r->blk + r->o_osrc, sizeof(int32_t) * r->kept, hipMemcpyDeviceToHost, r->st));
  }
  PTZ_HIP_TRY(stream_wait(r->st));
  return PTZ_OK;
}
