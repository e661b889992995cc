// ptz_ba_trim.cc -- host logic of the trimmed bundle adjustment: re-packing a problem without its rejected observations
// (ptz_ba_problem_trim, no device) and the loop solve / report / select / re-pack / solve again (ptz_ba_solve_trimmed_batch), which
// drives the batch API as any caller would: a problem's result is what the manual loop over the same calls gives.
#include <cstring>
#include <vector>

#include "../../include/ptz_calib_amd.h"
#include "ptz_ba_trim.h"

namespace {

bool problem_well_formed(const ptz_ba_problem* p)
{
  if (!p || p->n_cam <= 0 || p->n_ray <= 0 || p->n_obs <= 0 || p->n_obs > 0x7fffffff) return false;
  if (!p->obs_uv || !p->obs_cam || !p->obs_ray || !p->ray_weight) return false;
  int prev = 0;
  for (int64_t a = 0; a < p->n_obs; ++a) {
    const int r = p->obs_ray[a], c = p->obs_cam[a];
    if (r < prev || r >= p->n_ray || c < 0 || c >= p->n_cam) return false;
    prev = r;
  }
  return true;
}

// one problem of the trimmed solve: its current (re-packed) arrays, and where its rays and observations came from
struct TrimProblem {
  std::vector<float> uv;
  std::vector<int32_t> cam, ray;
  std::vector<double> w;
  int32_t n_ray = 0;
  std::vector<int32_t> ray_orig;  // current ray -> input ray
  std::vector<int64_t> obs_orig;  // current observation -> input observation
  std::vector<double> x_cam, x_ray;  // state: cameras, rays in the current numbering
  double tlw[6] = {0, 0, 0, 0, 0, 0};
  bool active = true;
  ptz_ba_problem view(const ptz_ba_problem& in) const
  {
    ptz_ba_problem p = in;
    p.n_ray = n_ray; p.n_obs = (int64_t)cam.size();
    p.obs_uv = uv.data(); p.obs_cam = cam.data(); p.obs_ray = ray.data(); p.ray_weight = w.data();
    return p;
  }
};

}  // namespace

extern "C" {

void ptz_trim_options_default(ptz_trim_options* o)
{
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->trim_px = 4.0;
  o->k_sigma = 3.0;
  o->max_rounds = 8;
}

int32_t ptz_ba_problem_trim(const ptz_ba_problem* in, const uint8_t* reject, float* obs_uv_out, int32_t* obs_cam_out, int32_t* obs_ray_out,
                            double* ray_weight_out, int32_t* ray_map, int32_t* n_ray_out, int64_t* n_obs_out)
{
  if (!problem_well_formed(in) || !reject || !obs_uv_out || !obs_cam_out || !obs_ray_out || !ray_weight_out || !ray_map || !n_ray_out || !n_obs_out)
    return PTZ_EINVAL;
  const ptz::TrimRule rule{1.0, 0.0, 2};
  const int64_t n_obs = in->n_obs;
  // what every ray keeps; a ray left below the minimum goes with what it still had
  std::vector<int32_t> left(in->n_ray, 0), total(in->n_ray, 0);
  for (int64_t a = 0; a < n_obs; ++a) {
    ++total[in->obs_ray[a]];
    if (!reject[a]) ++left[in->obs_ray[a]];
  }
  std::vector<int32_t> map(in->n_ray);
  int32_t nr = 0;
  for (int32_t r = 0; r < in->n_ray; ++r) map[r] = ptz::trim_ray_survives(rule, left[r]) ? nr++ : -1;
  std::vector<int32_t> cam_left(in->n_cam, 0);
  int64_t no = 0;
  for (int64_t a = 0; a < n_obs; ++a)
    if (!reject[a] && map[in->obs_ray[a]] >= 0) { ++cam_left[in->obs_cam[a]]; ++no; }
  for (int32_t c = 0; c < in->n_cam; ++c)
    if (cam_left[c] == 0) return PTZ_ENOOBS;  // trimming never drops a view: nothing is written
  int64_t k = 0;
  for (int64_t a = 0; a < n_obs; ++a) {
    const int32_t r = map[in->obs_ray[a]];
    if (reject[a] || r < 0) continue;
    obs_uv_out[2 * k] = in->obs_uv[2 * a]; obs_uv_out[2 * k + 1] = in->obs_uv[2 * a + 1];
    obs_cam_out[k] = in->obs_cam[a];
    obs_ray_out[k] = r;
    ++k;
  }
  for (int32_t r = 0; r < in->n_ray; ++r) {
    ray_map[r] = map[r];
    if (map[r] >= 0) ray_weight_out[map[r]] = in->ray_weight[r] - (double)(total[r] - left[r]);
  }
  *n_ray_out = nr;
  *n_obs_out = no;
  return PTZ_OK;
}

int32_t ptz_ba_solve_trimmed_batch(int32_t n, const ptz_ba_problem* problems, double* cam, double* ray, double* tlw, const ptz_trim_options* trim,
                                   const ptz_lm_options* opt, ptz_lm_summary* summaries, uint8_t* kept, ptz_trim_report* report)
{
  if (n < 0 || (n > 0 && (!problems || !cam || !ray))) return PTZ_EINVAL;
  ptz_trim_options to;
  ptz_trim_options_default(&to);
  if (trim) to = *trim;
  const ptz::TrimRule rule{to.trim_px, to.k_sigma, 2};
  if (!ptz::trim_rule_valid(rule) || to.max_rounds < 1) return PTZ_EINVAL;
  if (n == 0) return PTZ_OK;
  for (int i = 0; i < n; ++i) {
    if (!problem_well_formed(&problems[i])) return PTZ_EINVAL;
    if (problems[i].factor_type < PTZ_BA_PTZRay || problems[i].factor_type > PTZ_BA_PTZRayFxfyDist || problems[i].ic_of_cam) return PTZ_EUNSUPPORTED;
  }
  std::vector<TrimProblem> tp(n);
  std::vector<size_t> cam_off(n + 1, 0), ray_off(n + 1, 0), obs_off(n + 1, 0);
  for (int i = 0; i < n; ++i) {
    const ptz_ba_problem& p = problems[i];
    cam_off[i + 1] = cam_off[i] + p.n_cam; ray_off[i + 1] = ray_off[i] + p.n_ray; obs_off[i + 1] = obs_off[i] + (size_t)p.n_obs;
    TrimProblem& t = tp[i];
    t.uv.assign(p.obs_uv, p.obs_uv + 2 * p.n_obs); t.cam.assign(p.obs_cam, p.obs_cam + p.n_obs); t.ray.assign(p.obs_ray, p.obs_ray + p.n_obs);
    t.w.assign(p.ray_weight, p.ray_weight + p.n_ray);
    t.n_ray = p.n_ray;
    t.ray_orig.resize(p.n_ray); t.obs_orig.resize(p.n_obs);
    for (int32_t r = 0; r < p.n_ray; ++r) t.ray_orig[r] = r;
    for (int64_t a = 0; a < p.n_obs; ++a) t.obs_orig[a] = a;
    t.x_cam.assign(cam + 15 * cam_off[i], cam + 15 * cam_off[i + 1]);
    t.x_ray.assign(ray + 3 * ray_off[i], ray + 3 * ray_off[i + 1]);
    if (tlw) memcpy(t.tlw, tlw + 6 * (size_t)i, sizeof(t.tlw));
  }
  std::vector<ptz_trim_report> rep(n);
  for (auto& r : rep) memset(&r, 0, sizeof(r));
  std::vector<ptz_lm_summary> summ(n);
  std::vector<int> act(n);
  for (int i = 0; i < n; ++i) act[i] = i;
  int32_t rc = PTZ_OK;
  while (!act.empty() && rc == PTZ_OK) {
    // the problems still active, as they stand, solved together from where their last round ended
    const int m = (int)act.size();
    std::vector<ptz_ba_problem> bp(m);
    std::vector<double> bc, br, bt;
    for (int k = 0; k < m; ++k) {
      const TrimProblem& t = tp[act[k]];
      bp[k] = t.view(problems[act[k]]);
      bc.insert(bc.end(), t.x_cam.begin(), t.x_cam.end());
      br.insert(br.end(), t.x_ray.begin(), t.x_ray.end());
      bt.insert(bt.end(), t.tlw, t.tlw + 6);
    }
    ptz_ba_batch* b = nullptr;
    rc = ptz_ba_batch_create(m, bp.data(), opt, &b);
    if (rc) break;
    std::vector<ptz_lm_summary> bs(m);
    size_t tot_obs = 0;
    for (int k = 0; k < m; ++k) tot_obs += (size_t)bp[k].n_obs;
    std::vector<uint8_t> rej(tot_obs);
    std::vector<double> thr(m), rms(m);
    std::vector<int32_t> nrej(m);
    rc = ptz_ba_batch_set_state(b, bc.data(), br.data(), bt.data());
    if (!rc) rc = ptz_ba_batch_solve(b, bs.data());
    if (!rc) rc = ptz_ba_batch_get_state(b, bc.data(), br.data(), bt.data());
    if (!rc) rc = ptz_ba_batch_residuals(b, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, rms.data(), nullptr, nullptr, nullptr, nullptr);
    if (!rc) rc = ptz_ba_batch_trim_select(b, rule.trim_px, rule.k_sigma, rej.data(), thr.data(), nrej.data(), nullptr);
    ptz_ba_batch_destroy(b);
    if (rc) break;
    std::vector<int> next;
    size_t co = 0, ro = 0, oo = 0;
    for (int k = 0; k < m; ++k) {
      const int i = act[k];
      TrimProblem& t = tp[i];
      ptz_trim_report& r = rep[i];
      const size_t nc = t.x_cam.size(), nr = t.x_ray.size(), no = t.cam.size();
      memcpy(t.x_cam.data(), bc.data() + co, sizeof(double) * nc);
      memcpy(t.x_ray.data(), br.data() + ro, sizeof(double) * nr);
      memcpy(t.tlw, bt.data() + 6 * (size_t)k, sizeof(t.tlw));
      summ[i] = bs[k];
      if (r.rounds == 0) r.rms_first = rms[k];
      r.rms_last = rms[k];
      r.threshold = thr[k];
      ++r.rounds;
      const uint8_t* rj = rej.data() + oo;
      co += nc; ro += nr; oo += no;
      if (nrej[k] == 0) continue;                                           // nothing left above the threshold: finished
      if (r.rounds >= to.max_rounds) { r.flags |= PTZ_TRIM_MAX_ROUNDS; continue; }  // has used its rounds
      const ptz_ba_problem cur = t.view(problems[i]);
      std::vector<float> uv(2 * no);
      std::vector<int32_t> oc(no), orr(no), map(t.n_ray);
      std::vector<double> w(t.n_ray);
      int32_t n_ray2 = 0;
      int64_t n_obs2 = 0;
      const int32_t trc = ptz_ba_problem_trim(&cur, rj, uv.data(), oc.data(), orr.data(), w.data(), map.data(), &n_ray2, &n_obs2);
      if (trc == PTZ_ENOOBS) { r.flags |= PTZ_TRIM_ENOOBS; continue; }      // a view would go: finished at this round's result
      if (trc) { rc = trc; break; }
      // observations and rays that stay, and the rays' state through the map
      std::vector<int64_t> obs_orig2;
      obs_orig2.reserve((size_t)n_obs2);
      for (size_t a = 0; a < no; ++a)
        if (!rj[a] && map[t.ray[a]] >= 0) obs_orig2.push_back(t.obs_orig[a]);
      std::vector<int32_t> ray_orig2(n_ray2);
      std::vector<double> x_ray2(3 * (size_t)n_ray2);
      for (int32_t q = 0; q < t.n_ray; ++q) {
        if (map[q] < 0) continue;
        ray_orig2[map[q]] = t.ray_orig[q];
        for (int e = 0; e < 3; ++e) x_ray2[3 * (size_t)map[q] + e] = t.x_ray[3 * (size_t)q + e];
      }
      uv.resize(2 * (size_t)n_obs2); oc.resize((size_t)n_obs2); orr.resize((size_t)n_obs2); w.resize(n_ray2);
      t.uv.swap(uv); t.cam.swap(oc); t.ray.swap(orr); t.w.swap(w);
      t.n_ray = n_ray2;
      t.ray_orig.swap(ray_orig2); t.obs_orig.swap(obs_orig2); t.x_ray.swap(x_ray2);
      next.push_back(i);
    }
    act.swap(next);
  }
  if (rc) return rc;
  for (int i = 0; i < n; ++i) {
    const TrimProblem& t = tp[i];
    memcpy(cam + 15 * cam_off[i], t.x_cam.data(), sizeof(double) * t.x_cam.size());
    for (int32_t q = 0; q < t.n_ray; ++q)
      for (int e = 0; e < 3; ++e) ray[3 * (ray_off[i] + (size_t)t.ray_orig[q]) + e] = t.x_ray[3 * (size_t)q + e];
    if (tlw) memcpy(tlw + 6 * (size_t)i, t.tlw, sizeof(t.tlw));
    if (summaries) summaries[i] = summ[i];
    if (kept) {
      memset(kept + obs_off[i], 0, obs_off[i + 1] - obs_off[i]);
      for (int64_t a : t.obs_orig) kept[obs_off[i] + (size_t)a] = 1;
    }
    rep[i].n_obs_removed = (int64_t)(obs_off[i + 1] - obs_off[i]) - (int64_t)t.cam.size();
    rep[i].n_ray_removed = problems[i].n_ray - t.n_ray;
    if (report) report[i] = rep[i];
  }
  return PTZ_OK;
}

int32_t ptz_ba_solve_trimmed(const ptz_ba_problem* p, double* cam, double* ray, double* tlw, const ptz_trim_options* trim, const ptz_lm_options* opt,
                             ptz_lm_summary* summary, uint8_t* kept, ptz_trim_report* report)
{
  if (!p) return PTZ_EINVAL;
  return ptz_ba_solve_trimmed_batch(1, p, cam, ray, tlw, trim, opt, summary, kept, report);
}

}  // extern "C"
