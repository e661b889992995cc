// run_ptz_ba -- PTZ-IBA + georeferencing from a directory of images, COLMAP-format features and matches, and an annotation
// file; writes <output>/<basename(images)>.json.  Same options, stages, messages and exit codes as the reference tool
// (src/app/run_ptz_ba.cc:24-154): 0 on success, -1 when a stage fails, 1 on bad options.  Every solve runs on the MI355X
// library through the C++ classes of ptz-calib_amd/host.
// --uncertainty (not in the reference) writes a side file <output>/<basename(images)>_uncertainty.json with the standard
// deviations of every registered view: the 2D-2D bundle adjustment over the registered views is solved once more from PTZ-IBA's
// cameras and PTZRayOptimizer::StdDevs is taken at its solution, the first seed image anchoring the gauge.  This is the
// uncertainty of the PTZ-IBA stage, rotations RELATIVE TO THE ANCHOR, before georeferencing; the main output file and the exit
// codes do not depend on the flag.  With -a the side file gains one key, "georeferenced": after the georeferencing bundle
// adjustment succeeds, PTZRayOptimizer::WorldStdDevs of THAT optimizer (no extra solve) -- the standard deviations of the cameras
// the tool writes, in the world frame, and of the rig's projection centre.
// --trim_px <px> (with --trim_sigma, default 3, and --trim_rounds, default 8; not in the reference) trims outlying observations in
// the solves whose cameras and sigmas the tool writes: the georeferencing bundle adjustment and the re-solve of --uncertainty run
// PTZRayOptimizer::SetTrimming (solve, residual report, one rejected observation per offending track, re-pack, solve again).  A side
// file <output>/<basename(images)>_residuals.json then holds the rounds, the last threshold, the observations removed and, per
// registered image, rms_px / max_px / n_obs / n_removed of the georeferencing fit.  Without the flag nothing changes.
// --match_descriptors (with --match_ratio, --match_min, --match_window, --save_matches; not in the reference) builds the match table
// from the descriptors of the feature files on the GPU (MatchDescriptors) instead of reading pairs_matches.txt: every pair (i, j),
// i != j, of the sorted file names; the blocks go through the same loader as a file's.  Without the flag nothing changes.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <unordered_set>
#include <vector>

#include "../host/data_io.h"
#include "../host/ptz_incremental_optimizer.h"
#include "../host/ptzray_optimizer.h"
#include "args.h"

using namespace ptzcalib;

struct TrimArgs {
  bool on = false;
  double px = 0, sigma = 3.0;
  int rounds = 8;
};

static bool RunPtzBA(const std::vector<std::string>& fnames, const std::vector<ImageFeatures>& features,
                     const std::vector<MatchesInfo>& matches_info, int max_iter, std::vector<Camera>& cameras,
                     std::unordered_set<long>& reg_image_ids, long* first_seed = nullptr)
{  // run_ptz_ba.cc:116-129
  cameras.clear();
  cameras.resize(fnames.size());
  PtzIncrementalOptimizer ptz_iba(features, matches_info, cameras, fnames, max_iter);
  reg_image_ids.clear();
  const bool ok = ptz_iba.Solve(cameras, reg_image_ids);
  if (first_seed) {  // the first image of the seed pair the registered set grew from
    *first_seed = -1;
    for (const PtzIncrementalOptimizer::Event& e : ptz_iba.events())
      if (e.kind == PtzIncrementalOptimizer::Event::kInitPair && e.success) *first_seed = e.a;
  }
  return ok;
}

// --uncertainty: standard deviations of the registered views at the solution of their 2D-2D bundle adjustment, into a side file.
// Never changes `cameras`; a failure here is reported and is not a failure of the tool.
static void Appendf(std::string& s, const char* fmt, ...)
{
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  s += buf;
}

// `body` (if given) receives the file's text up to, not including, the "\n}\n" that closes it: the georeferencing stage appends
// its key there.
static void WriteUncertainty(const std::vector<std::string>& fnames, const std::vector<ImageFeatures>& features,
                             const std::vector<MatchesInfo>& matches_info, const std::vector<Camera>& cameras,
                             const std::unordered_set<long>& reg_image_ids, long seed, int max_iter, const std::string& path,
                             std::string* body = nullptr, const TrimArgs& trim = TrimArgs())
{
  PTZRayOptimizer optimizer(features, matches_info, cameras, reg_image_ids, max_iter, PTZRay);  // the factor PTZ-IBA adjusts with
  if (trim.on) optimizer.SetTrimming(trim.px, trim.sigma, trim.rounds);
  std::vector<Camera> refined = cameras;
  std::vector<double> sd;
  double sigma0 = 0;
  if (seed < 0 || !reg_image_ids.count(seed)) seed = -1;
  if (!optimizer.Solve(refined) || !optimizer.StdDevs(sd, sigma0, seed)) {
    fprintf(stderr, "Uncertainty: not available (the bundle adjustment over the registered views or its covariance failed)\n");
    return;
  }
  const std::vector<long>& images = optimizer.packed().cam_image;
  const size_t nf = sd.size() / images.size();
  const long anchor = seed >= 0 ? seed : images.front();
  const double deg = 180.0 / 3.14159265358979323846;
  std::string text;
  Appendf(text, "{\n  \"sigma0\": %.17g,\n  \"anchor\": \"%s\",\n  \"images\": {\n", sigma0, fnames[anchor].c_str());
  for (size_t c = 0; c < images.size(); ++c) {
    const double* s = sd.data() + nf * c;
    Appendf(text, "    \"%s\": {\"sigma_f\": %.17g, \"sigma_rot_deg\": [%.17g, %.17g, %.17g]", fnames[images[c]].c_str(), s[0], s[1] * deg,
            s[2] * deg, s[3] * deg);
    if (nf == 5) Appendf(text, ", \"sigma_k1\": %.17g", s[4]);
    Appendf(text, "}%s\n", c + 1 < images.size() ? "," : "");
  }
  text += "  }";
  FILE* f = fopen(path.c_str(), "w");
  if (!f) { fprintf(stderr, "Uncertainty: cannot write %s\n", path.c_str()); return; }
  fprintf(f, "%s\n}\n", text.c_str());
  fclose(f);
  if (body) *body = text;
}

static bool RunGeoreferencing(const std::vector<ImageFeatures>& features, const std::vector<MatchesInfo>& matches_info,
                              const std::vector<std::vector<Point2f>>& pixels, const std::vector<std::vector<Point3d>>& pts3d,
                              const std::unordered_set<long>& cam_ids, int max_iter, bool has_dist, std::vector<Camera>& cameras,
                              double& error_2d2d, double& error_2d3d, const std::vector<std::string>* fnames = nullptr,
                              std::string* georef = nullptr, const TrimArgs& trim = TrimArgs(), const std::vector<std::string>* all_fnames = nullptr,
                              const std::string& residuals_path = std::string())
{  // run_ptz_ba.cc:131-154; fnames / georef (--uncertainty): the "georeferenced" record of the side file, empty if not available
  PTZRayOptimizer optimizer(features, matches_info, cameras, pixels, pts3d, cam_ids, max_iter, has_dist ? PTZRayDist : PTZRay);
  if (trim.on) optimizer.SetTrimming(trim.px, trim.sigma, trim.rounds);
  std::vector<std::vector<Ray>> rays;
  if (!optimizer.Solve(cameras, rays)) {
    error_2d2d = error_2d3d = -1;
    return false;
  }
  error_2d2d = optimizer.final_reproj_error_2d2d();
  error_2d3d = optimizer.final_reproj_error_2d3d();
  if (trim.on && all_fnames) {  // --trim_px: what was removed and how every registered image fits, into the side file
    std::vector<double> rms, mx;
    std::vector<int32_t> cnt;
    const std::vector<long>& images = optimizer.packed().cam_image;
    if (!optimizer.ViewResiduals(rms, mx, cnt)) fprintf(stderr, "Residuals: the residual report is not available\n");
    else {
      std::vector<long> removed(images.size(), 0);
      const std::vector<uint8_t>& kept = optimizer.kept();
      const std::vector<int32_t>& oc = optimizer.packed_obs_cam_before_trim();
      for (size_t a = 0; a < kept.size() && a < oc.size(); ++a)
        if (!kept[a]) ++removed[oc[a]];
      const ptz_trim_report& r = optimizer.trim_report();
      std::string t;
      Appendf(t, "{\n  \"rounds\": %d,\n  \"threshold\": %.17g,\n  \"observations_removed\": %lld,\n  \"rays_removed\": %d,\n", (int)r.rounds, r.threshold,
              (long long)r.n_obs_removed, (int)r.n_ray_removed);
      Appendf(t, "  \"rms_px_first\": %.17g,\n  \"rms_px_last\": %.17g,\n  \"flags\": %d,\n  \"images\": {\n", r.rms_first, r.rms_last, (int)r.flags);
      for (size_t c = 0; c < images.size(); ++c)
        Appendf(t, "    \"%s\": {\"rms_px\": %.17g, \"max_px\": %.17g, \"n_obs\": %d, \"n_removed\": %ld}%s\n", (*all_fnames)[images[c]].c_str(), rms[c], mx[c],
                (int)cnt[c], removed[c], c + 1 < images.size() ? "," : "");
      t += "  }\n}\n";
      FILE* f = fopen(residuals_path.c_str(), "w");
      if (!f) fprintf(stderr, "Residuals: cannot write %s\n", residuals_path.c_str());
      else { fputs(t.c_str(), f); fclose(f); }
    }
  }
  if (fnames && georef) {
    std::vector<double> sd;
    std::array<double, 3> sc, centre;
    std::array<double, 2> s0;
    if (!optimizer.WorldStdDevs(sd, sc, s0) || !optimizer.WorldCentre(centre)) {
      fprintf(stderr, "Uncertainty: the covariance of the georeferenced cameras is not available\n");
      return true;
    }
    const std::vector<long>& images = optimizer.packed().cam_image;
    const size_t nf = sd.size() / images.size();
    const double deg = 180.0 / 3.14159265358979323846;
    std::string& t = *georef;
    Appendf(t, "{\n    \"sigma0_features\": %.17g,\n    \"sigma0_annotations\": %.17g,\n", s0[0], s0[1]);
    Appendf(t, "    \"centre\": [%.17g, %.17g, %.17g],\n    \"sigma_centre\": [%.17g, %.17g, %.17g],\n    \"images\": {\n", centre[0], centre[1],
            centre[2], sc[0], sc[1], sc[2]);
    for (size_t c = 0; c < images.size(); ++c) {
      const double* s = sd.data() + nf * c;
      Appendf(t, "      \"%s\": {\"sigma_f\": %.17g, \"sigma_rot_deg\": [%.17g, %.17g, %.17g]", (*fnames)[images[c]].c_str(), s[0], s[1] * deg,
              s[2] * deg, s[3] * deg);
      if (nf == 5) Appendf(t, ", \"sigma_k1\": %.17g", s[4]);
      Appendf(t, "}%s\n", c + 1 < images.size() ? "," : "");
    }
    t += "    }\n  }";
  }
  return true;
}

int main(int argc, char** argv)
{
  ptzapp::Args parser;
  parser.Add("images", 'i', "Images directory", true);
  parser.Add("features", 'f', "Features and matches directory", true);
  parser.Add("annotation", 'a', "Annotation filepath", false);
  parser.Add("output", 'o', "Output directory", true);
  parser.AddFlag("dist", "Whether images have distortion");
  parser.AddFlag("gpu_homography", "Compute the pair homographies of the match table on the GPU (same results)");
  parser.AddFlag("inlier_matches", "Keep only the RANSAC inliers of every pair's homography (4 px) as the pair's matches");
  parser.Add("min_inliers", '\0', "With --inlier_matches: inliers a pair needs to keep any match (default 6, at least 4)", false);
  parser.AddFlag(ptzapp::kUncertaintyFlag, ptzapp::kBaUncertaintyHelp);
  parser.Add("trim_px", '\0', "Trim outlying observations in the georeferencing / uncertainty solves: threshold floor in pixels (off unless given)", false);
  parser.Add("trim_sigma", '\0', "With --trim_px: threshold = max(trim_px, trim_sigma * robust sigma) (default 3; 0: trim_px alone)", false);
  parser.Add("trim_rounds", '\0', "With --trim_px: solves at most (default 8)", false);
  parser.AddFlag("match_descriptors", "Build the match table from the descriptors of the feature files on the GPU; pairs_matches.txt is not read");
  parser.Add("match_ratio", '\0', "With --match_descriptors: Lowe's ratio (default 0.8; 0: no ratio test)", false);
  parser.Add("match_min", '\0', "With --match_descriptors: matches a pair needs to keep any (default 8)", false);
  parser.Add("match_window", '\0', "With --match_descriptors: only pairs of cyclic index distance <= k in the sorted file names (default: all)", false);
  parser.Add("save_matches", '\0', "With --match_descriptors: also write the matches to this file, in the format of pairs_matches.txt", false);
  parser.Add("match_guided", '\0', "With --match_descriptors: match every pair again within this many pixels of its RANSAC homography "
                                   "and keep these matches instead; a pair without a verified model keeps none (off unless given)", false);
  parser.AddFlag("guided_grid", "With --match_guided: run the guided pass through the grid-binned kernel (the same matches, the same output)");
  parser.ParseCheck(argc, argv);
  TrimArgs trim;
  if (parser.Exist("trim_px")) {
    trim.on = true;
    trim.px = atof(parser.Get("trim_px").c_str());
    if (parser.Exist("trim_sigma")) trim.sigma = atof(parser.Get("trim_sigma").c_str());
    if (parser.Exist("trim_rounds")) trim.rounds = atoi(parser.Get("trim_rounds").c_str());
    if (!(trim.px > 0.0) || !(trim.sigma >= 0.0) || trim.rounds < 1) {
      fprintf(stderr, "--trim_px must be positive, --trim_sigma not negative, --trim_rounds at least 1\n");
      return 1;
    }
  }
  const int min_inliers = parser.Exist("min_inliers") ? atoi(parser.Get("min_inliers").c_str()) : kDefaultMinInliers;
  if (min_inliers < 0) {
    fprintf(stderr, "--min_inliers must not be negative\n");
    return 1;
  }

  std::vector<std::string> fnames;
  std::vector<ImageFeatures> features;
  std::vector<Size> sizes;
  if (!LoadImgsAndFeatures(parser.Get("images"), parser.Get("features"), fnames, features, sizes)) {
    fprintf(stderr, "Error loading images and features. Exiting ...\n");
    return -1;
  }
  if (parser.Exist("match_guided") && !parser.Exist("match_descriptors")) {
    fprintf(stderr, "--match_guided needs --match_descriptors\n");
    return 1;
  }
  std::vector<MatchesInfo> matches_info;
  const std::string matches_path = parser.Get("features") + "/pairs_matches.txt";
  const bool gpu_h = parser.Exist("gpu_homography");
  bool loaded;
  if (parser.Exist("match_descriptors")) {
    // every unordered pair once on the device, (j, i) as its transpose; the blocks then go where a file's blocks go
    DescMatchOptions mo;
    if (parser.Exist("match_ratio")) mo.ratio = atof(parser.Get("match_ratio").c_str());
    if (parser.Exist("match_min")) mo.min_matches = atoi(parser.Get("match_min").c_str());
    const long n_img = static_cast<long>(fnames.size());
    const long window = parser.Exist("match_window") ? atol(parser.Get("match_window").c_str()) : n_img;
    if (!(mo.ratio >= 0.0) || !std::isfinite(mo.ratio) || mo.min_matches < 0 || window < 1) {
      fprintf(stderr, "--match_ratio must not be negative, --match_min not negative, --match_window at least 1\n");
      return 1;
    }
    if (parser.Exist("match_guided")) {
      mo.guided_radius = atof(parser.Get("match_guided").c_str());
      mo.min_inliers = min_inliers;
      mo.guided_grid = parser.Exist("guided_grid");
      if (!(mo.guided_radius > 0.0) || !std::isfinite(mo.guided_radius)) {
        fprintf(stderr, "--match_guided must be a positive number of pixels\n");
        return 1;
      }
    }
    std::vector<std::pair<long, long>> pairs;
    for (long i = 0; i < n_img; ++i)
      for (long j = i + 1; j < n_img; ++j)
        if (std::min(j - i, n_img - (j - i)) <= window) pairs.push_back({i, j});
    std::vector<std::vector<DMatch>> pairs_matches;
    std::vector<std::pair<std::string, std::string>> img_pairs_name;
    if (!MatchDescriptors(parser.Get("features"), fnames, parser.Get("features"), fnames, pairs, mo, true, pairs_matches, img_pairs_name)) {
      fprintf(stderr, "Error matching the descriptors of %s. Exiting ...\n", parser.Get("features").c_str());
      return -1;
    }
    if (parser.Exist("save_matches") && !WriteColmapMatches(parser.Get("save_matches"), pairs_matches, img_pairs_name)) {
      fprintf(stderr, "Error writing matches to %s. Exiting ...\n", parser.Get("save_matches").c_str());
      return -1;
    }
    loaded = LoadMatchesInfoFromBlocks(pairs_matches, img_pairs_name, fnames, features, matches_info, gpu_h ? 0 : -1, parser.Exist("inlier_matches"),
                                       min_inliers);
  }
  else
    loaded = parser.Exist("inlier_matches") ? LoadInlierMatchesInfo(matches_path, fnames, features, matches_info, gpu_h ? 0 : -1, min_inliers)
             : gpu_h                        ? LoadMatchesInfo(matches_path, fnames, features, matches_info, 0)
                                            : LoadMatchesInfo(matches_path, fnames, features, matches_info);
  if (!loaded) {
    if (parser.Exist("match_descriptors")) fprintf(stderr, "Error building the match table from the matched descriptors. Exiting ...\n");
    else fprintf(stderr, "Error loading matches from %s. Exiting ...\n", matches_path.c_str());
    return -1;
  }
  fprintf(stderr, "================== PTZ-IBA Begin ==========================\n");
  std::vector<Camera> cameras;
  std::unordered_set<long> reg_image_ids;
  static const int MAX_ITER = 200;
  long first_seed = -1;
  if (!RunPtzBA(fnames, features, matches_info, MAX_ITER, cameras, reg_image_ids, &first_seed)) {
    fprintf(stderr, "================== PTZ-IBA End: failed ==========================\n");
    return -1;
  }
  fprintf(stderr, "================== PTZ-IBA End: success ==========================\n");
  const bool uncertainty = parser.Exist(ptzapp::kUncertaintyFlag);
  const std::string side_path = parser.Get("output") + "/" + BaseName(parser.Get("images")) + "_uncertainty.json";
  std::string side_body;
  if (uncertainty || trim.on) MkdirIfNotExist(parser.Get("output"));
  if (uncertainty) {
    MkdirIfNotExist(parser.Get("output"));
    WriteUncertainty(fnames, features, matches_info, cameras, reg_image_ids, first_seed, MAX_ITER, side_path, &side_body, trim);
  }

  std::vector<std::vector<Point2f>> pixels;
  std::vector<std::vector<Point3d>> pts3d;
  if (!LoadAnnotation(parser.Get("annotation"), fnames, pixels, pts3d)) {
    fprintf(stderr, "Error loading annotation from %s. Exiting ...\n", parser.Get("annotation").c_str());
    return -1;
  }
  fprintf(stderr, "================== Georeferencing Begin ==========================\n");
  double error_2d2d, error_2d3d;
  std::string georef;
  if (!RunGeoreferencing(features, matches_info, pixels, pts3d, reg_image_ids, MAX_ITER, parser.Exist("dist"), cameras, error_2d2d, error_2d3d,
                         uncertainty ? &fnames : nullptr, uncertainty ? &georef : nullptr, trim, &fnames,
                         parser.Get("output") + "/" + BaseName(parser.Get("images")) + "_residuals.json")) {
    fprintf(stderr, "================== Georeferencing End: failed ==========================\n");
    return -1;
  }
  fprintf(stderr, "================== Georeferencing End: success ==========================\n");
  if (uncertainty && !georef.empty()) {  // the side file again, its earlier keys as they were, plus "georeferenced"
    FILE* f = fopen(side_path.c_str(), "w");
    if (!f) fprintf(stderr, "Uncertainty: cannot write %s\n", side_path.c_str());
    else {
      fprintf(f, "%s\n  \"georeferenced\": %s\n}\n", side_body.empty() ? "{" : (side_body + ",").c_str(), georef.c_str());
      fclose(f);
    }
  }

  const std::string cam_id = BaseName(parser.Get("images"));
  const std::string out_dir = parser.Get("output");
  MkdirIfNotExist(out_dir);
  const std::string out_path = out_dir + "/" + cam_id + ".json";
  SaveRegisteredCam(cameras, reg_image_ids, fnames, pixels, pts3d, out_path);

  fprintf(stderr, "================== Summary Begin ==========================\n");
  fprintf(stderr, "Registered/Total: %zu/%zu\n", reg_image_ids.size(), fnames.size());
  fprintf(stderr, "Error 2d-2d: %g\n", error_2d2d);
  fprintf(stderr, "Error 2d-3d: %g\n", error_2d3d);
  fprintf(stderr, "==================== Summary End ==========================\n");
  return 0;
}
