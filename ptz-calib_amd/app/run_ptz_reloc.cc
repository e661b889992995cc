// run_ptz_reloc -- relocalise test images against calibrated reference images; same options, inputs and output file as the
// reference tool (src/app/run_ptz_reloc.cc:23-148).  Where the reference runs one KRTOptimizer per test image in a loop
// (:68-118), this tool gathers every test image's problem and solves them all in ONE ptz_krt_solve_batch launch.
// --inlier_matches (not in the reference) solves on the RANSAC inliers of each query's matches: ptz_krt_solve_batch_gated.
// --uncertainty (not in the reference) adds the standard deviations of focal length and rotation to every registered image's
// record, from ONE ptz_krt_covariance_batch call over all test images.
// --trim_px <px> (not in the reference; with --trim_sigma, --trim_rounds) solves every test image with the outlier-trimming loop of
// ptz_krt_solve_batch_trimmed: with --inlier_matches the gate's inliers are the loop's universe, with --uncertainty the covariance is
// taken over the matches the last solve kept, and every record gains rms_px, n_matches, n_removed, trim_rounds.
// --shortlist R (not in the reference; with --shortlist_probes, --shortlist_min_votes; implies --on_device) matches every test image
// against the R reference images its probe features vote for instead of all of them (ptz_relocalizer_run_shortlisted); every record
// gains n_shortlist.
// --prior_params <json> (not in the reference; implies --on_device and --inlier_matches) relocalizes every test image that has a camera
// in that file from it (ptz_relocalizer_run_tracked: overlap list, guided matching under the predicted homography, no dense pass), in
// one run; the rest go through the path the other flags select.  --sequence takes the test images in name order, one run per frame: a
// frame after a registered one is tracked with that frame's camera as its prior, the first frame and any frame after a lost one run
// untracked (--shortlist if given, else all pairs), and a tracked frame that is lost is run again untracked -- one frame per run and
// therefore latency-bound.  --prior_radius, --prior_refs: the matcher's radius (40 px) and the list length (8).  Every record gains
// "tracked" and n_shortlist.
// --gate_model rotfocal [--gate_iters T] (not in the reference; needs --inlier_matches or a flag that implies it; implies --on_device) gates
// a test image's assembled matches with the two-point rotation-and-focal gate (ptz_relocalizer_set_gate_model) in the place of the
// homography gate, in whichever run the other flags select; the tracked runs' rule that half of a frame's guided matches lie on the
// gate's model then counts that gate's mask; every record gains gate_model and gate_f, the gate's focal length.
// --landmarks (not in the reference; with --landmark_min_views; implies --on_device) relocalizes against a landmark MAP instead of
// reference images: the reference images are matched among themselves (MatchDescriptors, --match_ratio and --match_min), the host
// TracksBuilder turns the matches into tracks as PTZRayOptimizer does, ptz_landmark_map_create makes one ray and one descriptor per
// track, and every test image goes through ptz_relocalizer_run_landmarks -- one (map, image) pair each.  Every record gains
// n_landmarks and n_matches.
// --landmark_prior_params <json> / --landmark_sequence (with --landmarks and --landmark_prior_radius; they imply --inlier_matches) are
// --prior_params / --sequence against the map: a test image with a prior camera goes through ptz_relocalizer_run_landmarks_tracked -- only
// the landmarks the prior sees are matched, around their predicted pixels -- and the untracked path is the dense landmark run.  Every
// record gains "tracked" and n_visible.
// --landmark_shortlist R (with --landmarks; takes --shortlist_probes and --shortlist_min_votes) sends every test image that has no prior
// -- all of them, the images without an entry in --landmark_prior_params, the untracked frames of --landmark_sequence -- through
// ptz_relocalizer_run_landmarks_shortlisted: its probe features vote for the map's homes and only the landmarks of the R listed homes
// are matched.  An image that run does not register is run once more against the whole map, so the fallback chain ends where it
// ends without the flag.  Every record gains n_shortlist and n_visible (both 0 for an image the dense run answered).
// --device_tracks (with --landmarks) keeps the map's tracks on the device: the references are matched among themselves by
// ptz_desc_match_pairs on the resident reference set, ptz_tracks_from_matches turns the resident table into tracks and
// ptz_landmark_map_create_from_tracks reads them where they lie -- no match, track or offset crosses the bus.  The landmarks are
// those of the host route in the order of their tracks' smallest features, so the records agree to rounding, not to the bit.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <unordered_set>
#include <utility>
#include <vector>

#include "../../include/ptz_calib_amd.h"
#include "../host/data_io.h"
#include "../host/json_mini.h"
#include "../host/tracks.h"
#include "args.h"

using namespace ptzcalib;

typedef std::pair<std::string, std::vector<DMatch>> BestMatchT;

// the reference image with the most matches towards this test image; the first one wins a tie (run_ptz_reloc.cc:150-170)
static BestMatchT FindBestMatch(const std::string& fname, const std::vector<std::pair<std::string, std::string>>& img_pairs_name,
                                const std::vector<std::vector<DMatch>>& pairs_matches)
{
  BestMatchT best;
  for (size_t i = 0; i < img_pairs_name.size(); ++i) {
    if (img_pairs_name[i].second != fname) continue;
    if (pairs_matches[i].size() > best.second.size()) best = {img_pairs_name[i].first, pairs_matches[i]};
  }
  return best;
}

// the descriptors of the feature files and the key points already loaded, as one resident set (image m: features ptr[m] .. ptr[m + 1])
static bool BuildDescSet(const std::string& dir, const std::vector<std::string>& fnames, const std::vector<ImageFeatures>& features,
                         ptz_desc_set** set)
{
  std::vector<unsigned char> all, one;
  std::vector<float> kp_xy;
  std::vector<int64_t> ptr(1, 0);
  int dim = 0;
  for (size_t i = 0; i < fnames.size(); ++i) {
    const std::string path = dir + "/" + fnames[i] + ".txt";
    if (!ReadColmapDescriptors(path, one, dim) || dim < 1 || one.size() / static_cast<size_t>(dim) != features[i].keypoints.size()) {
      fprintf(stderr, "Error reading the descriptors of %s (missing, of another dimension, or not one per key point)\n", path.c_str());
      return false;
    }
    all.insert(all.end(), one.begin(), one.end());
    for (const KeyPoint& k : features[i].keypoints) { kp_xy.push_back(k.pt.x); kp_xy.push_back(k.pt.y); }
    ptr.push_back(ptr.back() + static_cast<int64_t>(features[i].keypoints.size()));
  }
  const int32_t rc = ptz_desc_set_create(static_cast<int32_t>(fnames.size()), ptr.data(), all.data(), dim, kp_xy.data(), 0, set);
  if (rc != PTZ_OK) fprintf(stderr, "ptz_desc_set_create failed with status %d (no usable HIP device?)\n", rc);
  return rc == PTZ_OK;
}

int main(int argc, char** argv)
{
  ptzapp::Args parser;
  parser.Add("ref_images", '\0', "Reference images directory", true);
  parser.Add("ref_features", '\0', "Reference images features directory", true);
  parser.Add("ref_params", '\0', "Reference camera parameters filepath", true);
  parser.Add("test_images", '\0', "Test images directory", true);
  parser.Add("test_features", '\0', "Test images features and matches directory", true);
  parser.Add("output", '\0', "Output directory", true);
  parser.AddFlag("dist", "Whether images have distortion");
  parser.AddFlag("inlier_matches", "Solve each test image on the RANSAC inliers (homography, 4 px) of its matches; the reference image "
                                   "is still the one with the most raw matches");
  parser.Add("min_inliers", '\0', "With --inlier_matches: inliers a pair needs to keep any match (default 6, at least 4)", false);
  parser.AddFlag(ptzapp::kUncertaintyFlag, ptzapp::kUncertaintyHelp);
  parser.Add("trim_px", '\0', "Trim outlier matches: solve, measure every match with the fitted camera, drop those above "
                              "max(trim_px, trim_sigma * median / 1.1774) pixels, solve again, until nothing changes", false);
  parser.Add("trim_sigma", '\0', "With --trim_px: the threshold's multiple of the robust pixel noise (default 3, 0: trim_px alone)", false);
  parser.Add("trim_rounds", '\0', "With --trim_px: solves per test image at most (default 8)", false);
  parser.AddFlag("match_descriptors", "Match every test image against every reference image by the descriptors of the feature files, on "
                 "the GPU; pairs_matches.txt is not read");
  parser.Add("match_ratio", '\0', "With --match_descriptors: Lowe's ratio (default 0.8; 0: no ratio test)", false);
  parser.Add("match_min", '\0', "With --match_descriptors: matches a pair needs to keep any (default 8)", false);
  parser.Add("save_matches", '\0', "With --match_descriptors: also write the matches to this file, in the format of pairs_matches.txt", false);
  parser.Add("match_guided", '\0', "With --match_descriptors: match every pair again within this many pixels of its RANSAC homography "
                                   "and keep these matches instead; a pair without a verified model keeps none (off unless given)", false);
  parser.AddFlag("on_device", "With --match_descriptors: keep the match table on the GPU -- reference selection, the initial camera, the gate, "
                              "the solve and the covariance run there and only per-image results come back; the output is the same");
  parser.Add("multi_ref", '\0', "With --match_descriptors: solve each test image against its K best reference images at once (implies "
                                "--on_device); every record gains n_refs and n_matches", false);
  parser.Add("shortlist", '\0', "With --match_descriptors: match each test image against the R reference images that most of its probe "
                                "features vote for instead of all of them (implies --on_device); every record gains n_shortlist", false);
  parser.Add("shortlist_probes", '\0', "With --shortlist: features of a test image that vote (default 256)", false);
  parser.Add("shortlist_min_votes", '\0', "With --shortlist: votes a reference image needs to be listed (default 1)", false);
  parser.Add("prior_params", '\0', "With --match_descriptors: prior cameras of test images (a parameters file keyed by image name); an image "
                                   "with an entry is relocalized from it by guided matching alone (implies --on_device, --inlier_matches)", false);
  parser.AddFlag("sequence", "With --match_descriptors: the test images are frames in name order; a frame after a registered one is relocalized "
                             "from that frame's camera (implies --on_device, --inlier_matches)");
  parser.Add("prior_radius", '\0', "With --prior_params / --sequence: the guided matcher's radius in pixels (default 40)", false);
  parser.Add("prior_refs", '\0', "With --prior_params / --sequence: reference images a prior lists at most (default 8)", false);
  parser.AddFlag("guided_grid", "With --match_guided, --prior_params or --sequence: run the guided matcher through the grid-binned kernel "
                                "(the same matches, the same output)");
  parser.AddFlag("landmarks", "With --match_descriptors: relocalize every test image against a landmark map -- one ray and one descriptor per "
                              "track of the reference images -- instead of reference images (implies --on_device); every record gains "
                              "n_landmarks and n_matches");
  parser.Add("landmark_min_views", '\0', "With --landmarks: reference images a track needs to become a landmark (default 2; the tracks come from "
                                         "matches between reference images, so they have two views at least and 1 acts as 2)", false);
  parser.AddFlag("device_tracks", "With --landmarks: build the map's tracks on the device from the resident match table of the reference "
                                  "images (ptz_tracks_from_matches) instead of downloading it for the host TracksBuilder");
  parser.Add("landmark_prior_params", '\0', "With --landmarks: prior cameras of test images (a parameters file keyed by image name); an image "
                                            "with an entry is matched against the landmarks its prior sees only (implies --inlier_matches)", false);
  parser.AddFlag("landmark_sequence", "With --landmarks: the test images are frames in name order; a frame after a registered one is relocalized "
                                      "against the landmarks that frame's camera sees (implies --inlier_matches)");
  parser.Add("landmark_prior_radius", '\0', "With --landmark_prior_params / --landmark_sequence: the margin of the predicted view and the guided "
                                            "matcher's radius in pixels (default 40)", false);
  parser.Add("landmark_shortlist", '\0', "With --landmarks: match each test image without a prior against the landmarks of the R homes (cells "
                                         "of the map) that most of its probe features vote for; takes --shortlist_probes and "
                                         "--shortlist_min_votes; every record gains n_shortlist and n_visible", false);
  parser.Add("gate_model", '\0', "With --inlier_matches (or a flag that implies it): the model of the gate on a test image's assembled matches: "
                                 "homography (default) or rotfocal, the two-point rotation-and-focal gate (implies --on_device); with rotfocal "
                                 "every record gains gate_model and gate_f", false);
  parser.Add("gate_iters", '\0', "With --gate_model rotfocal: its samples, 1 .. 4096 (default 128)", false);
  parser.ParseCheck(argc, argv);
  const int min_inliers = parser.Exist("min_inliers") ? atoi(parser.Get("min_inliers").c_str()) : kDefaultMinInliers;
  if (min_inliers < 0) {
    fprintf(stderr, "--min_inliers must not be negative\n");
    return 1;
  }

  if (parser.Exist("match_guided") && !parser.Exist("match_descriptors")) {
    fprintf(stderr, "--match_guided needs --match_descriptors\n");
    return 1;
  }
  const int multi_ref = parser.Exist("multi_ref") ? atoi(parser.Get("multi_ref").c_str()) : 0;
  const bool shortlisting = parser.Exist("shortlist");
  const bool prior_file = parser.Exist("prior_params"), sequence = parser.Exist("sequence"), tracking = prior_file || sequence;
  const bool landmarks = parser.Exist("landmarks");
  const bool lm_prior_file = parser.Exist("landmark_prior_params"), lm_sequence = parser.Exist("landmark_sequence"),
             lm_tracking = lm_prior_file || lm_sequence;
  if (!landmarks && (lm_tracking || parser.Exist("landmark_prior_radius"))) {
    fprintf(stderr, "--landmark_prior_params, --landmark_sequence and --landmark_prior_radius need --landmarks\n");
    return 1;
  }
  const bool lm_shortlisting = parser.Exist("landmark_shortlist");
  if (!landmarks && lm_shortlisting) {
    fprintf(stderr, "--landmark_shortlist needs --landmarks\n");
    return 1;
  }
  if (!lm_tracking && parser.Exist("landmark_prior_radius")) {
    fprintf(stderr, "--landmark_prior_radius needs --landmark_prior_params or --landmark_sequence\n");
    return 1;
  }
  ptz_landmark_prior_options lpo;
  ptz_landmark_prior_options_default(&lpo);
  if (parser.Exist("landmark_prior_radius")) lpo.radius_px = atof(parser.Get("landmark_prior_radius").c_str());
  if (!(lpo.radius_px > 0.0) || !std::isfinite(lpo.radius_px)) {
    fprintf(stderr, "--landmark_prior_radius must be a positive number of pixels\n");
    return 1;
  }
  if (parser.Exist("gate_model") && parser.Get("gate_model") != "homography" && parser.Get("gate_model") != "rotfocal") {
    fprintf(stderr, "--gate_model is homography or rotfocal\n");
    return 1;
  }
  const bool rotfocal = parser.Exist("gate_model") && parser.Get("gate_model") == "rotfocal";
  if (rotfocal && !(parser.Exist("inlier_matches") || tracking || lm_tracking)) {
    fprintf(stderr, "--gate_model rotfocal needs --inlier_matches or a flag that implies it\n");
    return 1;
  }
  const int gate_iters = parser.Exist("gate_iters") ? atoi(parser.Get("gate_iters").c_str()) : 128;
  if (parser.Exist("gate_iters") && (!rotfocal || gate_iters < 1 || gate_iters > 4096)) {
    fprintf(stderr, "--gate_iters needs --gate_model rotfocal and is 1 .. 4096\n");
    return 1;
  }
  const bool on_device = parser.Exist("on_device") || parser.Exist("multi_ref") || shortlisting || tracking || landmarks || rotfocal;
  if (on_device && !parser.Exist("match_descriptors")) {
    fprintf(stderr, "--on_device, --multi_ref, --shortlist, --prior_params, --sequence, --landmarks and --gate_model rotfocal need "
                    "--match_descriptors\n");
    return 1;
  }
  if (landmarks && (parser.Exist("match_guided") || shortlisting || parser.Exist("multi_ref") || tracking || parser.Exist("save_matches"))) {
    fprintf(stderr, "--landmarks matches against the map, not against reference images: it does not go with --match_guided, --shortlist, "
                    "--multi_ref, --prior_params, --sequence or --save_matches\n");
    return 1;
  }
  if (!landmarks && parser.Exist("landmark_min_views")) {
    fprintf(stderr, "--landmark_min_views needs --landmarks\n");
    return 1;
  }
  const bool device_tracks = parser.Exist("device_tracks");
  if (!landmarks && device_tracks) {
    fprintf(stderr, "--device_tracks needs --landmarks\n");
    return 1;
  }
  const int landmark_min_views = parser.Exist("landmark_min_views") ? atoi(parser.Get("landmark_min_views").c_str()) : 2;
  if (landmark_min_views < 1) {
    fprintf(stderr, "--landmark_min_views must be at least 1\n");
    return 1;
  }
  ptz_prior_options po;
  ptz_prior_options_default(&po);
  if (!tracking && (parser.Exist("prior_radius") || parser.Exist("prior_refs"))) {
    fprintf(stderr, "--prior_radius and --prior_refs need --prior_params or --sequence\n");
    return 1;
  }
  if (parser.Exist("prior_radius")) po.radius_px = atof(parser.Get("prior_radius").c_str());
  if (parser.Exist("prior_refs")) po.max_refs = atoi(parser.Get("prior_refs").c_str());
  if (!(po.radius_px > 0.0) || !std::isfinite(po.radius_px) || po.max_refs < 1) {
    fprintf(stderr, "--prior_radius must be a positive number of pixels, --prior_refs at least 1\n");
    return 1;
  }
  ptz_shortlist_options sl;
  ptz_shortlist_options_default(&sl);
  if (!shortlisting && !lm_shortlisting && (parser.Exist("shortlist_probes") || parser.Exist("shortlist_min_votes"))) {
    fprintf(stderr, "--shortlist_probes and --shortlist_min_votes need --shortlist or --landmark_shortlist\n");
    return 1;
  }
  if (shortlisting || lm_shortlisting) {
    sl.max_refs = atoi(parser.Get(shortlisting ? "shortlist" : "landmark_shortlist").c_str());
    if (parser.Exist("shortlist_probes")) sl.n_probes = atoi(parser.Get("shortlist_probes").c_str());
    if (parser.Exist("shortlist_min_votes")) sl.min_votes = atoi(parser.Get("shortlist_min_votes").c_str());
    if (sl.max_refs < 1 || sl.n_probes < 1 || sl.min_votes < 0) {
      fprintf(stderr, "--shortlist, --landmark_shortlist and --shortlist_probes must be at least 1, --shortlist_min_votes not negative\n");
      return 1;
    }
  }
  if (parser.Exist("multi_ref") && multi_ref < 1) {
    fprintf(stderr, "--multi_ref must be at least 1\n");
    return 1;
  }
  const bool trimming = parser.Exist("trim_px");
  ptz_krt_trim_options trim;
  ptz_krt_trim_options_default(&trim);
  if (trimming) {
    trim.trim_px = atof(parser.Get("trim_px").c_str());
    if (parser.Exist("trim_sigma")) trim.k_sigma = atof(parser.Get("trim_sigma").c_str());
    if (parser.Exist("trim_rounds")) trim.max_rounds = atoi(parser.Get("trim_rounds").c_str());
    if (!(trim.trim_px > 0) || !(trim.k_sigma >= 0) || trim.max_rounds < 1 || trim.max_rounds > 64) {
      fprintf(stderr, "--trim_px must be positive, --trim_sigma not negative, --trim_rounds in 1 .. 64\n");
      return 1;
    }
  }

  std::vector<std::string> ref_fnames, test_fnames;
  std::vector<ImageFeatures> ref_features, test_features;
  std::vector<Size> ref_sizes, test_sizes;
  if (!LoadImgsAndFeatures(parser.Get("ref_images"), parser.Get("ref_features"), ref_fnames, ref_features, ref_sizes)) {
    fprintf(stderr, "Error loading reference images and features. Exiting ...\n");
    return -1;
  }
  if (!LoadImgsAndFeatures(parser.Get("test_images"), parser.Get("test_features"), test_fnames, test_features, test_sizes)) {
    fprintf(stderr, "Error loading test images and features. Exiting ...\n");
    return -1;
  }
  std::vector<std::vector<DMatch>> pairs_matches;
  std::vector<std::pair<std::string, std::string>> img_pairs_name;
  if (on_device) {
    // (the table stays on the GPU: below, once the reference cameras are read)
  }
  else if (parser.Exist("match_descriptors")) {
    // blocks test image by test image, the references in ref_fnames order: FindBestMatch's first-wins tie picks the lowest reference
    DescMatchOptions mo;
    if (parser.Exist("match_ratio")) mo.ratio = atof(parser.Get("match_ratio").c_str());
    if (parser.Exist("match_min")) mo.min_matches = atoi(parser.Get("match_min").c_str());
    if (!(mo.ratio >= 0.0) || !std::isfinite(mo.ratio) || mo.min_matches < 0) {
      fprintf(stderr, "--match_ratio and --match_min must not be negative\n");
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
    for (size_t t = 0; t < test_fnames.size(); ++t)
      for (size_t r = 0; r < ref_fnames.size(); ++r) pairs.push_back({static_cast<long>(r), static_cast<long>(t)});
    if (!MatchDescriptors(parser.Get("ref_features"), ref_fnames, parser.Get("test_features"), test_fnames, pairs, mo, false, pairs_matches,
                          img_pairs_name)) {
      fprintf(stderr, "Error matching the descriptors of the test images against the references. Exiting ...\n");
      return -1;
    }
    if (parser.Exist("save_matches") && !WriteColmapMatches(parser.Get("save_matches"), pairs_matches, img_pairs_name)) {
      fprintf(stderr, "Error writing matches to %s. Exiting ...\n", parser.Get("save_matches").c_str());
      return -1;
    }
  }
  else
    ReadColmapMatches(parser.Get("test_features") + "/pairs_matches.txt", pairs_matches, img_pairs_name);
  std::vector<Camera> ref_cameras;
  if (!ReadCamFromJson(parser.Get("ref_params"), ref_fnames, ref_cameras)) {
    fprintf(stderr, "Error loading reference camera parameters. Exiting ...\n");
    return -1;
  }

  // gather one query per test image that has a usable reference (run_ptz_reloc.cc:68-104)
  std::vector<size_t> query_image;
  std::vector<int64_t> match_ptr{0};
  std::vector<float> uv_ref, uv_cur;
  std::vector<double> cam_ref, cam_cur;
  for (size_t test_idx = 0; !on_device && test_idx < test_fnames.size(); ++test_idx) {
    const BestMatchT best = FindBestMatch(test_fnames[test_idx], img_pairs_name, pairs_matches);
    const long ref_idx = FindImgIndex(ref_fnames, best.first);
    bool usable = ref_idx != -1 && !best.second.empty();
    if (usable)
      for (const DMatch& m : best.second)
        usable &= m.queryIdx >= 0 && m.trainIdx >= 0 && static_cast<size_t>(m.queryIdx) < ref_features[ref_idx].keypoints.size() &&
                  static_cast<size_t>(m.trainIdx) < test_features[test_idx].keypoints.size();
    if (!usable) {
      fprintf(stderr, "Running ptz-reloc failed: %s\n", test_fnames[test_idx].c_str());
      continue;
    }
    const Camera& ref_cam = ref_cameras[ref_idx];
    const double f = ref_cam.K()[0];
    const double cx = 0.5 * test_sizes[test_idx].width, cy = 0.5 * test_sizes[test_idx].height;
    const Camera init(Mat33{f, 0, cx, 0, f, cy, 0, 0, 1}, ref_cam.R(), ref_cam.t(), ref_cam.dist());
    const std::vector<double> vr = ref_cam.ToVector(), vc = init.ToVector();
    cam_ref.insert(cam_ref.end(), vr.begin(), vr.end());
    cam_cur.insert(cam_cur.end(), vc.begin(), vc.end());
    for (const DMatch& m : best.second) {
      const Point2f a = ref_features[ref_idx].keypoints[m.queryIdx].pt, b = test_features[test_idx].keypoints[m.trainIdx].pt;
      uv_ref.push_back(a.x); uv_ref.push_back(a.y);
      uv_cur.push_back(b.x); uv_cur.push_back(b.y);
    }
    match_ptr.push_back(static_cast<int64_t>(uv_ref.size() / 2));
    query_image.push_back(test_idx);
  }

  std::vector<Camera> test_cameras(test_fnames.size());
  std::unordered_set<long> success_ids;
  const bool uncertainty = parser.Exist(ptzapp::kUncertaintyFlag);
  struct Sigma { bool ok = false; double f = 0, rot_deg[3] = {0, 0, 0}, s0 = 0; };
  std::vector<Sigma> sigmas(test_fnames.size());
  struct Trimmed { double rms = 0; int n_matches = 0, n_removed = 0, rounds = 0; };
  std::vector<Trimmed> trimmed(test_fnames.size());
  std::vector<int> multi_n_refs(test_fnames.size(), 0), multi_n_matches(test_fnames.size(), 0), n_shortlist(test_fnames.size(), 0);
  std::vector<int> tracked(test_fnames.size(), 0), n_visible(test_fnames.size(), 0);
  std::vector<double> gate_f(test_fnames.size(), 0.0);  // --gate_model rotfocal: the gate's focal length of a test image
  int n_landmarks = 0;
  if (on_device && !test_fnames.empty()) {
    // the same options as the host path reads them, handed to the resident loop (ptz_relocalizer_run): pass 1 over all pairs, the
    // guided pass, the assembly, the gate, the solve or the trimming loop, the covariance -- in the order of the code below
    ptz_reloc_options ro;
    ptz_reloc_options_default(&ro);
    const DescMatchOptions defaults;
    ro.match.ratio = parser.Exist("match_ratio") ? atof(parser.Get("match_ratio").c_str()) : defaults.ratio;
    ro.match.min_matches = parser.Exist("match_min") ? atoi(parser.Get("match_min").c_str()) : defaults.min_matches;
    if (!(ro.match.ratio >= 0.0) || !std::isfinite(ro.match.ratio) || ro.match.min_matches < 0) {
      fprintf(stderr, "--match_ratio and --match_min must not be negative\n");
      return 1;
    }
    if (parser.Exist("match_guided")) {
      ro.guided_radius = atof(parser.Get("match_guided").c_str());
      if (!(ro.guided_radius > 0.0) || !std::isfinite(ro.guided_radius)) {
        fprintf(stderr, "--match_guided must be a positive number of pixels\n");
        return 1;
      }
    }
    ro.guided_grid = parser.Exist("guided_grid") ? 1 : 0;
    ro.ransac_thresh = 4.0;  // LoadMatchesInfo's (data_io.cc:384)
    ro.min_inliers = min_inliers;
    ro.inlier_matches = (parser.Exist("inlier_matches") || tracking || lm_tracking) ? 1 : 0;
    ro.trim = trimming ? 1 : 0;
    ro.trim_options = trim;
    ro.uncertainty = uncertainty ? 1 : 0;
    ro.max_refs = multi_ref > 0 ? multi_ref : 1;
    ro.factor_type = parser.Exist("dist") ? PTZ_KRT_FDist : PTZ_KRT_F;
    ro.max_reproj_error = 100.0;
    ro.lm.max_num_iterations = 200;
    const int32_t n_ref = static_cast<int32_t>(ref_fnames.size()), K = ro.max_refs;
    const int32_t nf = ptz_krt_free_dim(ro.factor_type);
    const bool gated = ro.inlier_matches != 0;
    ptz_desc_set* ref_set = nullptr;
    ptz_relocalizer* rl = nullptr;
    std::vector<double> ref_cams;
    for (const Camera& c : ref_cameras) {
      const std::vector<double> v = c.ToVector();
      ref_cams.insert(ref_cams.end(), v.begin(), v.end());
    }
    bool ok = n_ref > 0 && static_cast<size_t>(n_ref) == ref_cameras.size() && BuildDescSet(parser.Get("ref_features"), ref_fnames, ref_features, &ref_set);
    int32_t rc = PTZ_OK;
    if (ok) rc = ptz_relocalizer_create(ref_set, ref_cams.data(), n_ref, 0, &rl);
    if (ok && rc == PTZ_OK && rotfocal) rc = ptz_relocalizer_set_gate_model(rl, 1, gate_iters);  // stage 4 of every run below
    ptz_landmark_map* lmap = nullptr;
    if (ok && rc == PTZ_OK && landmarks && device_tracks) {
      // the same pairs on the resident set, the table, the tracks and the map without leaving the device
      std::vector<int32_t> ia, ib;
      for (int32_t r = 0; r < n_ref; ++r)
        for (int32_t s = r + 1; s < n_ref; ++s) { ia.push_back(r); ib.push_back(s); }
      ptz_desc_options mo;
      ptz_desc_options_default(&mo);
      mo.ratio = ro.match.ratio;
      mo.min_matches = ro.match.min_matches;
      ptz_desc_matches* table = nullptr;
      ptz_tracks* tracks = nullptr;
      rc = ptz_desc_match_pairs(ref_set, ref_set, static_cast<int32_t>(ia.size()), ia.data(), ib.data(), &mo, &table);
      if (rc == PTZ_OK) rc = ptz_tracks_from_matches(ref_set, table, ia.data(), ib.data(), std::max(landmark_min_views, 2), &tracks);
      if (rc == PTZ_OK) rc = ptz_landmark_map_create_from_tracks(ref_set, ref_cams.data(), n_ref, tracks, ro.factor_type, landmark_min_views, &lmap);
      if (rc == PTZ_OK) fprintf(stderr, "Landmark map: %d landmarks from %zu tracks of %d reference images\n", ptz_landmark_map_n_landmarks(lmap),
                                static_cast<size_t>(ptz_tracks_n_tracks(tracks)), n_ref);
      ptz_tracks_destroy(tracks);
      ptz_desc_matches_destroy(table);
    }
    else if (ok && rc == PTZ_OK && landmarks) {
      // the references among themselves, every pair once; the tracks of those matches; one landmark per track
      DescMatchOptions mo;
      mo.ratio = ro.match.ratio;
      mo.min_matches = ro.match.min_matches;
      std::vector<std::pair<long, long>> pairs;
      for (long r = 0; r < n_ref; ++r)
        for (long s = r + 1; s < n_ref; ++s) pairs.push_back({r, s});
      std::vector<std::vector<DMatch>> ref_matches;
      std::vector<std::pair<std::string, std::string>> ref_pairs_name;
      ok = MatchDescriptors(parser.Get("ref_features"), ref_fnames, parser.Get("ref_features"), ref_fnames, pairs, mo, false, ref_matches,
                            ref_pairs_name);
      if (!ok) fprintf(stderr, "Error matching the descriptors of the reference images among themselves. Exiting ...\n");
      std::vector<MatchesInfo> infos(ref_matches.size());
      for (size_t i = 0; ok && i < ref_matches.size(); ++i) {
        infos[i].src_img_idx = FindImgIndex(ref_fnames, ref_pairs_name[i].first);
        infos[i].dst_img_idx = FindImgIndex(ref_fnames, ref_pairs_name[i].second);
        infos[i].matches = ref_matches[i];
      }
      if (ok) {
        TracksBuilder builder;
        builder.Build(infos);
        builder.Filter(std::max(landmark_min_views, 2));  // (a track of the builder has two views at least)
        std::vector<int> id, img, feat;
        std::vector<int64_t> ptr;
        builder.ExportFlat(id, ptr, img, feat);
        if (ptr.empty()) ptr.push_back(0);
        const std::vector<int32_t> timg(img.begin(), img.end()), tfeat(feat.begin(), feat.end());
        rc = ptz_landmark_map_create(ref_set, ref_cams.data(), n_ref, static_cast<int32_t>(ptr.size() - 1), ptr.data(), timg.data(), tfeat.data(),
                                     ro.factor_type, landmark_min_views, 0, &lmap);
        if (rc == PTZ_OK) fprintf(stderr, "Landmark map: %d landmarks from %zu tracks of %d reference images\n", ptz_landmark_map_n_landmarks(lmap),
                                  ptr.size() - 1, n_ref);
      }
    }

    // one run over the test images idx (in that order): tracked from priors [15 per image], or by the path the other flags select;
    // dense: against the whole map although --landmark_shortlist is given (the second run of an image the shortlisted one lost)
    const auto run_block = [&](const std::vector<size_t>& idx, const double* priors, bool dense) {
      const bool listing = lmap && lm_shortlisting && !priors && !dense;
      const int32_t nq = static_cast<int32_t>(idx.size());
      if (!ok || rc != PTZ_OK || nq == 0) return;
      std::vector<std::string> names;
      std::vector<ImageFeatures> feats;
      std::vector<int32_t> wh;
      for (const size_t i : idx) {
        names.push_back(test_fnames[i]);
        feats.push_back(test_features[i]);
        wh.push_back(test_sizes[i].width); wh.push_back(test_sizes[i].height);
      }
      ptz_desc_set* test_set = nullptr;
      ok = BuildDescSet(parser.Get("test_features"), names, feats, &test_set);
      if (!ok) return;
      std::vector<double> cam(15 * static_cast<size_t>(nq)), cov(static_cast<size_t>(nf) * nf * nq, 0.0), sigma0(nq, 0.0);
      std::vector<int32_t> accepted(nq, 0), n_sel(nq, 0), n_matches(nq, 0), n_inliers(nq, 0), status(nq, -1), sel_ref(static_cast<size_t>(K) * nq, -1);
      std::vector<ptz_lm_summary> summaries(nq);
      std::vector<ptz_krt_trim_report> reports(nq);
      ptz_reloc_result rr;
      rr.cam = cam.data(); rr.accepted = accepted.data(); rr.summaries = summaries.data(); rr.sel_ref = sel_ref.data(); rr.n_sel = n_sel.data();
      rr.n_matches = n_matches.data(); rr.n_inliers = n_inliers.data(); rr.trim_report = reports.data(); rr.cov = cov.data();
      rr.sigma0 = sigma0.data(); rr.cov_status = status.data();
      std::vector<int32_t> n_short(nq, priors || shortlisting || lm_shortlisting ? 0 : n_ref);
      ptz_shortlist_result sr;
      sr.shortlist = nullptr; sr.n_short = n_short.data(); sr.votes = nullptr; sr.shortlist_ms = 0;
      ptz_prior_result pr;
      pr.shortlist = nullptr; pr.n_short = n_short.data(); pr.overlap = nullptr; pr.prior_ms = 0;
      std::vector<int32_t> n_vis(nq, 0);
      ptz_landmark_view_result vr;
      vr.n_visible = n_vis.data(); vr.view_ms = 0;
      rc = lmap && priors ? ptz_relocalizer_run_landmarks_tracked(rl, lmap, test_set, nq, wh.data(), priors, &ro, &lpo, &rr, &vr)
           : listing ? ptz_relocalizer_run_landmarks_shortlisted(rl, lmap, test_set, nq, wh.data(), &ro, &sl, &rr, &sr, &vr)
           : lmap ? ptz_relocalizer_run_landmarks(rl, lmap, test_set, nq, wh.data(), &ro, &rr)
           : priors ? ptz_relocalizer_run_tracked(rl, test_set, nq, wh.data(), priors, &ro, &po, &rr, &pr)
           : shortlisting ? ptz_relocalizer_run_shortlisted(rl, test_set, nq, wh.data(), &ro, &sl, &rr, &sr)
                          : ptz_relocalizer_run(rl, test_set, nq, wh.data(), &ro, &rr);
      for (int32_t q = 0; q < nq; ++q) n_shortlist[idx[q]] = n_short[q];
      if (rc == PTZ_OK && rotfocal && gated) {
        std::vector<double> models(10 * static_cast<size_t>(nq), 0.0);
        rc = ptz_relocalizer_gate_models(rl, models.data(), nullptr);
        for (int32_t q = 0; rc == PTZ_OK && q < nq; ++q) gate_f[idx[q]] = models[10 * static_cast<size_t>(q)];
      }
      if (rc == PTZ_OK && parser.Exist("save_matches")) {
        // the table comes to the host once, for the file alone: blocks in the pairs' order, a pair without matches has none
        const ptz_desc_matches* t = ptz_relocalizer_table(rl);
        const size_t n = static_cast<size_t>(ptz_desc_matches_n_matches(t));
        // (the run's own pair list: every reference of every test image, or the listed ones)
        int32_t n_pair = 0;
        rc = ptz_relocalizer_pairs(rl, &n_pair, nullptr, nullptr);
        std::vector<int32_t> pair_ref(std::max<int32_t>(n_pair, 1));
        std::vector<int64_t> query_ptr(static_cast<size_t>(nq) + 1, 0);
        if (rc == PTZ_OK) rc = ptz_relocalizer_pairs(rl, nullptr, pair_ref.data(), query_ptr.data());
        std::vector<int64_t> mptr(static_cast<size_t>(n_pair) + 1, 0);
        std::vector<int32_t> qa(std::max<size_t>(n, 1)), tb(std::max<size_t>(n, 1));
        if (rc == PTZ_OK) rc = ptz_desc_matches_download(t, mptr.data(), qa.data(), tb.data(), nullptr, nullptr, nullptr);
        size_t pq = 0;  // the test image of pair p
        for (size_t p = 0; rc == PTZ_OK && p + 1 < mptr.size(); ++p) {
          while (static_cast<int64_t>(p) >= query_ptr[pq + 1]) ++pq;
          if (mptr[p + 1] == mptr[p]) continue;
          std::vector<DMatch> ms;
          for (int64_t k = mptr[p]; k < mptr[p + 1]; ++k) {
            DMatch m;
            m.queryIdx = qa[static_cast<size_t>(k)];
            m.trainIdx = tb[static_cast<size_t>(k)];
            ms.push_back(m);
          }
          pairs_matches.push_back(ms);
          img_pairs_name.push_back({ref_fnames[pair_ref[p]], names[pq]});
        }
      }
      ptz_desc_set_destroy(test_set);
      if (rc != PTZ_OK) return;
      for (int32_t q = 0; q < nq; ++q) {
        const size_t i = idx[q];
        tracked[i] = priors ? 1 : 0;
        n_visible[i] = n_vis[q];
        multi_n_refs[i] = n_sel[q];
        multi_n_matches[i] = n_matches[q];
        // a tracked frame must also have MOST of its guided matches on one homography: under a true prior nearly all are, while the lone
        // wrong candidates a wrong prior admits agree with some model in a dozen matches by chance (min_inliers alone lets those pass)
        const bool consistent = !priors || 2 * static_cast<int64_t>(n_inliers[q]) >= n_matches[q];
        if (n_sel[q] > 0 && accepted[q] && (!gated || n_inliers[q] > 0) && consistent) {
          test_cameras[i].FromVector(std::vector<double>(cam.begin() + 15 * q, cam.begin() + 15 * (q + 1)));
          success_ids.insert(static_cast<long>(i));
          fprintf(stderr, "Running ptz-reloc success: %s\n", test_fnames[i].c_str());
        }
        else fprintf(stderr, "Running ptz-reloc failed: %s\n", test_fnames[i].c_str());
        if (trimming) {
          Trimmed& t = trimmed[i];
          t.rms = reports[q].rms_last;
          t.n_matches = n_matches[q];
          t.n_removed = t.n_matches - reports[q].n_kept;
          t.rounds = reports[q].rounds;
        }
        sigmas[i] = Sigma();
        if (uncertainty && status[q] == PTZ_COV_OK) {
          Sigma& sg = sigmas[i];
          const double* c = cov.data() + static_cast<size_t>(nf) * nf * q;
          sg.ok = true;
          sg.f = std::sqrt(c[0]);
          for (int k = 0; k < 3; ++k) sg.rot_deg[k] = std::sqrt(c[(1 + k) * nf + 1 + k]) * 180.0 / M_PI;
          sg.s0 = sigma0[q];
        }
      }
    };

    // the images without a prior: by the path the flags select; with --landmark_shortlist the ones it loses once more, dense
    const auto run_untracked = [&](const std::vector<size_t>& idx) {
      run_block(idx, nullptr, false);
      if (!lm_shortlisting || !ok || rc != PTZ_OK) return;
      std::vector<size_t> lost;
      for (const size_t i : idx)
        if (!success_ids.count(static_cast<long>(i))) lost.push_back(i);
      run_block(lost, nullptr, true);
    };

    std::vector<size_t> all(test_fnames.size());
    for (size_t i = 0; i < all.size(); ++i) all[i] = i;
    if (sequence || lm_sequence) {
      // frame by frame: the camera of a registered frame is the next frame's prior; a lost tracked frame is run again untracked
      std::vector<double> prev;
      for (const size_t t : all) {
        const size_t mark = pairs_matches.size();
        if (!prev.empty()) {
          run_block({t}, prev.data(), false);
          if (ok && rc == PTZ_OK && !success_ids.count(static_cast<long>(t))) {
            pairs_matches.resize(mark);
            img_pairs_name.resize(mark);
            prev.clear();
          }
        }
        if (prev.empty()) run_untracked({t});
        prev = success_ids.count(static_cast<long>(t)) ? test_cameras[t].ToVector() : std::vector<double>();
      }
    }
    else if (prior_file || lm_prior_file) {
      const std::string prior_path = parser.Get(lm_prior_file ? "landmark_prior_params" : "prior_params");
      // one tracked run over the test images the file has a camera for, one run of the other flags' path over the rest
      std::vector<size_t> with, without;
      std::vector<double> priors;
      for (const size_t t : all) {
        std::vector<Camera> one;
        if (ReadCamFromJson(prior_path, {test_fnames[t]}, one)) {
          const std::vector<double> v = one[0].ToVector();
          priors.insert(priors.end(), v.begin(), v.end());
          with.push_back(t);
        }
        else without.push_back(t);
      }
      run_block(with, priors.data(), false);
      run_untracked(without);
    }
    else run_untracked(all);
    if (ok && rc == PTZ_OK && parser.Exist("save_matches") && !WriteColmapMatches(parser.Get("save_matches"), pairs_matches, img_pairs_name)) {
      fprintf(stderr, "Error writing matches to %s. Exiting ...\n", parser.Get("save_matches").c_str());
      ok = false;
    }
    n_landmarks = ptz_landmark_map_n_landmarks(lmap);
    ptz_relocalizer_destroy(rl);
    ptz_landmark_map_destroy(lmap);
    ptz_desc_set_destroy(ref_set);
    if (!ok) return -1;
    if (rc != PTZ_OK) {
      fprintf(stderr, "ptz_relocalizer_run failed with status %d (no usable HIP device?)\n", rc);
      return -1;
    }
  }
  if (!query_image.empty()) {
    static const int MAX_ITER = 200;
    static const double MAX_REPROJ_ERROR = 100.0;
    ptz_lm_options opt;
    ptz_lm_options_default(&opt);
    opt.max_num_iterations = MAX_ITER;
    const int32_t nq = static_cast<int32_t>(query_image.size());
    std::vector<ptz_lm_summary> summaries(nq);
    std::vector<int32_t> accepted(nq, 0);
    const int32_t type = parser.Exist("dist") ? PTZ_KRT_FDist : PTZ_KRT_F;
    static const double RANSAC_THRESH = 4.0;  // LoadMatchesInfo's (data_io.cc:384)
    const bool gated = parser.Exist("inlier_matches");
    std::vector<int32_t> n_inliers(nq, 0);
    std::vector<uint8_t> inlier_mask((gated && uncertainty) || trimming ? uv_ref.size() / 2 : 0);  // the covariance is over the matches a query kept
    std::vector<ptz_krt_trim_report> reports(trimming ? nq : 0);
    int32_t rc = PTZ_OK;
    if (trimming) {
      // the gate first: its kept set is the universe of the loop (a query that does not pass has an empty one)
      std::vector<uint8_t> universe;
      if (gated) {
        std::vector<double> H(9 * static_cast<size_t>(nq));
        std::vector<int32_t> found(nq, 0);
        universe.assign(uv_ref.size() / 2, 0);
        rc = ptz_homography_ransac_batch(nq, match_ptr.data(), uv_ref.data(), uv_cur.data(), RANSAC_THRESH, opt.device_id, H.data(), found.data(),
                                         universe.data(), nullptr);
        for (int32_t q = 0; q < nq && rc == PTZ_OK; ++q) {
          int32_t ones = 0;
          for (int64_t m = match_ptr[q]; m < match_ptr[q + 1]; ++m) ones += found[q] == 1 && universe[m] != 0;
          n_inliers[q] = (found[q] == 1 && ones >= (min_inliers > 4 ? min_inliers : 4)) ? ones : 0;
          if (n_inliers[q] == 0)
            for (int64_t m = match_ptr[q]; m < match_ptr[q + 1]; ++m) universe[m] = 0;
        }
      }
      if (rc == PTZ_OK)
        rc = ptz_krt_solve_batch_trimmed(nq, match_ptr.data(), uv_ref.data(), uv_cur.data(), nullptr, nullptr, nullptr, cam_ref.data(), cam_cur.data(),
                                         type, MAX_REPROJ_ERROR, gated ? universe.data() : nullptr, &trim, &opt, summaries.data(), accepted.data(),
                                         inlier_mask.data(), reports.data(), nullptr);
      for (int32_t q = 0; q < nq && rc == PTZ_OK; ++q) {
        Trimmed& t = trimmed[query_image[q]];
        t.rms = reports[q].rms_last;
        t.n_matches = static_cast<int>(match_ptr[q + 1] - match_ptr[q]);
        t.n_removed = t.n_matches - reports[q].n_kept;
        t.rounds = reports[q].rounds;
      }
    }
    else
      rc = gated ? ptz_krt_solve_batch_gated(nq, match_ptr.data(), uv_ref.data(), uv_cur.data(), cam_ref.data(), cam_cur.data(), type,
                                             MAX_REPROJ_ERROR, RANSAC_THRESH, min_inliers, &opt, summaries.data(), accepted.data(),
                                             n_inliers.data(), inlier_mask.empty() ? nullptr : inlier_mask.data(), nullptr, nullptr)
               : ptz_krt_solve_batch(nq, match_ptr.data(), uv_ref.data(), uv_cur.data(), cam_ref.data(), cam_cur.data(), type,
                                     MAX_REPROJ_ERROR, &opt, summaries.data(), accepted.data(), nullptr);
    if (rc != PTZ_OK) {
      fprintf(stderr, "ptz_krt_solve_batch failed with status %d (no usable HIP device?)\n", rc);
      return -1;
    }
    for (int32_t q = 0; q < nq; ++q) {
      const size_t test_idx = query_image[q];
      // (a query the gate left without matches is solved on nothing and comes back as it went in: not a relocalization)
      if (accepted[q] && (!gated || n_inliers[q] > 0)) {
        test_cameras[test_idx].FromVector(std::vector<double>(cam_cur.begin() + 15 * q, cam_cur.begin() + 15 * (q + 1)));
        success_ids.insert(static_cast<long>(test_idx));
        fprintf(stderr, "Running ptz-reloc success: %s\n", test_fnames[test_idx].c_str());
      }
      else fprintf(stderr, "Running ptz-reloc failed: %s\n", test_fnames[test_idx].c_str());
    }
    if (uncertainty) {
      const int32_t nf = ptz_krt_free_dim(type);  // [fx, d1, d2, d3, (k1)]
      std::vector<double> cov(static_cast<size_t>(nf) * nf * nq, 0.0), sigma0(nq, 0.0);
      std::vector<int32_t> status(nq, -1);
      const int32_t rc_cov = ptz_krt_covariance_batch(nq, match_ptr.data(), uv_ref.data(), uv_cur.data(), nullptr, nullptr, nullptr, cam_ref.data(),
                                                      cam_cur.data(), type, (gated || trimming) ? inlier_mask.data() : nullptr, accepted.data(), 0.0,
                                                      opt.device_id, cov.data(), sigma0.data(), status.data(), nullptr);
      if (rc_cov != PTZ_OK) {
        fprintf(stderr, "ptz_krt_covariance_batch failed with status %d\n", rc_cov);
        return -1;
      }
      for (int32_t q = 0; q < nq; ++q) {
        if (status[q] != PTZ_COV_OK) continue;
        Sigma& s = sigmas[query_image[q]];
        const double* c = cov.data() + static_cast<size_t>(nf) * nf * q;
        s.ok = true;
        s.f = std::sqrt(c[0]);
        for (int k = 0; k < 3; ++k) s.rot_deg[k] = std::sqrt(c[(1 + k) * nf + 1 + k]) * 180.0 / M_PI;
        s.s0 = sigma0[q];
      }
    }
  }

  const std::string cam_id = BaseName(parser.Get("test_images"));
  const std::string out_dir = parser.Get("output");
  MkdirIfNotExist(out_dir);
  std::vector<std::vector<Point2f>> pixels(test_fnames.size());
  std::vector<std::vector<Point3d>> pts3d(test_fnames.size());
  const std::string out_path = out_dir + "/" + cam_id + ".json";
  SaveRegisteredCam(test_cameras, success_ids, test_fnames, pixels, pts3d, out_path);
  if (uncertainty || trimming || multi_ref > 0 || shortlisting || tracking || landmarks || rotfocal) {
    // the keys go into the records SaveRegisteredCam wrote (the writer lays a parsed file out as it was: insertion order,
    // shortest round-trip numbers); a registered image whose covariance could not be computed keeps its record without them
    std::stringstream ss;
    {
      std::ifstream in(out_path);
      ss << in.rdbuf();
    }
    Json all;
    if (!Json::Parse(ss.str(), all) || !all.contains("cameras")) {
      fprintf(stderr, "Error reading back %s\n", out_path.c_str());
      return -1;
    }
    Json& cams = all["cameras"];
    for (size_t i = 0; i < test_fnames.size(); ++i) {
      if (!success_ids.count(static_cast<long>(i))) continue;
      std::string rootname, ext;
      SplitExt(test_fnames[i], &rootname, &ext);
      if (!cams.contains(rootname)) continue;
      Json& j = cams[rootname];
      if (multi_ref > 0) {
        j["n_refs"] = Json::Int(multi_n_refs[i]);
        if (!trimming) j["n_matches"] = Json::Int(multi_n_matches[i]);
      }
      if (landmarks) {
        j["n_landmarks"] = Json::Int(n_landmarks);
        if (!trimming) j["n_matches"] = Json::Int(multi_n_matches[i]);
      }
      if (shortlisting || tracking || lm_shortlisting) j["n_shortlist"] = Json::Int(n_shortlist[i]);
      if (tracking || lm_tracking) j["tracked"] = Json::Int(tracked[i]);
      if (lm_tracking || lm_shortlisting) j["n_visible"] = Json::Int(n_visible[i]);
      if (rotfocal) {
        j["gate_model"] = Json::String("rotfocal");
        j["gate_f"] = Json::Float(gate_f[i]);
      }
      if (trimming) {
        j["rms_px"] = Json::Float(trimmed[i].rms);
        j["n_matches"] = Json::Int(trimmed[i].n_matches);
        j["n_removed"] = Json::Int(trimmed[i].n_removed);
        j["trim_rounds"] = Json::Int(trimmed[i].rounds);
      }
      if (!uncertainty || !sigmas[i].ok) continue;
      j["sigma_f"] = Json::Float(sigmas[i].f);
      j["sigma_rot_deg"] = Json::FloatArray({sigmas[i].rot_deg[0], sigmas[i].rot_deg[1], sigmas[i].rot_deg[2]});
      j["sigma0"] = Json::Float(sigmas[i].s0);
    }
    std::ofstream fout(out_path, std::ios_base::out);
    if (!fout.good()) return -1;
    fout << all.dump(4) << std::endl;
  }
  return 0;
}
