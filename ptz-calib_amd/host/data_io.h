// data_io.h -- on-disk formats of the reference (src/core/data_io.h / data_io.cc) without OpenCV / nlohmann:
//   * COLMAP text features  "N D\n x y scale ori d0 .. d(D-1)\n ..."                     (data_io.cc:24-52)
//   * pairs_matches.txt      blocks "nameA nameB\n i j\n ...\n<blank line>"                 (data_io.cc:64-110)
//   * camera / annotation JSON  {"cameras": {name: {name,pos,res,K,R,t,dist,distType,marker{pix,pos},version}}} (:112-295)
//   * image directory listing with sizes read from the file headers                       (data_io.cc:294-333)
//   * the N x N MatchesInfo table with one RANSAC homography per listed pair              (data_io.cc:336-400),
//     on the host or, batched over the pairs, on the device
#pragma once

#include <string>
#include <unordered_set>
#include <utility>
#include <vector>

#include "types.h"

namespace ptzcalib {

void ReadColmapFeatures(const std::string& filepath, std::vector<KeyPoint>& kpts);
void ReadColmapMatches(const std::string& filepath, std::vector<std::vector<DMatch>>& pairs_matches,
                       std::vector<std::pair<std::string, std::string>>& img_pairs_name);
// The uint8 descriptors behind the key points of a COLMAP text feature file, [n, dim] row-major.  A file whose values are all
// integers in 0 .. 255 is taken as it is; any other (unit-norm float descriptors) is quantised as clamp(rint(128 + 127 v), 0, 255),
// with one warning on stderr per run.  dim: 0 on entry takes the file's, otherwise the file's must equal it.  false: no file, a
// short file, or a dimension mismatch.
bool ReadColmapDescriptors(const std::string& filepath, std::vector<unsigned char>& desc, int& dim);
// The inverse of ReadColmapMatches: a block "name_a name_b", its "queryIdx trainIdx" lines, a blank line -- after the last block too.
bool WriteColmapMatches(const std::string& filepath, const std::vector<std::vector<DMatch>>& pairs_matches,
                        const std::vector<std::pair<std::string, std::string>>& img_pairs_name);
// The descriptor matcher on device `device_id` (ptz_desc_match_pairs): fills what ReadColmapMatches fills.  Pair p matches image
// pairs[p].first of (dir_a, fnames_a) with image pairs[p].second of (dir_b, fnames_b); queryIdx is the feature of the first image,
// trainIdx that of the second; blocks come in the pairs' order and a pair without matches has no block, as in a file.
// transpose_back: also emit every pair's (second, first) block -- its matches swapped and sorted by the feature of the second
// image (the matcher's (B, A) result: the rule is symmetric under cross_check) -- and put all blocks in table order (first image,
// then second); needs dir_a == dir_b.
// guided_radius > 0: a second, homography-guided pass (ptz_desc_match_pairs_guided) for texture that repeats.  The first pass's
// pixel pairs go through ptz_homography_ransac_batch (ransac_thresh); a pair with a model and at least max(min_inliers, 4) mask-1
// matches is matched again over the candidates within guided_radius pixels of where its H puts the feature, and these matches
// REPLACE the pair's; a pair without such a model keeps none (the gate's rule: a first-pass pair no model verified is where the
// wrong matches live).  The feature files' key points are then loaded with the descriptors.
struct DescMatchOptions {
  double ratio = 0.8;
  int min_matches = 8;
  int device_id = 0;
  double guided_radius = 0.0;  // pixels; 0: off
  double ransac_thresh = 4.0;
  int min_inliers = 6;         // kDefaultMinInliers
  bool guided_grid = false;    // the guided pass through ptz_desc_match_pairs_guided_grid: the same matches
};
bool MatchDescriptors(const std::string& dir_a, const std::vector<std::string>& fnames_a, const std::string& dir_b,
                      const std::vector<std::string>& fnames_b, const std::vector<std::pair<long, long>>& pairs, const DescMatchOptions& options,
                      bool transpose_back, std::vector<std::vector<DMatch>>& pairs_matches,
                      std::vector<std::pair<std::string, std::string>>& img_pairs_name);
// LoadMatchesInfo / LoadInlierMatchesInfo on blocks already in memory (what they read from matches_path): device_id < 0: the host
// estimator; inliers: the gated table.
bool LoadMatchesInfoFromBlocks(const std::vector<std::vector<DMatch>>& pairs_matches,
                               const std::vector<std::pair<std::string, std::string>>& img_pairs_name, const std::vector<std::string>& fnames,
                               const std::vector<ImageFeatures>& features, std::vector<MatchesInfo>& matches_info, int device_id, bool inliers,
                               int min_inliers);
bool SaveToJson(const std::vector<Camera>& cameras, const std::vector<std::string>& names,
                const std::vector<std::vector<Point2f>>& pixels_gt, const std::vector<std::vector<Point3d>>& pts3d_gt,
                const std::string& filepath);
bool ReadFromJson(const std::string& filepath, std::vector<Camera>& cameras, std::vector<std::string>& names,
                  std::vector<std::vector<Point2f>>& pixels, std::vector<std::vector<Point3d>>& pts3d, std::vector<Size>& sizes);
bool ReadCamFromJson(const std::string& filepath, const std::vector<std::string>& names, std::vector<Camera>& cameras);
bool LoadImgsAndFeatures(const std::string& img_dir, const std::string& feature_dir, std::vector<std::string>& fnames,
                         std::vector<ImageFeatures>& features, std::vector<Size>& sizes);
bool LoadMatchesInfo(const std::string& matches_path, const std::vector<std::string>& fnames, const std::vector<ImageFeatures>& features,
                     std::vector<MatchesInfo>& matches_info);
// The same table with the pair homographies computed on device `device_id` in one call (ptz_homography_ransac_batch): the same
// pairs skipped, the same fields, the same bits.  Returns false (after a message on stderr) if the device call fails.
bool LoadMatchesInfo(const std::string& matches_path, const std::vector<std::string>& fnames, const std::vector<ImageFeatures>& features,
                     std::vector<MatchesInfo>& matches_info, int device_id);
// The inlier-gated table: the reference drops the mask cv::findHomography returns (data_io.cc:351-352) and hands every listed
// match on; here a cell's `matches` are the matches with mask byte 1 of the pair's RANSAC homography, in their order, if the
// pair has a model and at least max(min_inliers, 4) of them, and none otherwise.  (Four matches fit a homography exactly: a
// model with four inliers is verified by nothing.  kDefaultMinInliers is what the tools ask for.)  inliers_mask (all ones), num_inliers and confidence follow
// the kept matches; H, H_empty and the image indices are those of the ungated loader, computed on ALL matches.  Whatever
// reads `matches` (the track builder, the resident tables, CalPixelDiff, the rankings) then sees inliers only.
// device_id < 0: the host estimator; otherwise the pair estimator runs on that device.  Both give the same table.
bool LoadInlierMatchesInfo(const std::string& matches_path, const std::vector<std::string>& fnames, const std::vector<ImageFeatures>& features,
                           std::vector<MatchesInfo>& matches_info, int device_id = -1, int min_inliers = 0);
// cv::detail::BestOf2NearestMatcher's num_matches_thresh2: the inliers OpenCV's stitching matcher wants before it trusts a pair
static const int kDefaultMinInliers = 6;
bool LoadAnnotation(const std::string& annot_path, const std::vector<std::string>& fnames, std::vector<std::vector<Point2f>>& pixels,
                    std::vector<std::vector<Point3d>>& pts3d);
void SaveRegisteredCam(const std::vector<Camera>& cameras, const std::unordered_set<long>& reg_image_ids,
                       const std::vector<std::string>& fnames, const std::vector<std::vector<Point2f>>& pixels,
                       const std::vector<std::vector<Point3d>>& pts3d, const std::string& out_path);
long FindImgIndex(const std::vector<std::string>& fnames, const std::string& fname);

// path helpers with the semantics of the reference's utils/os_path.cc
std::string BaseName(const std::string& path);                                      // text after the last / or \ ("" for "dir/")
void SplitExt(const std::string& path, std::string* root, std::string* ext);         // ext keeps its dot and its case
bool MkdirIfNotExist(const std::string& dir);
std::vector<std::string> ListDir(const std::string& dir);                            // full paths, unsorted

}  // namespace ptzcalib
