// krt_optimizer.h -- KRTOptimizer with the reference's public interface (src/core/krt_optimizer.h:108-145).
// Solve() hands the single-view problem to the MI355X library (ptz_krt_solve_batch with one query); the batched
// entry point is what relocalization over many queries should call directly.
#pragma once

#include <cstdint>
#include <vector>

#include "../../include/ptz_calib_amd.h"
#include "types.h"

namespace ptzcalib {

class KRTOptimizer {
 public:
  enum FACTOR_TYPE { F, FDist, Fxfy, FxfyDist };
  KRTOptimizer(int max_iter, double max_reproj_error, FACTOR_TYPE factor_type);
  void SetInitParams(const Mat33& K, const Mat33& R, const Vec3& t, const Vec5& dist);
  void Add2d2dConstraints(const Camera& cam_ref, const std::vector<KeyPoint>& kpts_ref, const std::vector<KeyPoint>& kpts_curr,
                          const std::vector<DMatch>& matches);
  void Add2d3dConstraints(const std::vector<Point2f>& pts2d, const std::vector<Point3d>& pts3d);
  bool Solve(Mat33& K, Mat33& R, Vec3& t, Vec5& dist);
  double Cal2d2dReprojError(const Camera& cam_ref, const std::vector<KeyPoint>& kpts_ref, const std::vector<KeyPoint>& kpts_curr,
                            const std::vector<DMatch>& matches);
  double Cal2d3dReprojError(const std::vector<Point2f>& pts2d, const std::vector<Point3d>& pts3d);
  // Covariance of the refined camera over the constraints this object holds (ptz_krt_covariance_batch with one query, a-posteriori
  // scale): cov = [NF x NF] row-major in the parameters [fx, (fy), d1, d2, d3, (k1)], NF = ptz_krt_free_dim(factor type), d a left
  // perturbation of the rotation in radians about the camera's own axes; sigma0 = the estimated pixel noise.  Valid after a Solve()
  // that returned true; false otherwise, without a device, or when the query's status is not PTZ_COV_OK (too few constraints,
  // a singular normal matrix).
  bool Covariance(std::vector<double>& cov, double& sigma0) const;
  // the square roots of its diagonal: focal length (fx) in pixels, rotation about x, y, z in radians
  bool StdDevs(double& sigma_f, double sigma_rot[3]) const;
  // Outlier trimming (ptz_krt_solve_batch_trimmed with one query): after SetTrimming, Solve() runs the solve / report / rule loop of
  // include/ptz_calib_amd.h over the 2D-2D matches and Covariance() is taken over the matches the last solve kept.  Never called:
  // Solve() is ptz_krt_solve_batch, as before.
  void SetTrimming(const ptz_krt_trim_options& trim) { trim_ = trim; trimming_ = true; }
  const ptz_krt_trim_report& trim_report() const { return trim_report_; }
  // After a Solve() that returned true: |e_m| of every match at the refined camera in the order of Add2d2dConstraints (-1: skipped by
  // the border guard; ptz_krt_residuals_batch) and the matches of the last solve (all 1 without trimming).  false otherwise.
  bool MatchResiduals(std::vector<double>& err_px, std::vector<uint8_t>& kept) const;
  // The gate in front of Solve() over the 2D-2D matches.  model 0: none, as before.  model 1: the rotation-and-focal gate
  // (ptz_rotfocal_gate_run with one query: `iters` two-match samples, 4 px, at least 6 inliers; the reference camera given to
  // Add2d2dConstraints is the anchor, the initial camera's principal point the query's centre) -- Solve() runs on the matches it keeps
  // (with trimming they are the loop's universe), returns false where it keeps none, and Covariance() / MatchResiduals() report the
  // kept set.  Any other model, or iters outside 1 .. 4096: false, nothing changed.
  bool SetGateModel(int model, int iters = 128);
  double gate_f() const { return gate_f_; }  // the gate's focal length of the last Solve() (0 without one)
  void SetFixedFocal() { set_fixed_focal_ = true; }  // a flag nobody reads, as in the reference (krt_optimizer.cc:502)
  int num_iter_ = 0;

  const ptz_lm_summary& summary() const { return summary_; }
  void SetDevice(int device_id) { device_id_ = device_id; }

 private:
  bool SolveGated(Mat33& K, Mat33& R, Vec3& t, Vec5& dist);
  Camera cam_curr_world_, cam_ref_;
  std::vector<float> uv_ref_, uv_cur_, pts2d_;
  std::vector<double> pts3d_;
  bool has_2d2d_ = false, set_fixed_focal_ = false, solved_ = false;
  FACTOR_TYPE factor_type_;
  int max_iter_;
  double max_reproj_error_;
  int device_id_ = 0;
  ptz_lm_summary summary_{};
  bool trimming_ = false;
  ptz_krt_trim_options trim_{};
  ptz_krt_trim_report trim_report_{};
  std::vector<uint8_t> kept_;  // of the last trimmed or gated Solve(); empty without either
  int gate_model_ = 0, gate_iters_ = 128;
  double gate_f_ = 0;
};

}  // namespace ptzcalib
