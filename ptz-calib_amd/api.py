"""ctypes binding of include/ptz_calib_amd.h (libptzcalib_hip.so).

No compute happens in Python and there is no CPU fallback: if the HIP library is missing or no device is
present, every compute call raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PTZCALIB_LIB", os.path.join(_HERE, "libptzcalib_hip.so"))  # override: A/B probe builds only

CONVERGENCE, NO_CONVERGENCE, FAILURE = 0, 1, 2
BA_PTZRay, BA_PTZRayDist, BA_PTZRayFxfyDist, BA_PTZRayDistDisp = 0, 1, 2, 3
KRT_F, KRT_FDist, KRT_Fxfy, KRT_FxfyDist = 0, 1, 2, 3
COV_OK, COV_DOF, COV_SINGULAR, COV_SKIPPED = 0, 1, 2, 3
PROF_SLOTS = 16
_ERR = {-1: "PTZ_EINVAL", -2: "PTZ_ENODEVICE", -3: "PTZ_ENOMEM", -4: "PTZ_EUNSUPPORTED", -5: "PTZ_ELIMIT", -6: "PTZ_ENOOBS",
        -7: "PTZ_EINTERNAL"}

EXPORTS = ["ptz_lm_options_default", "ptz_version", "ptz_device_count", "ptz_ba_batch_create", "ptz_ba_batch_destroy",
           "ptz_ba_batch_set_state", "ptz_ba_batch_solve", "ptz_ba_batch_get_state", "ptz_ba_batch_last_solve_ms",
           "ptz_ba_batch_set_profiling", "ptz_ba_batch_get_profile", "ptz_ba_solve", "ptz_ba_cam_block_dim",
           "ptz_ba_batch_linearize", "ptz_ba_batch_pix2ray", "ptz_ba_batch_cam_block_dim", "ptz_chol_solve_batch", "ptz_krt_solve_batch",
           "ptz_krt_solve_batch_2d3d", "ptz_krt_solve_batch_device", "ptz_trim_cache", "ptz_mfma_f64_peak", "ptz_ba_solve_sharded",
           "ptz_krt_solve_batch_sharded", "ptz_hbm_bandwidth", "ptz_ba_batch_set_disp", "ptz_ba_batch_get_disp", "ptz_ba_solve_disp",
           "ptz_ba_plan_tile_order", "ptz_rig_create", "ptz_rig_destroy", "ptz_ba_batch_create_views", "ptz_ba_batch_set_state_pix2ray",
           "ptz_debug_batch_structure_hash", "ptz_debug_batch_initial_rays", "ptz_krt_table_create", "ptz_krt_table_destroy",
           "ptz_krt_solve_attempts", "ptz_homography_ransac_batch", "ptz_debug_homography_bounds", "ptz_match_gate_create",
           "ptz_match_gate_destroy", "ptz_match_gate_run_device", "ptz_match_gate_run", "ptz_krt_solve_batch_gated", "ptz_debug_match_gate_table",
           "ptz_krt_free_dim", "ptz_krt_covariance_batch", "ptz_krt_covariance_batch_device", "ptz_ba_cov_dim",
           "ptz_ba_batch_covariance", "ptz_ba_covariance", "ptz_ba_geo_cov_dim", "ptz_ba_batch_covariance_georef",
           "ptz_ba_covariance_georef", "ptz_ba_batch_residuals", "ptz_ba_batch_trim_select", "ptz_ba_problem_trim",
           "ptz_trim_options_default", "ptz_ba_solve_trimmed_batch", "ptz_ba_solve_trimmed", "ptz_krt_residuals_batch",
           "ptz_krt_residuals_batch_device", "ptz_krt_trim_options_default", "ptz_krt_trim_workspace_bytes", "ptz_krt_solve_batch_trimmed",
           "ptz_krt_solve_batch_trimmed_device", "ptz_desc_options_default", "ptz_desc_set_create", "ptz_desc_set_destroy",
           "ptz_desc_match_pairs", "ptz_desc_matches_n_matches", "ptz_desc_matches_n_pairs", "ptz_desc_matches_device_ms",
           "ptz_desc_matches_n_chunks", "ptz_desc_matches_download", "ptz_desc_matches_device_ptrs", "ptz_desc_matches_destroy",
           "ptz_debug_desc_dist2", "ptz_desc_match_pairs_guided", "ptz_desc_match_pairs_guided_device",
           "ptz_desc_match_pairs_guided_grid", "ptz_desc_match_pairs_guided_grid_device", "ptz_reloc_ref_rotations",
           "ptz_reloc_assemble_workspace_bytes", "ptz_reloc_assemble_device", "ptz_reloc_assemble", "ptz_reloc_options_default",
           "ptz_relocalizer_create", "ptz_relocalizer_destroy", "ptz_relocalizer_run", "ptz_relocalizer_n_matches", "ptz_relocalizer_matches", "ptz_relocalizer_table",
           "ptz_shortlist_options_default", "ptz_desc_shortlist", "ptz_desc_shortlist_workspace_bytes", "ptz_desc_shortlist_device",
           "ptz_relocalizer_run_shortlisted", "ptz_relocalizer_pairs", "ptz_debug_chol_solve", "ptz_prior_options_default",
           "ptz_reloc_prior_pairs", "ptz_reloc_prior_pairs_device", "ptz_relocalizer_run_tracked", "ptz_landmark_map_create",
           "ptz_landmark_map_destroy", "ptz_landmark_map_n_landmarks", "ptz_landmark_map_build_ms", "ptz_landmark_map_download",
           "ptz_landmark_map_desc_set", "ptz_landmark_assemble_workspace_bytes", "ptz_landmark_assemble", "ptz_landmark_assemble_device",
           "ptz_relocalizer_run_landmarks", "ptz_landmark_prior_options_default", "ptz_landmark_visible", "ptz_landmark_view_destroy",
           "ptz_landmark_view_n_visible", "ptz_landmark_view_download", "ptz_landmark_view_desc_set", "ptz_landmark_view_device_ptrs",
           "ptz_landmark_view_device_ms", "ptz_landmark_visible_workspace_bytes", "ptz_landmark_visible_device",
           "ptz_relocalizer_run_landmarks_tracked", "ptz_relocalizer_view", "ptz_landmark_map_home_set", "ptz_landmark_map_home_groups",
           "ptz_landmark_shortlist", "ptz_landmark_shortlist_workspace_bytes", "ptz_landmark_shortlist_device", "ptz_landmark_view_from_homes",
           "ptz_landmark_view_from_homes_device", "ptz_landmark_view_kind", "ptz_relocalizer_run_landmarks_shortlisted",
           "ptz_debug_batch_reduced_system", "ptz_rotfocal_gate_create", "ptz_rotfocal_gate_destroy", "ptz_rotfocal_gate_run_device",
           "ptz_rotfocal_gate_run", "ptz_relocalizer_gate_models", "ptz_relocalizer_set_gate_model", "ptz_tracks_build",
           "ptz_tracks_from_matches", "ptz_tracks_workspace_bytes", "ptz_tracks_build_device", "ptz_tracks_destroy", "ptz_tracks_n_tracks",
           "ptz_tracks_n_views", "ptz_tracks_counts", "ptz_tracks_download", "ptz_tracks_device_ptrs", "ptz_tracks_device_ms",
           "ptz_landmark_map_create_from_tracks"]


class PtzError(RuntimeError):
    def __init__(self, code, where):
        super().__init__(f"{where}: {_ERR.get(code, code)}")
        self.code = code


class LmOptions(C.Structure):
    _fields_ = [("max_num_iterations", C.c_int32), ("device_id", C.c_int32),
                ("max_num_consecutive_invalid_steps", C.c_int32), ("jacobi_scaling", C.c_int32),
                ("initial_trust_region_radius", C.c_double), ("max_trust_region_radius", C.c_double),
                ("min_trust_region_radius", C.c_double), ("min_relative_decrease", C.c_double),
                ("min_lm_diagonal", C.c_double), ("max_lm_diagonal", C.c_double), ("function_tolerance", C.c_double),
                ("gradient_tolerance", C.c_double), ("parameter_tolerance", C.c_double),
                ("krt_lanes_per_query", C.c_int32), ("reserved_", C.c_int32)]


class LmSummary(C.Structure):
    _fields_ = [("termination_type", C.c_int32), ("num_iterations", C.c_int32), ("num_lm_steps", C.c_int32),
                ("num_successful_steps", C.c_int32), ("num_unsuccessful_steps", C.c_int32),
                ("num_residuals", C.c_int32), ("num_linear_solves", C.c_int32), ("num_jacobian_evals", C.c_int32),
                ("initial_cost", C.c_double), ("final_cost", C.c_double), ("final_radius", C.c_double),
                ("final_gradient_max_norm", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class BaProblem(C.Structure):
    _fields_ = [("n_cam", C.c_int32), ("n_ray", C.c_int32), ("n_obs", C.c_int64), ("obs_uv", C.c_void_p),
                ("obs_cam", C.c_void_p), ("obs_ray", C.c_void_p), ("ray_weight", C.c_void_p),
                ("n_obs3d", C.c_int32), ("obs3d_uv", C.c_void_p), ("obs3d_xyz", C.c_void_p),
                ("obs3d_cam", C.c_void_p), ("factor_type", C.c_int32), ("ic_of_cam", C.c_void_p)]


class TrimOptions(C.Structure):
    _fields_ = [("trim_px", C.c_double), ("k_sigma", C.c_double), ("max_rounds", C.c_int32), ("reserved_", C.c_int32)]


class TrimReport(C.Structure):
    _fields_ = [("rounds", C.c_int32), ("flags", C.c_int32), ("n_obs_removed", C.c_int64), ("n_ray_removed", C.c_int32),
                ("reserved_", C.c_int32), ("threshold", C.c_double), ("rms_first", C.c_double), ("rms_last", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved_"}


TRIM_ENOOBS, TRIM_MAX_ROUNDS = 1, 2


class KrtTrimOptions(C.Structure):
    _fields_ = [("trim_px", C.c_double), ("k_sigma", C.c_double), ("max_rounds", C.c_int32), ("min_keep", C.c_int32)]


class KrtTrimReport(C.Structure):
    _fields_ = [("rounds", C.c_int32), ("flags", C.c_int32), ("n_removed", C.c_int32), ("n_kept", C.c_int32),
                ("threshold", C.c_double), ("rms_first", C.c_double), ("rms_last", C.c_double), ("median_last", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


KRT_TRIM_MIN_KEEP, KRT_TRIM_REJECTED = 4, 8
KRT_OPEN_BOUND = 1e300  # the error bound of the trimmed solve's rounds

_lib = None


def lib():
    """Load the HIP library; fails loudly if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950)")
        _lib = C.CDLL(LIB_PATH)
        _lib.ptz_version.restype = C.c_char_p
        _lib.ptz_device_count.restype = C.c_int32
        _lib.ptz_ba_cam_block_dim.restype = C.c_int32
        _lib.ptz_krt_free_dim.restype = C.c_int32
        _lib.ptz_ba_cov_dim.restype = C.c_int32
        _lib.ptz_ba_geo_cov_dim.restype = C.c_int32
        _lib.ptz_krt_trim_workspace_bytes.restype = C.c_int64
        _lib.ptz_krt_trim_workspace_bytes.argtypes = [C.c_int32, C.c_int64]
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _check(rc, where):
    if rc != 0:
        raise PtzError(rc, where)


def version() -> str:
    return lib().ptz_version().decode()


def trim_cache() -> None:
    """Give the library's parked device blocks / streams / events back to the driver (ptz_trim_cache)."""
    lib().ptz_trim_cache()


def device_count() -> int:
    return int(lib().ptz_device_count())


def default_options(**kw) -> LmOptions:
    o = LmOptions()
    lib().ptz_lm_options_default(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _pack_problem(sc, keep):
    arrs = dict(uv=np.ascontiguousarray(sc.obs_uv, dtype=np.float32), cam=np.ascontiguousarray(sc.obs_cam, dtype=np.int32),
                ray=np.ascontiguousarray(sc.obs_ray, dtype=np.int32), w=np.ascontiguousarray(sc.ray_weight, dtype=np.float64))
    keep.append(arrs)
    p = BaProblem()
    p.n_cam, p.n_ray, p.n_obs = sc.n_cam, sc.n_ray, len(arrs["cam"])
    p.obs_uv, p.obs_cam, p.obs_ray, p.ray_weight = _p(arrs["uv"]), _p(arrs["cam"]), _p(arrs["ray"]), _p(arrs["w"])
    o3 = getattr(sc, "obs3d", None)
    if o3 is not None and len(o3["cam"]) > 0:
        arrs["o3uv"] = np.ascontiguousarray(o3["uv"], dtype=np.float32)
        arrs["o3xyz"] = np.ascontiguousarray(o3["xyz"], dtype=np.float64)
        arrs["o3cam"] = np.ascontiguousarray(o3["cam"], dtype=np.int32)
        p.n_obs3d = len(arrs["o3cam"])
        p.obs3d_uv, p.obs3d_xyz, p.obs3d_cam = _p(arrs["o3uv"]), _p(arrs["o3xyz"]), _p(arrs["o3cam"])
    else:
        p.n_obs3d = 0
    p.factor_type = sc.factor_type
    ic = getattr(sc, "ic_of_cam", None)
    if ic is not None:
        arrs["ic"] = np.ascontiguousarray(ic, dtype=np.int32)
        if len(arrs["ic"]) != sc.n_cam:
            raise ValueError("ic_of_cam must have one id per camera")
        p.ic_of_cam = _p(arrs["ic"])
    return p


class BaBatch:
    """Device-resident batch of independent PTZ-IBA problems (ptz_ba_batch_*)."""

    def __init__(self, scenes, **opt):
        self.scenes = list(scenes)
        self.n = len(self.scenes)
        keep = []
        probs = (BaProblem * self.n)(*[_pack_problem(s, keep) for s in self.scenes])
        self.opt = default_options(**opt)
        self.handle = C.c_void_p()
        _check(lib().ptz_ba_batch_create(self.n, probs, C.byref(self.opt), C.byref(self.handle)), "ptz_ba_batch_create")
        self.cam_off = np.concatenate([[0], np.cumsum([s.n_cam for s in self.scenes])])
        self.ray_off = np.concatenate([[0], np.cumsum([s.n_ray for s in self.scenes])])
        self.obs_off = np.concatenate([[0], np.cumsum([s.n_obs for s in self.scenes])])
        self.nw = int(lib().ptz_ba_cam_block_dim(self.scenes[0].factor_type))
        self.nc = int(lib().ptz_ba_batch_cam_block_dim(self.handle))

    def close(self):
        if self.handle:
            lib().ptz_ba_batch_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_state(self, cams=None, rays=None, tlws=None):
        cam = np.ascontiguousarray(np.concatenate([s.cam_init for s in self.scenes] if cams is None else cams), dtype=np.float64)
        ray = np.ascontiguousarray(np.concatenate([s.ray_init for s in self.scenes] if rays is None else rays), dtype=np.float64)
        if tlws is None and any(getattr(s, "tlw_init", None) is not None for s in self.scenes):
            tlws = [getattr(s, "tlw_init", None) if getattr(s, "tlw_init", None) is not None else np.zeros(6) for s in self.scenes]
        tlw = None if tlws is None else np.ascontiguousarray(np.stack(tlws), dtype=np.float64)
        _check(lib().ptz_ba_batch_set_state(self.handle, _p(cam), _p(ray), _p(tlw)), "ptz_ba_batch_set_state")

    def set_disp(self, disps):
        """PTZRayDistDisp: the initial displacement block (d0, d1, d2) of every scene ([n, 3]; zeros unless set)."""
        d = np.ascontiguousarray(np.asarray(disps, dtype=np.float64).reshape(self.n, 3))
        _check(lib().ptz_ba_batch_set_disp(self.handle, _p(d)), "ptz_ba_batch_set_disp")

    def get_disp(self):
        d = np.zeros((self.n, 3))
        _check(lib().ptz_ba_batch_get_disp(self.handle, _p(d)), "ptz_ba_batch_get_disp")
        return d

    def pix2ray(self):
        _check(lib().ptz_ba_batch_pix2ray(self.handle), "ptz_ba_batch_pix2ray")

    def solve(self):
        summ = (LmSummary * self.n)()
        _check(lib().ptz_ba_batch_solve(self.handle, summ), "ptz_ba_batch_solve")
        return [s.as_dict() for s in summ]

    def get_state(self):
        cam = np.zeros((int(self.cam_off[-1]), 15))
        ray = np.zeros((int(self.ray_off[-1]), 3))
        tlw = np.zeros((self.n, 6))
        _check(lib().ptz_ba_batch_get_state(self.handle, _p(cam), _p(ray), _p(tlw)), "ptz_ba_batch_get_state")
        cams = [cam[self.cam_off[i]:self.cam_off[i + 1]] for i in range(self.n)]
        rays = [ray[self.ray_off[i]:self.ray_off[i + 1]] for i in range(self.n)]
        self.last_tlw = tlw
        return cams, rays

    def last_solve_ms(self) -> float:
        ms = C.c_double()
        _check(lib().ptz_ba_batch_last_solve_ms(self.handle, C.byref(ms)), "ptz_ba_batch_last_solve_ms")
        return ms.value

    def set_profiling(self, enable: bool):
        _check(lib().ptz_ba_batch_set_profiling(self.handle, int(enable)), "ptz_ba_batch_set_profiling")

    def get_profile(self):
        ms = (C.c_double * PROF_SLOTS)()
        cnt = (C.c_int64 * PROF_SLOTS)()
        names = (C.c_char_p * PROF_SLOTS)()
        _check(lib().ptz_ba_batch_get_profile(self.handle, ms, cnt, names), "ptz_ba_batch_get_profile")
        return {names[i].decode(): {"ms": ms[i], "launches": cnt[i]} for i in range(PROF_SLOTS) if names[i]}

    def linearize(self, index=0):
        s = self.scenes[index]
        nc = self.nc
        cost = C.c_double()
        g_c = np.zeros((s.n_cam, nc)); U = np.zeros((s.n_cam, nc, nc))
        g_r = np.zeros((s.n_ray, 3)); V = np.zeros((s.n_ray, 3, 3)); W = np.zeros((s.n_obs, self.nw, 3))
        _check(lib().ptz_ba_batch_linearize(self.handle, index, C.byref(cost), _p(g_c), _p(U), _p(g_r), _p(V), _p(W)),
               "ptz_ba_batch_linearize")
        return dict(cost=cost.value, g_c=g_c, U=U, g_r=g_r, V=V, W=W, nc=nc)

    REDUCED_INFO = ("kernel", "table_global", "np", "n_tiles", "reordered", "max_cam_obs", "max_cam_run", "threads")

    def reduced_system(self, index=0, scale_c=None, scale_r=None, poison=True):
        """ptz_debug_batch_reduced_system: the damped reduced camera system of problem `index`'s first LM step as the solver's own
        launches build it, with the caller's Jacobi scales (scale_c [n_cam, NC], scale_r [n_ray, 3]; None: 1.0).  Returns
        (S [n, n], b [n], diag_c [n_cam, NC], info: int32 [8], see REDUCED_INFO) in the cameras' numbering."""
        if not 0 <= index < self.n:  # (the library refuses it before it reads anything)
            one = np.zeros(1)
            _check(lib().ptz_debug_batch_reduced_system(self.handle, int(index), None, None, 0, _p(one), _p(one), None, None),
                   "ptz_debug_batch_reduced_system")
        s = self.scenes[index]
        nc = self.nc
        n = s.n_cam * nc
        if scale_c is not None:
            scale_c = np.ascontiguousarray(scale_c, dtype=np.float64)
            if scale_c.shape != (s.n_cam, nc):
                raise ValueError("scale_c must be [n_cam, NC]")
        if scale_r is not None:
            scale_r = np.ascontiguousarray(scale_r, dtype=np.float64)
            if scale_r.shape != (s.n_ray, 3):
                raise ValueError("scale_r must be [n_ray, 3]")
        S = np.zeros((n, n)); b = np.zeros(n); diag_c = np.zeros((s.n_cam, nc)); info = np.zeros(8, dtype=np.int32)
        _check(lib().ptz_debug_batch_reduced_system(self.handle, int(index), _p(scale_c), _p(scale_r), 1 if poison else 0, _p(S), _p(b),
                                                    _p(diag_c), _p(info)), "ptz_debug_batch_reduced_system")
        return S, b, diag_c, info

    def covariance(self, gauge_cam=None, pixel_sigma=0.0, cov=None, sigma0=None):
        """ptz_ba_batch_covariance at the batch's current state (after a solve: the minimum-cost point).  gauge_cam: the anchor
        camera of every problem (None: camera 0).  Returns (cov: list of [n_cam, NF, NF], sigma0 [n], status [n], device_ms);
        free parameters [fx, (fy), d1, d2, d3, (k1)] per camera.  Problems whose status is not COV_OK keep what `cov` / `sigma0`
        held (zeros unless given: cov as one [sum n_cam, NF, NF] array)."""
        n_cams = self.n_cams if hasattr(self, "n_cams") else [s.n_cam for s in self.scenes]
        ft = self.scenes[0].factor_type if self.scenes else self.factor_type
        nf = ba_cov_dim(ft)
        off = np.concatenate([[0], np.cumsum(n_cams)]).astype(int)
        cov = np.zeros((off[-1], nf, nf)) if cov is None else cov
        sigma0 = np.zeros(self.n) if sigma0 is None else sigma0
        assert cov.dtype == np.float64 and cov.flags.c_contiguous and cov.size == off[-1] * nf * nf
        assert sigma0.dtype == np.float64 and sigma0.flags.c_contiguous and len(sigma0) == self.n
        status = np.full(self.n, -1, dtype=np.int32)
        g = None if gauge_cam is None else np.ascontiguousarray(gauge_cam, dtype=np.int32)
        if g is not None and len(g) != self.n:
            raise ValueError("gauge_cam must name one camera per problem")
        ms = C.c_double()
        _check(lib().ptz_ba_batch_covariance(self.handle, _p(g), C.c_double(pixel_sigma), _p(cov), _p(sigma0), _p(status), C.byref(ms)),
               "ptz_ba_batch_covariance")
        return [cov[off[i]:off[i + 1]] for i in range(self.n)], sigma0, status, ms.value

    def covariance_georef(self, gauge_cam=None, pixel_sigma=0.0, annotation_sigma=0.0, cov=None, cov_centre=None, sigma0=None):
        """ptz_ba_batch_covariance_georef at the batch's current state, T_l_w included: the covariance of the WORLD cameras
        R_i R_lw and of the rig's projection centre.  Returns (cov: list of [n_cam, NF, NF] over [fx, d1, d2, d3, (k1)],
        cov_centre [n, 3, 3], sigma0 [n, 2] = (key points, annotations), status [n], device_ms).  Problems whose status is not
        COV_OK keep what `cov` / `cov_centre` / `sigma0` held (zeros unless given: cov as one [sum n_cam, NF, NF] array)."""
        n_cams = self.n_cams if hasattr(self, "n_cams") else [s.n_cam for s in self.scenes]
        ft = self.scenes[0].factor_type if self.scenes else self.factor_type
        nf = ba_geo_cov_dim(ft)
        off = np.concatenate([[0], np.cumsum(n_cams)]).astype(int)
        cov = np.zeros((off[-1], nf, nf)) if cov is None else cov
        cov_centre = np.zeros((self.n, 3, 3)) if cov_centre is None else cov_centre
        sigma0 = np.zeros((self.n, 2)) if sigma0 is None else sigma0
        for a, size in ((cov, off[-1] * nf * nf), (cov_centre, 9 * self.n), (sigma0, 2 * self.n)):
            assert a.dtype == np.float64 and a.flags.c_contiguous and a.size == size
        status = np.full(self.n, -1, dtype=np.int32)
        g = None if gauge_cam is None else np.ascontiguousarray(gauge_cam, dtype=np.int32)
        if g is not None and len(g) != self.n:
            raise ValueError("gauge_cam must name one camera per problem")
        ms = C.c_double()
        _check(lib().ptz_ba_batch_covariance_georef(self.handle, _p(g), C.c_double(pixel_sigma), C.c_double(annotation_sigma), _p(cov),
                                                    _p(cov_centre), _p(sigma0), _p(status), C.byref(ms)), "ptz_ba_batch_covariance_georef")
        return [cov[off[i]:off[i + 1]] for i in range(self.n)], cov_centre, sigma0, status, ms.value


    def _extents(self, n_obs, n_ray):
        """per-problem (n_cam, n_ray, n_obs, n_obs3d); a ViewBatch has no host-side scenes and is told the packed problems' counts"""
        if self.scenes:
            return ([s.n_cam for s in self.scenes], [s.n_ray for s in self.scenes], [s.n_obs for s in self.scenes],
                    [0 if getattr(s, "obs3d", None) is None else len(s.obs3d["cam"]) for s in self.scenes])
        if n_obs is None or n_ray is None:
            raise ValueError("a ViewBatch needs n_obs and n_ray of the packed problem of every view (api.view_problem)")
        return list(self.n_cams), [int(x) for x in n_ray], [int(x) for x in n_obs], [0] * self.n

    def residuals(self, median=True, n_obs=None, n_ray=None, only=None):
        """ptz_ba_batch_residuals at the batch's current state.  Returns a list of dicts, one per problem: err_px [n_obs] in the
        caller's observation order, ray_max / ray_worst [n_ray], view_rms / view_max / view_count [n_cam], rms, median (the exact
        lower median; None when median=False), err3d_px [n_obs3d], rms3d (NaN without annotations); plus device_ms on the first.
        only: names of the outputs wanted (the others are passed as NULL and come back as None)."""
        ncam, nray, nobs, no3 = self._extents(n_obs, n_ray)
        names = ["err_px", "ray_max", "ray_worst", "view_rms", "view_max", "view_count", "rms", "median", "err3d_px", "rms3d"]
        want = set(names if only is None else only)
        if not median:
            want.discard("median")
        size = dict(err_px=sum(nobs), ray_max=sum(nray), ray_worst=sum(nray), view_rms=sum(ncam), view_max=sum(ncam), view_count=sum(ncam),
                    rms=self.n, median=self.n, err3d_px=sum(no3), rms3d=self.n)
        arr = {k: (np.zeros(max(size[k], 1), dtype=np.int32 if k in ("ray_worst", "view_count") else np.float64) if k in want else None)
               for k in names}
        ms = C.c_double()
        _check(lib().ptz_ba_batch_residuals(self.handle, *[_p(arr[k]) for k in names], C.byref(ms)), "ptz_ba_batch_residuals")
        out = []
        off = dict(o=0, r=0, c=0, a=0)
        for i in range(self.n):
            d = {}
            for k, (key, cnt) in dict(err_px=("o", nobs[i]), ray_max=("r", nray[i]), ray_worst=("r", nray[i]), view_rms=("c", ncam[i]),
                                      view_max=("c", ncam[i]), view_count=("c", ncam[i]), err3d_px=("a", no3[i])).items():
                d[k] = None if arr[k] is None else arr[k][off[key]:off[key] + cnt].copy()
            for k in ("rms", "median", "rms3d"):
                d[k] = None if arr[k] is None else float(arr[k][i])
            off["o"] += nobs[i]; off["r"] += nray[i]; off["c"] += ncam[i]; off["a"] += no3[i]
            out.append(d)
        if out:
            out[0]["device_ms"] = ms.value
        return out

    def trim_select(self, trim_px=4.0, k_sigma=3.0, n_obs=None, n_ray=None):
        """ptz_ba_batch_trim_select at the batch's current state.  Returns (reject: list of uint8 [n_obs] in the caller's order,
        threshold [n], n_reject [n], device_ms)."""
        _, _, nobs, _ = self._extents(n_obs, n_ray)
        rej = np.zeros(max(sum(nobs), 1), dtype=np.uint8)
        thr = np.zeros(self.n)
        nrej = np.zeros(self.n, dtype=np.int32)
        ms = C.c_double()
        _check(lib().ptz_ba_batch_trim_select(self.handle, C.c_double(trim_px), C.c_double(k_sigma), _p(rej), _p(thr), _p(nrej), C.byref(ms)),
               "ptz_ba_batch_trim_select")
        oo = np.concatenate([[0], np.cumsum(nobs)]).astype(int)
        return [rej[oo[i]:oo[i + 1]].copy() for i in range(self.n)], thr, nrej, ms.value


class RigView(C.Structure):
    _fields_ = [("rig", C.c_void_p), ("n_cam", C.c_int32), ("cam_image", C.c_void_p)]


class Rig:
    """One rig's tracks resident in HBM (ptz_rig_create): trk_ptr [n_track + 1], per view the image id (ascending inside a
    track) and the pixel."""

    def __init__(self, n_img, trk_ptr, trk_img, trk_uv, device_id=0):
        self.n_img = int(n_img)
        self.trk_ptr = np.ascontiguousarray(trk_ptr, dtype=np.int64)
        self.trk_img = np.ascontiguousarray(trk_img, dtype=np.int32)
        self.trk_uv = np.ascontiguousarray(trk_uv, dtype=np.float32)
        self.handle = C.c_void_p()
        _check(lib().ptz_rig_create(self.n_img, len(self.trk_ptr) - 1, _p(self.trk_ptr), _p(self.trk_img), _p(self.trk_uv), int(device_id),
                                    C.byref(self.handle)), "ptz_rig_create")

    @classmethod
    def from_scene(cls, sc, device_id=0):
        """The tracks of a synthetic scene (its observations are (track, image)-ordered: every ray is one track)."""
        ptr = np.concatenate([[0], np.cumsum(np.bincount(sc.obs_ray, minlength=sc.n_ray))]).astype(np.int64)
        return cls(sc.n_cam, ptr, sc.obs_cam, sc.obs_uv, device_id)

    def close(self):
        if self.handle:
            lib().ptz_rig_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def view_problem(sc, images):
    """The packed problem of the candidate set `images` (ascending) of a synthetic scene, as PTZRayOptimizer::Pack makes it on the
    host: observations of candidate views in (track, image) order, tracks without one dropped, cameras and rays renumbered,
    weights = FULL track length (ptzray_optimizer.cc:805).  Returns a scene-like object for BaBatch."""
    import copy
    images = np.asarray(images, dtype=np.int64)
    cmap = -np.ones(sc.n_cam, dtype=np.int64)
    cmap[images] = np.arange(len(images))
    keep = cmap[sc.obs_cam] >= 0
    v = copy.copy(sc)
    v.n_cam = len(images)
    v.obs_uv = sc.obs_uv[keep]
    v.obs_cam = cmap[sc.obs_cam[keep]].astype(np.int32)
    tracks, new_ray = np.unique(sc.obs_ray[keep], return_inverse=True)
    v.obs_ray = new_ray.astype(np.int32)
    v.n_ray = len(tracks)
    v.ray_weight = np.bincount(sc.obs_ray, minlength=sc.n_ray)[tracks].astype(np.float64)
    v.cam_init = sc.cam_init[images].copy(); v.cam_gt = sc.cam_gt[images].copy()
    v.ray_init = sc.ray_init[tracks].copy(); v.ray_gt = sc.ray_gt[tracks].copy()
    v.ic_of_cam = None
    v.view_tracks = tracks
    return v


class ViewBatch(BaBatch):
    """ptz_ba_batch_create_views: the batch of the packed problems of (rig, candidate images) views, built on the device."""

    def __init__(self, rigs, image_lists, factor_type=0, **opt):
        self.scenes = []
        self.n = len(rigs)
        self._keep = [np.ascontiguousarray(im, dtype=np.int32) for im in image_lists]
        views = (RigView * self.n)()
        for i, (rg, im) in enumerate(zip(rigs, self._keep)):
            views[i].rig = rg.handle
            views[i].n_cam = len(im)
            views[i].cam_image = _p(im)
        self.opt = default_options(**opt)
        self.handle = C.c_void_p()
        _check(lib().ptz_ba_batch_create_views(self.n, views, int(factor_type), C.byref(self.opt), C.byref(self.handle)), "ptz_ba_batch_create_views")
        self.nw = int(lib().ptz_ba_cam_block_dim(int(factor_type)))
        self.nc = int(lib().ptz_ba_batch_cam_block_dim(self.handle))
        self.n_cams = [len(im) for im in self._keep]
        self.factor_type = int(factor_type)

    def set_state_pix2ray(self, cams, rkinv):
        cam = np.ascontiguousarray(np.concatenate(cams), dtype=np.float64)
        rk = np.ascontiguousarray(np.concatenate(rkinv), dtype=np.float64)
        _check(lib().ptz_ba_batch_set_state_pix2ray(self.handle, _p(cam), _p(rk)), "ptz_ba_batch_set_state_pix2ray")

    def get_cams(self):
        cam = np.zeros((int(sum(self.n_cams)), 15))
        tlw = np.zeros((self.n, 6))
        _check(lib().ptz_ba_batch_get_state(self.handle, _p(cam), None, _p(tlw)), "ptz_ba_batch_get_state")
        off = np.concatenate([[0], np.cumsum(self.n_cams)])
        return [cam[off[i]:off[i + 1]] for i in range(self.n)]


def initial_rays(batch, total_rays) -> np.ndarray:
    r = np.zeros((int(total_rays), 3))
    _check(lib().ptz_debug_batch_initial_rays(batch.handle, _p(r)), "ptz_debug_batch_initial_rays")
    return r


def structure_hash(batch) -> int:
    h = C.c_uint64()
    _check(lib().ptz_debug_batch_structure_hash(batch.handle, C.byref(h)), "ptz_debug_batch_structure_hash")
    return int(h.value)


def ba_solve(scene, cam0=None, ray0=None, tlw0=None, return_tlw=False, **opt):
    """One-shot ptz_ba_solve.  Returns (cam, ray, summary dict) [+ tlw when return_tlw]."""
    keep = []
    p = _pack_problem(scene, keep)
    cam = np.array(scene.cam_init if cam0 is None else cam0, dtype=np.float64, order="C").copy()
    ray = np.array(scene.ray_init if ray0 is None else ray0, dtype=np.float64, order="C").copy()
    if tlw0 is None:
        tlw0 = getattr(scene, "tlw_init", None)
    tlw = np.zeros(6) if tlw0 is None else np.array(tlw0, dtype=np.float64).copy()
    o = default_options(**opt)
    s = LmSummary()
    _check(lib().ptz_ba_solve(C.byref(p), _p(cam), _p(ray), _p(tlw), C.byref(o), C.byref(s)), "ptz_ba_solve")
    return (cam, ray, s.as_dict(), tlw) if return_tlw else (cam, ray, s.as_dict())


def ba_trim_problem(scene, reject):
    """ptz_ba_problem_trim (host logic, no device): `scene` without the observations with a non-zero reject byte and without the
    rays left with fewer than two observations.  Returns (trimmed scene-like copy, ray_map [n_ray] with -1 for removed rays);
    ray_init / ray_gt of the copy follow the map.  Raises PtzError(PTZ_ENOOBS) if a camera would lose every observation."""
    import copy
    keep = []
    p = _pack_problem(scene, keep)
    rej = np.ascontiguousarray(reject, dtype=np.uint8)
    if len(rej) != p.n_obs:
        raise ValueError("one reject byte per observation")
    uv = np.zeros((p.n_obs, 2), dtype=np.float32)
    oc = np.zeros(p.n_obs, dtype=np.int32)
    orr = np.zeros(p.n_obs, dtype=np.int32)
    w = np.zeros(p.n_ray)
    rmap = np.zeros(p.n_ray, dtype=np.int32)
    nr, no = C.c_int32(), C.c_int64()
    _check(lib().ptz_ba_problem_trim(C.byref(p), _p(rej), _p(uv), _p(oc), _p(orr), _p(w), _p(rmap), C.byref(nr), C.byref(no)),
           "ptz_ba_problem_trim")
    t = copy.copy(scene)
    t.n_ray, n_obs = int(nr.value), int(no.value)
    t.obs_uv, t.obs_cam, t.obs_ray, t.ray_weight = uv[:n_obs].copy(), oc[:n_obs].copy(), orr[:n_obs].copy(), w[:t.n_ray].copy()
    for k in ("ray_init", "ray_gt"):
        if getattr(scene, k, None) is not None:
            setattr(t, k, np.asarray(getattr(scene, k))[rmap >= 0].copy())
    return t, rmap


def ba_solve_trimmed_batch(scenes, cams=None, rays=None, trim_px=4.0, k_sigma=3.0, max_rounds=8, **opt):
    """ptz_ba_solve_trimmed_batch.  Returns (cams, rays, summaries, kept, reports): per problem the cameras and summary of its
    last solve, the rays in the input numbering (removed rays as given), kept uint8 [n_obs], and the report dict (rounds, flags,
    n_obs_removed, n_ray_removed, threshold, rms_first, rms_last)."""
    keep = []
    n = len(scenes)
    probs = (BaProblem * n)(*[_pack_problem(s, keep) for s in scenes])
    o = default_options(**opt)
    cam = np.ascontiguousarray(np.concatenate([s.cam_init for s in scenes] if cams is None else cams), dtype=np.float64).copy()
    ray = np.ascontiguousarray(np.concatenate([s.ray_init for s in scenes] if rays is None else rays), dtype=np.float64).copy()
    tlw = np.ascontiguousarray(np.stack([getattr(s, "tlw_init", None) if getattr(s, "tlw_init", None) is not None else np.zeros(6)
                                         for s in scenes]), dtype=np.float64).copy()
    to = TrimOptions()
    lib().ptz_trim_options_default(C.byref(to))
    to.trim_px, to.k_sigma, to.max_rounds = float(trim_px), float(k_sigma), int(max_rounds)
    summ = (LmSummary * n)()
    rep = (TrimReport * n)()
    oo = np.concatenate([[0], np.cumsum([len(k["cam"]) for k in keep])]).astype(int)
    kept = np.zeros(max(int(oo[-1]), 1), dtype=np.uint8)
    _check(lib().ptz_ba_solve_trimmed_batch(n, probs, _p(cam), _p(ray), _p(tlw), C.byref(to), C.byref(o), summ, _p(kept), rep),
           "ptz_ba_solve_trimmed_batch")
    co = np.concatenate([[0], np.cumsum([s.n_cam for s in scenes])]).astype(int)
    ro = np.concatenate([[0], np.cumsum([s.n_ray for s in scenes])]).astype(int)
    ba_solve_trimmed_batch.last_tlw = tlw
    return ([cam[co[i]:co[i + 1]] for i in range(n)], [ray[ro[i]:ro[i + 1]] for i in range(n)], [s.as_dict() for s in summ],
            [kept[oo[i]:oo[i + 1]].copy() for i in range(n)], [r.as_dict() for r in rep])


def ba_solve_trimmed(scene, cam0=None, ray0=None, trim_px=4.0, k_sigma=3.0, max_rounds=8, **opt):
    """One problem through ptz_ba_solve_trimmed.  Returns (cam, ray, summary, kept, report)."""
    keep = []
    p = _pack_problem(scene, keep)
    cam = np.array(scene.cam_init if cam0 is None else cam0, dtype=np.float64, order="C").copy()
    ray = np.array(scene.ray_init if ray0 is None else ray0, dtype=np.float64, order="C").copy()
    tlw0 = getattr(scene, "tlw_init", None)
    tlw = np.zeros(6) if tlw0 is None else np.array(tlw0, dtype=np.float64).copy()
    o = default_options(**opt)
    to = TrimOptions()
    lib().ptz_trim_options_default(C.byref(to))
    to.trim_px, to.k_sigma, to.max_rounds = float(trim_px), float(k_sigma), int(max_rounds)
    s = LmSummary()
    rep = TrimReport()
    kept = np.zeros(max(int(p.n_obs), 1), dtype=np.uint8)
    _check(lib().ptz_ba_solve_trimmed(C.byref(p), _p(cam), _p(ray), _p(tlw), C.byref(to), C.byref(o), C.byref(s), _p(kept), C.byref(rep)),
           "ptz_ba_solve_trimmed")
    return cam, ray, s.as_dict(), kept[:int(p.n_obs)].copy(), rep.as_dict()


def ba_cov_dim(factor_type) -> int:
    """free parameters per camera of ptz_ba_batch_covariance, [fx, (fy), d1, d2, d3, (k1)]: 4, 5, 6 for PTZRay, PTZRayDist, PTZRayFxfyDist"""
    nf = int(lib().ptz_ba_cov_dim(int(factor_type)))
    _check(min(nf, 0), "ptz_ba_cov_dim")
    return nf


def ba_covariance(scene, cam, ray, gauge_cam=0, pixel_sigma=0.0, cov=None, **opt):
    """One-shot ptz_ba_covariance of one problem at the state (cam, ray), no solve.  Returns (cov [n_cam, NF, NF], sigma0, status);
    cov / sigma0 are those given (zeros / 0.0) unless status is COV_OK."""
    keep = []
    p = _pack_problem(scene, keep)
    nf = ba_cov_dim(scene.factor_type)
    cam = np.ascontiguousarray(cam, dtype=np.float64)
    ray = np.ascontiguousarray(ray, dtype=np.float64)
    cov = np.zeros((scene.n_cam, nf, nf)) if cov is None else cov
    s0 = C.c_double(0.0)
    st = C.c_int32(-1)
    o = default_options(**opt)
    _check(lib().ptz_ba_covariance(C.byref(p), _p(cam), _p(ray), int(gauge_cam), C.c_double(pixel_sigma), C.byref(o), _p(cov), C.byref(s0),
                                   C.byref(st)), "ptz_ba_covariance")
    return cov, s0.value, int(st.value)


def ba_geo_cov_dim(factor_type) -> int:
    """entries per camera of ptz_ba_batch_covariance_georef, [fx, d1, d2, d3, (k1)]: 4, 5 for PTZRay, PTZRayDist"""
    nf = int(lib().ptz_ba_geo_cov_dim(int(factor_type)))
    _check(min(nf, 0), "ptz_ba_geo_cov_dim")
    return nf


def ba_covariance_georef(scene, cam, ray, tlw, gauge_cam=0, pixel_sigma=0.0, annotation_sigma=0.0, cov=None, cov_centre=None, **opt):
    """One-shot ptz_ba_covariance_georef of one annotated problem at the state (cam, ray, tlw), no solve.  Returns
    (cov [n_cam, NF, NF], cov_centre [3, 3], sigma0 [2], status); the outputs are those given (zeros) unless status is COV_OK."""
    keep = []
    p = _pack_problem(scene, keep)
    nf = ba_geo_cov_dim(scene.factor_type)
    cam = np.ascontiguousarray(cam, dtype=np.float64)
    ray = np.ascontiguousarray(ray, dtype=np.float64)
    tlw = np.ascontiguousarray(tlw, dtype=np.float64)
    cov = np.zeros((scene.n_cam, nf, nf)) if cov is None else cov
    cov_centre = np.zeros((3, 3)) if cov_centre is None else cov_centre
    s0 = np.zeros(2)
    st = C.c_int32(-1)
    o = default_options(**opt)
    _check(lib().ptz_ba_covariance_georef(C.byref(p), _p(cam), _p(ray), _p(tlw), int(gauge_cam), C.c_double(pixel_sigma),
                                          C.c_double(annotation_sigma), C.byref(o), _p(cov), _p(cov_centre), _p(s0), C.byref(st)),
           "ptz_ba_covariance_georef")
    return cov, cov_centre, s0, int(st.value)


def ba_solve_disp(scene, cam0=None, ray0=None, tlw0=None, disp0=None, **opt):
    """One-shot ptz_ba_solve_disp (PTZRayDistDisp).  Returns (cam, ray, summary dict, tlw, disp).

    The returned camera vectors hold the refined PARAMETER blocks: t_z (cam[:, 9]) comes back as it went in.  The reference's
    ObtainRefinedCameraParams additionally folds the refined displacement into it, t_z += d0 + d1 fx + d2 fx^2
    (ptzray_optimizer.cc:693, 714); the C++ class PTZRayOptimizer does that on read-back, this C-ABI level (and
    ptz_ba_batch_get_state / get_disp) hands out the two blocks separately -- `fold_displacement(cam, disp)` applies it."""
    keep = []
    p = _pack_problem(scene, keep)
    cam = np.array(scene.cam_init if cam0 is None else cam0, dtype=np.float64, order="C").copy()
    ray = np.array(scene.ray_init if ray0 is None else ray0, dtype=np.float64, order="C").copy()
    if tlw0 is None:
        tlw0 = getattr(scene, "tlw_init", None)
    tlw = np.zeros(6) if tlw0 is None else np.array(tlw0, dtype=np.float64).copy()
    disp = np.zeros(3) if disp0 is None else np.array(disp0, dtype=np.float64).copy()
    o = default_options(**opt)
    s = LmSummary()
    _check(lib().ptz_ba_solve_disp(C.byref(p), _p(cam), _p(ray), _p(tlw), _p(disp), C.byref(o), C.byref(s)), "ptz_ba_solve_disp")
    return cam, ray, s.as_dict(), tlw, disp


def fold_displacement(cam, disp):
    """ObtainRefinedCameraParams' last step for PTZRayDistDisp (ptzray_optimizer.cc:693, 714): t_z += d0 + d1 fx + d2 fx^2."""
    out = np.array(cam, dtype=np.float64).copy()
    out[:, 9] += disp[0] + disp[1] * out[:, 0] + disp[2] * out[:, 0] ** 2
    return out


def plan_tile_order(mask, first_dense):
    """Elimination order of a tile graph (host logic of ptz_ba_batch_create).  mask: [nt, nt] lower-triangular adjacency.
    Returns (planned, perm, (lane_a, lane_b))."""
    m = np.ascontiguousarray(mask, dtype=np.uint8)
    nt = m.shape[0]
    perm = np.zeros(nt, dtype=np.int32)
    lanes = np.zeros(2, dtype=np.int32)
    sched = np.zeros((nt, 4), dtype=np.int32)
    n_steps = np.zeros(1, dtype=np.int32)
    rc = lib().ptz_ba_plan_tile_order(nt, int(first_dense), _p(m), _p(perm), _p(lanes), _p(sched), _p(n_steps))
    if rc < 0:
        raise PtzError(rc, "ptz_ba_plan_tile_order")
    plan_tile_order.last_schedule = sched[:int(n_steps[0])]
    return bool(rc), perm, (int(lanes[0]), int(lanes[1]))


def chol_solve_batch(A, rhs, device_id=0):
    """A: [count, n, n] SPD (lower triangle read), rhs: [count, n].  Returns (x, fail, device_ms)."""
    A = np.ascontiguousarray(A, dtype=np.float64)
    rhs = np.ascontiguousarray(rhs, dtype=np.float64)
    count, n = A.shape[0], A.shape[1]
    x = np.zeros((count, n))
    fail = np.zeros(count, dtype=np.int32)
    ms = C.c_double()
    _check(lib().ptz_chol_solve_batch(count, n, _p(A), _p(rhs), _p(x), _p(fail), device_id, C.byref(ms)), "ptz_chol_solve_batch")
    return x, fail, ms.value


CHOL_AUTO, CHOL_CHAIN, CHOL_STEP, CHOL_RIGHT, CHOL_LEFT = 0, 1, 2, 3, 4


def chol_solve_debug(A_list, rhs_list, path=0, poison=False, active=None, x0=None, fail0=None, device_id=0, ld=None):
    """The dense solve on a chosen launch path (CHOL_*), systems of different order in one call (ptz_debug_chol_solve).
    A_list: square arrays (lower triangle read), rhs_list: their right-hand sides.  poison: the buffers the kernels write
    before they read start as 0xFF bytes.  active: per system, 0 = skipped (its x and fail are x0[i] / fail0[i], default 0).
    Returns (list of x, fail [count] int32)."""
    count = len(A_list)
    n = np.array([np.shape(a)[0] for a in A_list], dtype=np.int32)
    ld = int(n.max()) if ld is None and count else int(ld or 0)
    A = np.zeros((count, max(ld, 1), max(ld, 1)))
    rhs = np.zeros((count, max(ld, 1)))
    x = np.zeros((count, max(ld, 1)))
    fail = np.zeros(count, dtype=np.int32) if fail0 is None else np.array(fail0, dtype=np.int32)
    for i in range(count):
        k = min(int(n[i]), ld)
        A[i, :k, :k] = np.asarray(A_list[i], dtype=np.float64)[:k, :k]
        rhs[i, :k] = np.asarray(rhs_list[i], dtype=np.float64)[:k]
        if x0 is not None:
            x[i, :k] = np.asarray(x0[i], dtype=np.float64)[:k]
    act = None if active is None else np.ascontiguousarray(active, dtype=np.int32)
    _check(lib().ptz_debug_chol_solve(count, _p(n), ld, _p(A), _p(rhs), _p(x), _p(fail), None if act is None else _p(act),
                                      int(path), 1 if poison else 0, device_id), "ptz_debug_chol_solve")
    return [x[i, :n[i]].copy() for i in range(count)], fail


def find_homographies(match_ptr, src_uv, dst_uv, ransac_thresh=4.0, device_id=0, mask=True):
    """RANSAC homography dst ~ H src of every pair of a match table on the device (the host estimator's bits; stands in
    for cv::findHomography(..., RANSAC, thresh) of LoadMatchesInfo).  Pair p owns matches [match_ptr[p], match_ptr[p+1]);
    src_uv / dst_uv: [n_match, 2].  Returns (H [n_pair, 3, 3] with h33 = 1 (zeros where not found), found [n_pair] int32,
    inlier mask [n_match] uint8 or None, device_ms)."""
    ptr = np.ascontiguousarray(match_ptr, dtype=np.int64)
    src = np.ascontiguousarray(src_uv, dtype=np.float32)
    dst = np.ascontiguousarray(dst_uv, dtype=np.float32)
    n = ptr.shape[0] - 1
    H = np.zeros((max(n, 0), 3, 3))
    found = np.zeros(max(n, 0), dtype=np.int32)
    m = np.zeros(int(ptr[-1]) if n > 0 else 0, dtype=np.uint8) if mask else None
    ms = C.c_double()
    _check(lib().ptz_homography_ransac_batch(n, _p(ptr), _p(src), _p(dst), C.c_double(ransac_thresh), device_id, _p(H), _p(found),
                                             _p(m), C.byref(ms)), "ptz_homography_ransac_batch")
    return H, found, m, ms.value


def _dptr(x):
    """A device buffer as a C pointer: an object with .data_ptr() (a torch tensor), an integer address, or None."""
    if x is None:
        return None
    return C.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else int(x))


def match_gate_table(max_pair_matches):
    """ptz_debug_match_gate_table (host logic only): (table int32, offsets int64 [max_pair_matches + 1])."""
    n = C.c_int64()
    off = np.zeros(max_pair_matches + 1, dtype=np.int64)
    _check(lib().ptz_debug_match_gate_table(int(max_pair_matches), None, C.byref(n), _p(off)), "ptz_debug_match_gate_table")
    tab = np.zeros(max(int(n.value), 1), dtype=np.int32)
    _check(lib().ptz_debug_match_gate_table(int(max_pair_matches), _p(tab), C.byref(n), None), "ptz_debug_match_gate_table")
    return tab[:int(n.value)], off


class MatchGate:
    """ptz_match_gate: RANSAC inlier gating of device-resident CSR match sets (up to max_pairs pairs, max_matches matches,
    max_pair_matches matches in one pair)."""

    def __init__(self, max_pairs, max_matches, max_pair_matches, device_id=0):
        self.max_pairs, self.max_matches, self.max_pair_matches = int(max_pairs), int(max_matches), int(max_pair_matches)
        self.handle = C.c_void_p()
        lib().ptz_match_gate_destroy.restype = None
        _check(lib().ptz_match_gate_create(self.max_pairs, C.c_int64(self.max_matches), self.max_pair_matches, int(device_id),
                                           C.byref(self.handle)), "ptz_match_gate_create")

    def run_device(self, n_pair, d_match_ptr, d_uv_a, d_uv_b, d_found, d_out_ptr, d_out_uv_a, d_out_uv_b, d_H=None, d_mask=None,
                   d_out_index=None, ransac_thresh=4.0, min_inliers=0, stream=None):
        """ptz_match_gate_run_device: every d_* is a device buffer (torch tensor or integer address).  Enqueues on `stream`
        (integer hipStream_t handle, None = default stream) and returns without synchronising."""
        _check(lib().ptz_match_gate_run_device(self.handle, int(n_pair), _dptr(d_match_ptr), _dptr(d_uv_a), _dptr(d_uv_b),
                                               C.c_double(ransac_thresh), int(min_inliers), _dptr(d_H), _dptr(d_found), _dptr(d_mask),
                                               _dptr(d_out_ptr), _dptr(d_out_uv_a), _dptr(d_out_uv_b), _dptr(d_out_index),
                                               C.c_void_p(stream) if stream else None), "ptz_match_gate_run_device")

    def close(self):
        if self.handle:
            lib().ptz_match_gate_destroy(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def gate_matches(match_ptr, uv_a, uv_b, ransac_thresh=4.0, min_inliers=0, max_pair_matches=4096, device_id=0, gate=None):
    """Gate a CSR match set on the device (ptz_match_gate_run; through `gate`, or a MatchGate of the set's size).
    Returns a dict of numpy arrays: H [n_pair, 3, 3] (zeros where found != 1), found [n_pair] (-1: more than max_pair_matches
    matches), mask [n_match] (zeros where found != 1), out_ptr [n_pair + 1], out_uv_a / out_uv_b [n_kept, 2], out_index [n_kept],
    and device_ms."""
    ptr = np.ascontiguousarray(match_ptr, dtype=np.int64)
    a = np.ascontiguousarray(uv_a, dtype=np.float32).reshape(-1, 2)
    b = np.ascontiguousarray(uv_b, dtype=np.float32).reshape(-1, 2)
    n, nm = len(ptr) - 1, len(a)
    H = np.zeros((n, 3, 3))
    found = np.zeros(n, dtype=np.int32)
    mask = np.zeros(nm, dtype=np.uint8)
    out_ptr = np.zeros(n + 1, dtype=np.int64)
    oa, ob = np.zeros((nm, 2), dtype=np.float32), np.zeros((nm, 2), dtype=np.float32)
    oi = np.zeros(nm, dtype=np.int32)
    ms = C.c_double()
    g = gate if gate is not None else MatchGate(max(n, 1), nm, max_pair_matches, device_id)
    try:
        _check(lib().ptz_match_gate_run(g.handle, n, _p(ptr), _p(a), _p(b), C.c_double(ransac_thresh), int(min_inliers), _p(H), _p(found),
                                        _p(mask), _p(out_ptr), _p(oa), _p(ob), _p(oi), C.byref(ms)), "ptz_match_gate_run")
    finally:
        if gate is None:
            g.close()
    k = int(out_ptr[-1])
    return dict(H=H, found=found, mask=mask, out_ptr=out_ptr, out_uv_a=oa[:k], out_uv_b=ob[:k], out_index=oi[:k], device_ms=ms.value)


class RotFocalGate:
    """ptz_rotfocal_gate: the two-point rotation-and-focal RANSAC gate of assembled relocalization queries (up to max_pairs queries,
    max_matches matches; a query may have any number of them).  The contract is csrc/ptz_rotfocal.h."""

    def __init__(self, max_pairs, max_matches, device_id=0):
        self.max_pairs, self.max_matches = int(max_pairs), int(max_matches)
        self.handle = C.c_void_p()
        lib().ptz_rotfocal_gate_destroy.restype = None
        _check(lib().ptz_rotfocal_gate_create(self.max_pairs, C.c_int64(self.max_matches), int(device_id), C.byref(self.handle)),
               "ptz_rotfocal_gate_create")

    def run_device(self, n_pair, d_match_ptr, d_uv_a, d_uv_b, d_cam_ref, d_cam_cur, d_found, d_out_ptr, d_out_uv_a, d_out_uv_b, d_model=None,
                   d_H=None, d_mask=None, d_out_index=None, thresh=4.0, min_inliers=0, iters=128, stream=None):
        """ptz_rotfocal_gate_run_device: every d_* is a device buffer (torch tensor or integer address).  Enqueues on `stream`
        (integer hipStream_t handle, None = default stream) and returns without synchronising."""
        _check(lib().ptz_rotfocal_gate_run_device(self.handle, int(n_pair), _dptr(d_match_ptr), _dptr(d_uv_a), _dptr(d_uv_b), _dptr(d_cam_ref),
                                                  _dptr(d_cam_cur), C.c_double(thresh), int(min_inliers), int(iters), _dptr(d_model), _dptr(d_H),
                                                  _dptr(d_found), _dptr(d_mask), _dptr(d_out_ptr), _dptr(d_out_uv_a), _dptr(d_out_uv_b),
                                                  _dptr(d_out_index), C.c_void_p(stream) if stream else None), "ptz_rotfocal_gate_run_device")

    def run(self, match_ptr, uv_a, uv_b, cam_ref, cam_cur, thresh=4.0, min_inliers=0, iters=128, fill=0):
        """ptz_rotfocal_gate_run on host arrays.  Returns a dict of numpy arrays: model [n_pair, 10] (f, R row-major), H [n_pair, 3, 3],
        found [n_pair], mask [n_match] (model, H and mask keep `fill` where found != 1), out_ptr [n_pair + 1], out_uv_a / out_uv_b
        [n_kept, 2], out_index [n_kept], and device_ms."""
        ptr = np.ascontiguousarray(match_ptr, dtype=np.int64)
        a = np.ascontiguousarray(uv_a, dtype=np.float32).reshape(-1, 2)
        b = np.ascontiguousarray(uv_b, dtype=np.float32).reshape(-1, 2)
        cr = np.ascontiguousarray(cam_ref, dtype=np.float64).reshape(-1, 15)
        cc = np.ascontiguousarray(cam_cur, dtype=np.float64).reshape(-1, 15)
        n, nm = len(ptr) - 1, len(a)
        if len(cr) != n or len(cc) != n:
            raise ValueError("cam_ref and cam_cur need one camera per query")
        model, H = np.full((n, 10), float(fill)), np.full((n, 3, 3), float(fill))
        found = np.zeros(n, dtype=np.int32)
        mask = np.full(nm, fill, dtype=np.uint8)
        out_ptr = np.zeros(n + 1, dtype=np.int64)
        oa, ob = np.zeros((nm, 2), dtype=np.float32), np.zeros((nm, 2), dtype=np.float32)
        oi = np.zeros(nm, dtype=np.int32)
        ms = C.c_double()
        _check(lib().ptz_rotfocal_gate_run(self.handle, n, _p(ptr), _p(a), _p(b), _p(cr), _p(cc), C.c_double(thresh), int(min_inliers), int(iters),
                                           _p(model), _p(H), _p(found), _p(mask), _p(out_ptr), _p(oa), _p(ob), _p(oi), C.byref(ms)),
               "ptz_rotfocal_gate_run")
        k = int(out_ptr[-1])
        return dict(model=model, H=H, found=found, mask=mask, out_ptr=out_ptr, out_uv_a=oa[:k], out_uv_b=ob[:k], out_index=oi[:k],
                    device_ms=ms.value)

    def close(self):
        if self.handle:
            lib().ptz_rotfocal_gate_destroy(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def krt_solve_batch_gated(batch, max_reproj_error=100.0, ransac_thresh=4.0, min_inliers=0, **opt):
    """ptz_krt_solve_batch_gated: krt_solve_batch on the RANSAC inliers of every query's matches (uv_ref -> uv_cur homography).
    Returns (cam_world [n, 15], summaries, accepted, n_inliers [n], inlier_mask [n_match], H [n, 3, 3], (gate ms, LM ms))."""
    o = default_options(**opt)
    n = batch.n_query
    ptr = np.ascontiguousarray(batch.match_ptr, dtype=np.int64)
    uvr = np.ascontiguousarray(batch.uv_ref, dtype=np.float32)
    uvc = np.ascontiguousarray(batch.uv_cur, dtype=np.float32)
    cref = np.ascontiguousarray(batch.cam_ref, dtype=np.float64)
    ccur = np.array(batch.cam_init, dtype=np.float64, order="C").copy()
    summ = (LmSummary * n)()
    acc = np.zeros(n, dtype=np.int32)
    ninl = np.zeros(n, dtype=np.int32)
    mask = np.zeros(int(ptr[-1]), dtype=np.uint8)
    H = np.zeros((n, 3, 3))
    ms = np.zeros(2)
    _check(lib().ptz_krt_solve_batch_gated(n, _p(ptr), _p(uvr), _p(uvc), _p(cref), _p(ccur), batch.factor_type, C.c_double(max_reproj_error),
                                           C.c_double(ransac_thresh), int(min_inliers), C.byref(o), summ, _p(acc), _p(ninl), _p(mask),
                                           _p(H), _p(ms)), "ptz_krt_solve_batch_gated")
    return ccur, [s.as_dict() for s in summ], acc, ninl, mask, H, (float(ms[0]), float(ms[1]))


def krt_solve_batch(batch, max_reproj_error=100.0, **opt):
    """batch: synth.RelocBatch-like.  Returns (cam_world [n,15], summaries, accepted, device_ms)."""
    o = default_options(**opt)
    n = batch.n_query
    ptr = np.ascontiguousarray(batch.match_ptr, dtype=np.int64)
    uvr = np.ascontiguousarray(batch.uv_ref, dtype=np.float32)
    uvc = np.ascontiguousarray(batch.uv_cur, dtype=np.float32)
    cref = np.ascontiguousarray(batch.cam_ref, dtype=np.float64)
    ccur = np.array(batch.cam_init, dtype=np.float64, order="C").copy()
    summ = (LmSummary * n)()
    acc = np.zeros(n, dtype=np.int32)
    ms = C.c_double()
    point_ptr = getattr(batch, "point_ptr", None)
    if point_ptr is not None:  # 2D-3D constraints per query (KRTOptimizer::Add2d3dConstraints), world points
        pptr = np.ascontiguousarray(point_ptr, dtype=np.int64)
        p2 = np.ascontiguousarray(batch.pts2d, dtype=np.float32)
        p3 = np.ascontiguousarray(batch.pts3d, dtype=np.float64)
        _check(lib().ptz_krt_solve_batch_2d3d(n, _p(ptr), _p(uvr), _p(uvc), _p(pptr), _p(p2), _p(p3), _p(cref), _p(ccur),
                                              batch.factor_type, C.c_double(max_reproj_error), C.byref(o), summ, _p(acc),
                                              C.byref(ms)),
               "ptz_krt_solve_batch_2d3d")
    else:
        _check(lib().ptz_krt_solve_batch(n, _p(ptr), _p(uvr), _p(uvc), _p(cref), _p(ccur), batch.factor_type,
                                         C.c_double(max_reproj_error), C.byref(o), summ, _p(acc), C.byref(ms)),
               "ptz_krt_solve_batch")
    return ccur, [s.as_dict() for s in summ], acc, ms.value


class KrtAttempt(C.Structure):
    _fields_ = [("table", C.c_void_p), ("entry", C.c_int32)]


class KrtTable:
    """ptz_krt_table: the matches of a rig's table entries, resident on a device (entry e owns matches
    [match_ptr[e], match_ptr[e+1]) of uv_ref / uv_cur)."""

    def __init__(self, match_ptr, uv_ref, uv_cur, device_id=0):
        ptr = np.ascontiguousarray(match_ptr, dtype=np.int64)
        uvr = np.ascontiguousarray(uv_ref, dtype=np.float32)
        uvc = np.ascontiguousarray(uv_cur, dtype=np.float32)
        self.n_entry = len(ptr) - 1
        self.handle = C.c_void_p()
        lib().ptz_krt_table_destroy.restype = None
        _check(lib().ptz_krt_table_create(self.n_entry, _p(ptr), _p(uvr), _p(uvc), int(device_id), C.byref(self.handle)), "ptz_krt_table_create")

    def close(self):
        if self.handle:
            lib().ptz_krt_table_destroy(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def krt_solve_attempts(attempts, cam_ref, cam_init, factor_type=0, max_reproj_error=100.0, **opt):
    """ptz_krt_solve_attempts: attempts = [(KrtTable, entry), ...].  Returns (cam_world [n,15], summaries, accepted, device_ms)."""
    o = default_options(**opt)
    n = len(attempts)
    att = (KrtAttempt * n)(*[KrtAttempt(t.handle.value, int(e)) for t, e in attempts])
    cref = np.ascontiguousarray(cam_ref, dtype=np.float64)
    ccur = np.array(cam_init, dtype=np.float64, order="C").copy()
    summ = (LmSummary * n)()
    acc = np.zeros(n, dtype=np.int32)
    ms = C.c_double()
    _check(lib().ptz_krt_solve_attempts(n, att, _p(cref), _p(ccur), int(factor_type), C.c_double(max_reproj_error), C.byref(o), summ, _p(acc),
                                        C.byref(ms)), "ptz_krt_solve_attempts")
    return ccur, [s.as_dict() for s in summ], acc, ms.value


def krt_solve_batch_device(n_query, d_match_ptr, d_uv_ref, d_uv_cur, d_cam_ref, d_cam_cur, d_summaries, d_accepted, factor_type=0,
                           max_reproj_error=100.0, d_point_ptr=None, d_pts2d=None, d_pts3d=None, stream=None, **opt):
    """ptz_krt_solve_batch_device: every d_* argument is a device buffer given as an object with .data_ptr() (a torch tensor)
    or as an integer address; d_summaries needs n_query * sizeof(LmSummary) bytes.  Enqueues on `stream` (integer hipStream_t
    handle, None = default stream) and returns without synchronising."""
    o = default_options(**opt)

    def ptr(x):
        if x is None:
            return None
        return C.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else int(x))

    _check(lib().ptz_krt_solve_batch_device(int(n_query), ptr(d_match_ptr), ptr(d_uv_ref), ptr(d_uv_cur), ptr(d_point_ptr), ptr(d_pts2d),
                                            ptr(d_pts3d), ptr(d_cam_ref), ptr(d_cam_cur), int(factor_type), C.c_double(max_reproj_error),
                                            C.byref(o), ptr(d_summaries), ptr(d_accepted), C.c_void_p(stream) if stream else None),
           "ptz_krt_solve_batch_device")


def krt_free_dim(factor_type) -> int:
    """ptz_krt_free_dim: free parameters [fx, (fy), d1, d2, d3, (k1)] of a factor type (4, 5, 5, 6)."""
    nf = int(lib().ptz_krt_free_dim(int(factor_type)))
    if nf < 0:
        raise PtzError(nf, "ptz_krt_free_dim")
    return nf


def krt_covariance_batch(batch, cam_cur, match_mask=None, accepted=None, pixel_sigma=0.0, device_id=0, cov=None, sigma0=None):
    """ptz_krt_covariance_batch: covariance of the refined cameras cam_cur [n, 15] (world frame, as krt_solve_batch returns them)
    of the queries of `batch` (synth.RelocBatch-like: match_ptr, uv_ref, uv_cur, cam_ref, factor_type, optional point_ptr /
    pts2d / pts3d).  match_mask [n_match] uint8 (the inlier mask of krt_solve_batch_gated) and accepted [n] int32 are optional.
    Returns (cov [n, NF, NF], sigma0 [n], status [n], device_ms); parameters [fx, (fy), d1, d2, d3, (k1)], rotations in radians
    about the camera's own axes.  Entries of queries whose status is not COV_OK keep what `cov` / `sigma0` held (NaN if not given)."""
    n = batch.n_query
    nf = krt_free_dim(batch.factor_type)
    ptr = np.ascontiguousarray(batch.match_ptr, dtype=np.int64)
    uvr = np.ascontiguousarray(batch.uv_ref, dtype=np.float32)
    uvc = np.ascontiguousarray(batch.uv_cur, dtype=np.float32)
    cref = np.ascontiguousarray(batch.cam_ref, dtype=np.float64)
    ccur = np.ascontiguousarray(cam_cur, dtype=np.float64)
    pp = p2 = p3 = None
    if getattr(batch, "point_ptr", None) is not None:
        pp = np.ascontiguousarray(batch.point_ptr, dtype=np.int64)
        p2 = np.ascontiguousarray(batch.pts2d, dtype=np.float32)
        p3 = np.ascontiguousarray(batch.pts3d, dtype=np.float64)
    mk = None if match_mask is None else np.ascontiguousarray(match_mask, dtype=np.uint8)
    ac = None if accepted is None else np.ascontiguousarray(accepted, dtype=np.int32)
    if mk is not None and len(mk) != int(ptr[-1]):
        raise ValueError("match_mask must have one byte per match")
    if ac is not None and len(ac) != n:
        raise ValueError("accepted must have one entry per query")
    cov = np.full((n, nf, nf), np.nan) if cov is None else np.ascontiguousarray(cov, dtype=np.float64).reshape(n, nf, nf)
    sigma0 = np.full(n, np.nan) if sigma0 is None else np.ascontiguousarray(sigma0, dtype=np.float64).reshape(n)
    status = np.full(n, -1, dtype=np.int32)
    ms = C.c_double()
    _check(lib().ptz_krt_covariance_batch(n, _p(ptr), _p(uvr), _p(uvc), _p(pp), _p(p2), _p(p3), _p(cref), _p(ccur), int(batch.factor_type),
                                          _p(mk), _p(ac), C.c_double(pixel_sigma), int(device_id), _p(cov), _p(sigma0), _p(status),
                                          C.byref(ms)), "ptz_krt_covariance_batch")
    return cov, sigma0, status, ms.value


def krt_covariance_batch_device(n_query, d_match_ptr, d_uv_ref, d_uv_cur, d_cam_ref, d_cam_cur, d_cov, d_sigma0, d_status, factor_type=0,
                                d_point_ptr=None, d_pts2d=None, d_pts3d=None, d_match_mask=None, d_accepted=None, pixel_sigma=0.0,
                                stream=None):
    """ptz_krt_covariance_batch_device: every d_* is a device buffer (torch tensor or integer address); enqueues on `stream`
    (integer hipStream_t handle, None = default stream) and returns without synchronising -- behind krt_solve_batch_device on the
    same stream it reads the d_cam_cur and d_accepted that call wrote."""
    _check(lib().ptz_krt_covariance_batch_device(int(n_query), _dptr(d_match_ptr), _dptr(d_uv_ref), _dptr(d_uv_cur), _dptr(d_point_ptr),
                                                 _dptr(d_pts2d), _dptr(d_pts3d), _dptr(d_cam_ref), _dptr(d_cam_cur), int(factor_type),
                                                 _dptr(d_match_mask), _dptr(d_accepted), C.c_double(pixel_sigma), _dptr(d_cov),
                                                 _dptr(d_sigma0), _dptr(d_status), C.c_void_p(stream) if stream else None),
           "ptz_krt_covariance_batch_device")


def _krt_batch_arrays(batch):
    """the CSR arrays of a RelocBatch-like object: (ptr, uv_ref, uv_cur, cam_ref, point_ptr, pts2d, pts3d), the last three None
    without 2D-3D constraints"""
    ptr = np.ascontiguousarray(batch.match_ptr, dtype=np.int64)
    uvr = np.ascontiguousarray(batch.uv_ref, dtype=np.float32)
    uvc = np.ascontiguousarray(batch.uv_cur, dtype=np.float32)
    cref = np.ascontiguousarray(batch.cam_ref, dtype=np.float64)
    pp = p2 = p3 = None
    if getattr(batch, "point_ptr", None) is not None:
        pp = np.ascontiguousarray(batch.point_ptr, dtype=np.int64)
        p2 = np.ascontiguousarray(batch.pts2d, dtype=np.float32)
        p3 = np.ascontiguousarray(batch.pts3d, dtype=np.float64)
    return ptr, uvr, uvc, cref, pp, p2, p3


def krt_residuals_batch(batch, cam_cur, match_mask=None, accepted=None, lanes_per_query=0, device_id=0, out=None):
    """ptz_krt_residuals_batch: the residual report of the refined cameras cam_cur [n, 15] (world frame) of the queries of `batch`.
    Returns a dict: err_px [n_match] (-1 where the border guard skips), err3d_px [n_point] or None, rms / max / median / rms3d [n],
    count [n], device_ms.  Over the matches of match_mask [n_match] uint8 (all if None); entries of queries with accepted[q] = 0
    keep what `out` (a dict of arrays by the same names) held, NaN / -1 (count) if not given."""
    n = batch.n_query
    ptr, uvr, uvc, cref, pp, p2, p3 = _krt_batch_arrays(batch)
    ccur = np.ascontiguousarray(cam_cur, dtype=np.float64)
    mk = None if match_mask is None else np.ascontiguousarray(match_mask, dtype=np.uint8)
    ac = None if accepted is None else np.ascontiguousarray(accepted, dtype=np.int32)
    if mk is not None and len(mk) != int(ptr[-1]):
        raise ValueError("match_mask must have one byte per match")
    if ac is not None and len(ac) != n:
        raise ValueError("accepted must have one entry per query")
    out = dict(out or {})
    res = {}
    for key, size in (("err_px", int(ptr[-1])), ("rms", n), ("max", n), ("median", n), ("rms3d", n)):
        res[key] = np.full(size, np.nan) if key not in out else np.ascontiguousarray(out[key], dtype=np.float64)
    res["err3d_px"] = None
    if pp is not None:
        res["err3d_px"] = np.full(int(pp[-1]), np.nan) if "err3d_px" not in out else np.ascontiguousarray(out["err3d_px"], dtype=np.float64)
    res["count"] = np.full(n, -1, dtype=np.int32) if "count" not in out else np.ascontiguousarray(out["count"], dtype=np.int32)
    ms = C.c_double()
    _check(lib().ptz_krt_residuals_batch(n, _p(ptr), _p(uvr), _p(uvc), _p(pp), _p(p2), _p(p3), _p(cref), _p(ccur), int(batch.factor_type),
                                         _p(mk), _p(ac), int(lanes_per_query), int(device_id), _p(res["err_px"]), _p(res["err3d_px"]),
                                         _p(res["rms"]), _p(res["max"]), _p(res["median"]), _p(res["count"]), _p(res["rms3d"]),
                                         C.byref(ms)), "ptz_krt_residuals_batch")
    res["device_ms"] = ms.value
    return res


def krt_residuals_batch_device(n_query, d_match_ptr, d_uv_ref, d_uv_cur, d_cam_ref, d_cam_cur, factor_type=0, d_point_ptr=None, d_pts2d=None,
                               d_pts3d=None, d_match_mask=None, d_accepted=None, lanes_per_query=0, d_err_px=None, d_err3d_px=None,
                               d_rms=None, d_max=None, d_median=None, d_count=None, d_rms3d=None, stream=None):
    """ptz_krt_residuals_batch_device: every d_* is a device buffer (torch tensor or integer address); enqueues on `stream` (integer
    hipStream_t handle, None = default stream) and returns without synchronising.  d_median needs d_err_px."""
    _check(lib().ptz_krt_residuals_batch_device(int(n_query), _dptr(d_match_ptr), _dptr(d_uv_ref), _dptr(d_uv_cur), _dptr(d_point_ptr),
                                                _dptr(d_pts2d), _dptr(d_pts3d), _dptr(d_cam_ref), _dptr(d_cam_cur), int(factor_type),
                                                _dptr(d_match_mask), _dptr(d_accepted), int(lanes_per_query), _dptr(d_err_px),
                                                _dptr(d_err3d_px), _dptr(d_rms), _dptr(d_max), _dptr(d_median), _dptr(d_count),
                                                _dptr(d_rms3d), C.c_void_p(stream) if stream else None),
           "ptz_krt_residuals_batch_device")


def krt_trim_options(**kw) -> KrtTrimOptions:
    t = KrtTrimOptions()
    lib().ptz_krt_trim_options_default(C.byref(t))
    for k, v in kw.items():
        setattr(t, k, v)
    return t


def krt_solve_batch_trimmed(batch, max_reproj_error=100.0, match_mask=None, trim_px=4.0, k_sigma=3.0, max_rounds=8, min_keep=8, **opt):
    """ptz_krt_solve_batch_trimmed: krt_solve_batch with the sigma-clipping loop on the device (solve, report, rule, compaction, solve
    again; include/ptz_calib_amd.h).  match_mask [n_match] uint8: the universe (all matches if None).
    Returns (cam_world [n, 15], summaries, accepted [n], kept [n_match] uint8, reports (list of dicts), device_ms)."""
    o = default_options(**opt)
    t = krt_trim_options(trim_px=trim_px, k_sigma=k_sigma, max_rounds=max_rounds, min_keep=min_keep)
    n = batch.n_query
    ptr, uvr, uvc, cref, pp, p2, p3 = _krt_batch_arrays(batch)
    ccur = np.array(batch.cam_init, dtype=np.float64, order="C").copy()
    mk = None if match_mask is None else np.ascontiguousarray(match_mask, dtype=np.uint8)
    if mk is not None and len(mk) != int(ptr[-1]):
        raise ValueError("match_mask must have one byte per match")
    summ = (LmSummary * n)()
    rep = (KrtTrimReport * n)()
    acc = np.zeros(n, dtype=np.int32)
    kept = np.zeros(int(ptr[-1]), dtype=np.uint8)
    ms = C.c_double()
    _check(lib().ptz_krt_solve_batch_trimmed(n, _p(ptr), _p(uvr), _p(uvc), _p(pp), _p(p2), _p(p3), _p(cref), _p(ccur), int(batch.factor_type),
                                             C.c_double(max_reproj_error), _p(mk), C.byref(t), C.byref(o), summ, _p(acc), _p(kept), rep,
                                             C.byref(ms)), "ptz_krt_solve_batch_trimmed")
    return ccur, [s.as_dict() for s in summ], acc, kept, [r.as_dict() for r in rep], ms.value


def krt_trim_workspace_bytes(n_query, n_match) -> int:
    return int(lib().ptz_krt_trim_workspace_bytes(int(n_query), int(n_match)))


def krt_solve_batch_trimmed_device(n_query, n_match, d_match_ptr, d_uv_ref, d_uv_cur, d_cam_ref, d_cam_cur, d_summaries, d_accepted,
                                   d_workspace, workspace_bytes, factor_type=0, max_reproj_error=100.0, d_point_ptr=None, d_pts2d=None,
                                   d_pts3d=None, d_match_mask=None, d_kept=None, d_report=None, trim=None, stream=None, **opt):
    """ptz_krt_solve_batch_trimmed_device: every d_* is a device buffer (torch tensor or integer address); d_workspace needs
    krt_trim_workspace_bytes(n_query, n_match) bytes, d_report n_query * sizeof(KrtTrimReport).  Enqueues every round on `stream`
    and returns without synchronising."""
    o = default_options(**opt)
    t = trim if trim is not None else krt_trim_options()
    _check(lib().ptz_krt_solve_batch_trimmed_device(int(n_query), C.c_int64(int(n_match)), _dptr(d_match_ptr), _dptr(d_uv_ref), _dptr(d_uv_cur),
                                                    _dptr(d_point_ptr), _dptr(d_pts2d), _dptr(d_pts3d), _dptr(d_cam_ref), _dptr(d_cam_cur),
                                                    int(factor_type), C.c_double(max_reproj_error), _dptr(d_match_mask), C.byref(t),
                                                    C.byref(o), _dptr(d_summaries), _dptr(d_accepted), _dptr(d_kept), _dptr(d_report),
                                                    _dptr(d_workspace), C.c_int64(int(workspace_bytes)),
                                                    C.c_void_p(stream) if stream else None), "ptz_krt_solve_batch_trimmed_device")


def mfma_f64_peak(device_id=0):
    """Measured FP64 MFMA rate of the device in TFLOP/s (register-resident v_mfma_f64_16x16x4_f64 loop)."""
    t = C.c_double()
    _check(lib().ptz_mfma_f64_peak(int(device_id), C.byref(t)), "ptz_mfma_f64_peak")
    return t.value


def ba_solve_sharded(scenes, device_ids, **opt):
    """ptz_ba_solve_sharded: many scenes over several devices from this one process.  Returns (cams, rays, summaries)."""
    keep = []
    n = len(scenes)
    probs = (BaProblem * n)(*[_pack_problem(s, keep) for s in scenes])
    o = default_options(**opt)
    cam = np.ascontiguousarray(np.concatenate([s.cam_init for s in scenes]), dtype=np.float64)
    ray = np.ascontiguousarray(np.concatenate([s.ray_init for s in scenes]), dtype=np.float64)
    has_tlw = any(getattr(s, "tlw_init", None) is not None for s in scenes)
    tlw = np.ascontiguousarray(np.stack([getattr(s, "tlw_init", None) if getattr(s, "tlw_init", None) is not None else np.zeros(6)
                                         for s in scenes]), dtype=np.float64) if has_tlw else None
    dev = np.ascontiguousarray(device_ids, dtype=np.int32)
    summ = (LmSummary * n)()
    _check(lib().ptz_ba_solve_sharded(n, probs, _p(cam), _p(ray), _p(tlw) if tlw is not None else None, _p(dev), len(dev), C.byref(o), summ),
           "ptz_ba_solve_sharded")
    co = np.concatenate([[0], np.cumsum([s.n_cam for s in scenes])])
    ro = np.concatenate([[0], np.cumsum([s.n_ray for s in scenes])])
    cams = [cam[co[i]:co[i + 1]] for i in range(n)]
    rays = [ray[ro[i]:ro[i + 1]] for i in range(n)]
    return cams, rays, [s.as_dict() for s in summ]


def krt_solve_batch_sharded(batch, device_ids, max_reproj_error=100.0, **opt):
    """ptz_krt_solve_batch_sharded: the queries of `batch` over several devices from this one process."""
    o = default_options(**opt)
    n = batch.n_query
    ptr = np.ascontiguousarray(batch.match_ptr, dtype=np.int64)
    uvr = np.ascontiguousarray(batch.uv_ref, dtype=np.float32)
    uvc = np.ascontiguousarray(batch.uv_cur, dtype=np.float32)
    cref = np.ascontiguousarray(batch.cam_ref, dtype=np.float64)
    ccur = np.array(batch.cam_init, dtype=np.float64, order="C").copy()
    pp = p2 = p3 = None
    if getattr(batch, "point_ptr", None) is not None:
        pp = np.ascontiguousarray(batch.point_ptr, dtype=np.int64)
        p2 = np.ascontiguousarray(batch.pts2d, dtype=np.float32)
        p3 = np.ascontiguousarray(batch.pts3d, dtype=np.float64)
    dev = np.ascontiguousarray(device_ids, dtype=np.int32)
    summ = (LmSummary * n)()
    acc = np.zeros(n, dtype=np.int32)
    _check(lib().ptz_krt_solve_batch_sharded(n, _p(ptr), _p(uvr), _p(uvc), _p(pp) if pp is not None else None,
                                             _p(p2) if p2 is not None else None, _p(p3) if p3 is not None else None, _p(cref), _p(ccur),
                                             batch.factor_type, C.c_double(max_reproj_error), _p(dev), len(dev), C.byref(o), summ, _p(acc)),
           "ptz_krt_solve_batch_sharded")
    return ccur, [s.as_dict() for s in summ], acc


def hbm_bandwidth(device_id=0):
    """Measured HBM rates in GB/s: (streaming read, copy counted as read + write)."""
    r, c = C.c_double(), C.c_double()
    _check(lib().ptz_hbm_bandwidth(int(device_id), C.byref(r), C.byref(c)), "ptz_hbm_bandwidth")
    return r.value, c.value


# ---- descriptor matching: the match table from features ----------------------------------------------------------------------
class DescOptions(C.Structure):
    _fields_ = [("ratio", C.c_double), ("max_dist2", C.c_int32), ("cross_check", C.c_int32), ("min_matches", C.c_int32),
                ("device_id", C.c_int32), ("workspace_bytes", C.c_int64)]


def desc_options(**kw) -> DescOptions:
    o = DescOptions()
    lib().ptz_desc_options_default.restype = None
    lib().ptz_desc_options_default(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError(f"unknown descriptor matching option {k}")
        setattr(o, k, v)
    return o


class DescSet:
    """ptz_desc_set: the uint8 descriptors [n_feat, D] (and key points [n_feat, 2], optional) of a set of images, image m owning
    features feat_ptr[m] .. feat_ptr[m + 1], packed and resident on the device."""

    def __init__(self, feat_ptr, desc, kp_xy=None, device_id=0):
        self.feat_ptr = np.ascontiguousarray(feat_ptr, dtype=np.int64)
        d = np.ascontiguousarray(desc, dtype=np.uint8)
        if d.ndim != 2:
            raise ValueError("desc: [n_feat, D]")
        kp = None if kp_xy is None else np.ascontiguousarray(kp_xy, dtype=np.float32).reshape(-1, 2)
        if len(self.feat_ptr) < 1 or int(self.feat_ptr[-1]) != d.shape[0] or (kp is not None and len(kp) != d.shape[0]):
            raise ValueError("feat_ptr, desc and kp_xy disagree on the number of features")
        self.n_img, self.D, self.device_id = len(self.feat_ptr) - 1, int(d.shape[1]), int(device_id)
        self.handle = C.c_void_p()
        lib().ptz_desc_set_destroy.restype = None
        _check(lib().ptz_desc_set_create(self.n_img, _p(self.feat_ptr), _p(d) if d.size else None, self.D, _p(kp) if kp is not None and kp.size else None,
                                         self.device_id, C.byref(self.handle)), "ptz_desc_set_create")
        self.has_kp = kp is not None and kp.size > 0

    def close(self):
        if self.handle:
            lib().ptz_desc_set_destroy(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DescMatches:
    """ptz_desc_matches: the result of match_descriptors, resident on the device until closed."""

    def __init__(self, handle):
        self.handle = handle
        L = lib()
        L.ptz_desc_matches_n_matches.restype = C.c_int64
        L.ptz_desc_matches_device_ms.restype = C.c_double
        L.ptz_desc_matches_destroy.restype = None
        self.n_matches = int(L.ptz_desc_matches_n_matches(handle))
        self.n_pairs = int(L.ptz_desc_matches_n_pairs(handle))
        self.n_chunks = int(L.ptz_desc_matches_n_chunks(handle))
        self.device_ms = float(L.ptz_desc_matches_device_ms(handle))

    def download(self, uv=True):
        """dict of numpy arrays: match_ptr [n_pair + 1], idx_a / idx_b / dist2 [n_matches], uv_a / uv_b [n_matches, 2] (uv=True)."""
        n = self.n_matches
        ptr = np.zeros(self.n_pairs + 1, dtype=np.int64)
        ia, ib, d2 = (np.zeros(n, dtype=np.int32) for _ in range(3))
        ua, ub = (np.zeros((n, 2), dtype=np.float32) for _ in range(2)) if uv else (None, None)
        _check(lib().ptz_desc_matches_download(self.handle, _p(ptr), _p(ia), _p(ib), _p(d2), _p(ua), _p(ub)), "ptz_desc_matches_download")
        out = dict(match_ptr=ptr, idx_a=ia, idx_b=ib, dist2=d2, device_ms=self.device_ms, n_chunks=self.n_chunks)
        if uv:
            out.update(uv_a=ua, uv_b=ub)
        return out

    def device_ptrs(self):
        """Integer device addresses (match_ptr, idx_a, idx_b, dist2, uv_a, uv_b), the result's until it is closed."""
        p = [C.c_void_p() for _ in range(6)]
        _check(lib().ptz_desc_matches_device_ptrs(self.handle, *[C.byref(x) for x in p]), "ptz_desc_matches_device_ptrs")
        return tuple(x.value for x in p)

    def close(self):
        if self.handle:
            lib().ptz_desc_matches_destroy(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def match_descriptors(set_a, set_b, img_a, img_b, resident=False, **options):
    """ptz_desc_match_pairs: mutual nearest neighbours under the ratio test for the pairs (img_a[p] of set_a, img_b[p] of set_b).
    options: ratio (0.8), max_dist2 (0), cross_check (1), min_matches (0), workspace_bytes (256 MiB).  Returns the CSR arrays as a
    dict (DescMatches.download; pixels if both sets carry key points), or with resident=True the DescMatches itself."""
    ia = np.ascontiguousarray(img_a, dtype=np.int32)
    ib = np.ascontiguousarray(img_b, dtype=np.int32)
    if ia.shape != ib.shape or ia.ndim != 1:
        raise ValueError("img_a and img_b: two index lists of equal length")
    options.setdefault("device_id", set_a.device_id)
    o = desc_options(**options)
    h = C.c_void_p()
    _check(lib().ptz_desc_match_pairs(set_a.handle, set_b.handle, len(ia), _p(ia), _p(ib), C.byref(o), C.byref(h)), "ptz_desc_match_pairs")
    m = DescMatches(h)
    if resident:
        return m
    try:
        return m.download(uv=set_a.has_kp and set_b.has_kp)
    finally:
        m.close()


def match_descriptors_guided(set_a, set_b, img_a, img_b, H, found=None, radius_px=4.0, resident=False, grid=False, **options):
    """ptz_desc_match_pairs_guided: match_descriptors over the candidates pair p's homography H[p] (b ~ H a, [n_pair, 9] or
    [n_pair, 3, 3]) admits within radius_px, the error measured in B's image; found [n_pair] or None (all 1): a pair whose found is
    not 1 has no matches.  H and found may also be DEVICE buffers (torch tensors or integer addresses) on the sets' device (what MatchGate.run_device leaves,
    its stream synchronised): ptz_desc_match_pairs_guided_device.  Both sets need key points.  Returns what match_descriptors does.
    grid=True: the grid-binned kernel (ptz_desc_match_pairs_guided_grid[_device]) -- the same arrays, bit for bit."""
    ia = np.ascontiguousarray(img_a, dtype=np.int32)
    ib = np.ascontiguousarray(img_b, dtype=np.int32)
    if ia.shape != ib.shape or ia.ndim != 1:
        raise ValueError("img_a and img_b: two index lists of equal length")
    options.setdefault("device_id", set_a.device_id)
    o = desc_options(**options)
    h = C.c_void_p()
    if isinstance(H, int) or hasattr(H, "data_ptr"):
        if found is not None and not (isinstance(found, int) or hasattr(found, "data_ptr")):
            raise ValueError("a device H goes with a device found (or None)")
        name = "ptz_desc_match_pairs_guided_grid_device" if grid else "ptz_desc_match_pairs_guided_device"
        _check(getattr(lib(), name)(set_a.handle, set_b.handle, len(ia), _p(ia), _p(ib), _dptr(H), _dptr(found), C.c_double(radius_px),
                                    C.byref(o), C.byref(h)), name)
    else:
        Hh = np.ascontiguousarray(H, dtype=np.float64).reshape(-1, 9)
        fh = None if found is None else np.ascontiguousarray(found, dtype=np.int32)
        if len(Hh) != len(ia) or (fh is not None and fh.shape != ia.shape):
            raise ValueError("H: one 3 x 3 matrix per pair, found: one flag per pair")
        name = "ptz_desc_match_pairs_guided_grid" if grid else "ptz_desc_match_pairs_guided"
        _check(getattr(lib(), name)(set_a.handle, set_b.handle, len(ia), _p(ia), _p(ib), _p(Hh) if len(ia) else None,
                                    _p(fh) if fh is not None and len(ia) else None, C.c_double(radius_px), C.byref(o), C.byref(h)), name)
    m = DescMatches(h)
    if resident:
        return m
    try:
        return m.download(uv=set_a.has_kp and set_b.has_kp)
    finally:
        m.close()


def desc_dist2(set_a, img_a, set_b, img_b):
    """ptz_debug_desc_dist2: the int32 matrix d2 [n_a, n_b] of one pair, from the matcher's own tile code (tests)."""
    na = int(set_a.feat_ptr[img_a + 1] - set_a.feat_ptr[img_a])
    nb = int(set_b.feat_ptr[img_b + 1] - set_b.feat_ptr[img_b])
    out = np.zeros((na, nb), dtype=np.int32)
    _check(lib().ptz_debug_desc_dist2(set_a.handle, int(img_a), set_b.handle, int(img_b), _p(out) if out.size else None), "ptz_debug_desc_dist2")
    return out


# ---- reference shortlist (csrc/ptz_desc_shortlist.h) -------------------------------------------------------------------------------
class ShortlistOptions(C.Structure):
    _fields_ = [("max_refs", C.c_int32), ("n_probes", C.c_int32), ("min_votes", C.c_int32), ("reserved_", C.c_int32)]


def shortlist_options(**kw) -> ShortlistOptions:
    o = ShortlistOptions()
    lib().ptz_shortlist_options_default.restype = None
    lib().ptz_shortlist_options_default(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError(f"unknown shortlist option {k}")
        setattr(o, k, int(v))
    return o


def _shortlist_split(options):
    """The ShortlistOptions among one keyword dict, taken out of it (what stays are desc_options fields)"""
    sl = {k: options.pop(k) for k in ("max_refs", "n_probes", "min_votes") if k in options}
    return shortlist_options(**sl)


def desc_shortlist(ref_set, query_set, query_img=None, **options):
    """ptz_desc_shortlist: the references worth matching for each query image.  A query's first n_probes features in the index rule
    of the header vote for the references in which their nearest neighbour passes the ratio test; the max_refs references with the
    most votes (at least max(min_votes, 1)) are its shortlist, in ascending reference index.  query_img: image of query_set per query
    (default: all, in order).  options: max_refs (8), n_probes (256), min_votes (1) and the fields of desc_options (ratio,
    max_dist2).  Returns dict(shortlist [n_query, max_refs] with -1 in unused slots, n_short [n_query], votes [n_query, n_ref],
    device_ms)."""
    qi = np.arange(query_set.n_img, dtype=np.int32) if query_img is None else np.ascontiguousarray(query_img, dtype=np.int32)
    if qi.ndim != 1:
        raise ValueError("query_img: one image index per query")
    sl = _shortlist_split(options)
    options.setdefault("device_id", ref_set.device_id)
    o = desc_options(**options)
    n, R = len(qi), max(int(sl.max_refs), 1)
    out = np.full((n, R), -1, dtype=np.int32)
    ns = np.zeros(n, dtype=np.int32)
    votes = np.zeros((n, ref_set.n_img), dtype=np.int32)
    ms = C.c_double()
    _check(lib().ptz_desc_shortlist(ref_set.handle, query_set.handle, n, _p(qi) if n else None, C.byref(o), C.byref(sl), _p(out) if n else None,
                                    _p(ns) if n else None, _p(votes) if votes.size else None, C.byref(ms)), "ptz_desc_shortlist")
    return dict(shortlist=out, n_short=ns, votes=votes, device_ms=ms.value)


def desc_shortlist_workspace_bytes(ref_set, query_set, n_query, **sl) -> int:
    lib().ptz_desc_shortlist_workspace_bytes.restype = C.c_int64
    o = shortlist_options(**sl)
    return int(lib().ptz_desc_shortlist_workspace_bytes(ref_set.handle, query_set.handle, int(n_query), C.byref(o)))


def desc_shortlist_device(ref_set, query_set, n_query, d_shortlist, d_n_short, d_workspace, workspace_bytes, d_query_img=None, d_votes=None,
                          stream=None, **options):
    """ptz_desc_shortlist_device: every d_* is a device buffer (torch tensor or integer address) on the sets' device; d_workspace
    needs desc_shortlist_workspace_bytes(...) bytes.  d_query_img = None: query q is image q.  Enqueues on `stream` and returns
    without synchronising."""
    sl = _shortlist_split(options)
    options.setdefault("device_id", ref_set.device_id)
    o = desc_options(**options)
    _check(lib().ptz_desc_shortlist_device(ref_set.handle, query_set.handle, int(n_query), _dptr(d_query_img), C.byref(o), C.byref(sl),
                                           _dptr(d_shortlist), _dptr(d_n_short), _dptr(d_votes), _dptr(d_workspace),
                                           C.c_int64(int(workspace_bytes)), C.c_void_p(stream) if stream else None), "ptz_desc_shortlist_device")


# ---- relocalization assembly (csrc/ptz_reloc_assemble.h) ----------------------------------------------------------------------------
def reloc_ref_rotations(ref_cams):
    """ptz_reloc_ref_rotations (host logic only): Rodrigues of every reference camera [n_ref, 15] -> [n_ref, 9] row-major."""
    cams = np.ascontiguousarray(ref_cams, dtype=np.float64).reshape(-1, 15)
    R = np.zeros((len(cams), 9))
    _check(lib().ptz_reloc_ref_rotations(len(cams), _p(cams), _p(R)), "ptz_reloc_ref_rotations")
    return R


def reloc_assemble_workspace_bytes(n_query, n_match) -> int:
    lib().ptz_reloc_assemble_workspace_bytes.restype = C.c_int64
    return int(lib().ptz_reloc_assemble_workspace_bytes(int(n_query), C.c_int64(int(n_match))))


def reloc_assemble(match_ptr, uv_ref, uv_cur, pair_ref, query_ptr, ref_cams, query_wh, factor_type=0, max_refs=1, ref_R=None, device_id=0):
    """ptz_reloc_assemble: from the match CSR of every (reference, query) pair to the solve's inputs, for the max_refs best references
    of every query.  pair_ref [n_pair]: the reference of each pair; query_ptr [n_query + 1]: the contiguous pair list of each query;
    ref_cams [n_ref, 15]; query_wh [n_query, 2]; ref_R: reloc_ref_rotations(ref_cams) unless given.
    Returns a dict: sel_pair [n_query, K] (-1: unused slot), n_sel [n_query], match_ptr [n_query + 1], uv_ref / uv_cur [n_kept, 2],
    src [n_kept] (index in the input arrays), cam_ref / cam_init [n_query, 15], device_ms."""
    ptr = np.ascontiguousarray(match_ptr, dtype=np.int64)
    a = np.ascontiguousarray(uv_ref, dtype=np.float32).reshape(-1, 2)
    b = np.ascontiguousarray(uv_cur, dtype=np.float32).reshape(-1, 2)
    pref = np.ascontiguousarray(pair_ref, dtype=np.int32)
    qptr = np.ascontiguousarray(query_ptr, dtype=np.int64)
    cams = np.ascontiguousarray(ref_cams, dtype=np.float64).reshape(-1, 15)
    wh = np.ascontiguousarray(query_wh, dtype=np.int32).reshape(-1, 2)
    R = reloc_ref_rotations(cams) if ref_R is None else np.ascontiguousarray(ref_R, dtype=np.float64).reshape(-1, 9)
    nq, npair, nm, K = len(qptr) - 1, len(ptr) - 1, len(a), int(max_refs)
    if len(pref) != npair or len(wh) != nq or len(R) != len(cams) or len(b) != nm:
        raise ValueError("pair_ref: one reference per pair, query_wh: one size per query, ref_R: one matrix per reference")
    sel = np.full((nq, max(K, 1)), -1, dtype=np.int32)
    nsel = np.zeros(nq, dtype=np.int32)
    optr = np.zeros(nq + 1, dtype=np.int64)
    oa, ob = np.zeros((nm, 2), dtype=np.float32), np.zeros((nm, 2), dtype=np.float32)
    osrc = np.zeros(nm, dtype=np.int32)
    cref, ccur = np.zeros((nq, 15)), np.zeros((nq, 15))
    ms = C.c_double()
    _check(lib().ptz_reloc_assemble(nq, npair, len(cams), _p(ptr), _p(a) if nm else None, _p(b) if nm else None, _p(pref) if npair else None,
                                    _p(qptr), _p(cams), _p(R), _p(wh), int(factor_type), K, int(device_id), _p(sel), _p(nsel), _p(optr),
                                    _p(oa) if nm else None, _p(ob) if nm else None, _p(osrc) if nm else None, _p(cref), _p(ccur),
                                    C.byref(ms)), "ptz_reloc_assemble")
    k = int(optr[-1])
    return dict(sel_pair=sel, n_sel=nsel, match_ptr=optr, uv_ref=oa[:k], uv_cur=ob[:k], src=osrc[:k], cam_ref=cref, cam_init=ccur,
                device_ms=ms.value)


def reloc_assemble_device(n_query, n_pair, n_match, n_ref, d_match_ptr, d_uv_ref, d_uv_cur, d_pair_ref, d_query_ptr, d_ref_cams, d_ref_R,
                          d_query_wh, d_sel_pair, d_n_sel, d_out_ptr, d_out_uv_ref, d_out_uv_cur, d_out_src, d_cam_ref, d_cam_cur,
                          d_workspace, workspace_bytes, factor_type=0, max_refs=1, stream=None):
    """ptz_reloc_assemble_device: every d_* is a device buffer (torch tensor or integer address); d_workspace needs
    reloc_assemble_workspace_bytes(n_query, n_match) bytes.  Enqueues on `stream` and returns without synchronising."""
    _check(lib().ptz_reloc_assemble_device(int(n_query), int(n_pair), C.c_int64(int(n_match)), int(n_ref), _dptr(d_match_ptr), _dptr(d_uv_ref),
                                           _dptr(d_uv_cur), _dptr(d_pair_ref), _dptr(d_query_ptr), _dptr(d_ref_cams), _dptr(d_ref_R),
                                           _dptr(d_query_wh), int(factor_type), int(max_refs), _dptr(d_sel_pair), _dptr(d_n_sel),
                                           _dptr(d_out_ptr), _dptr(d_out_uv_ref), _dptr(d_out_uv_cur), _dptr(d_out_src), _dptr(d_cam_ref),
                                           _dptr(d_cam_cur), _dptr(d_workspace), C.c_int64(int(workspace_bytes)),
                                           C.c_void_p(stream) if stream else None), "ptz_reloc_assemble_device")


# ---- relocalization from a prior camera (csrc/ptz_reloc_prior.h) --------------------------------------------------------------------
class PriorOptions(C.Structure):
    _fields_ = [("radius_px", C.c_double), ("max_refs", C.c_int32), ("min_overlap", C.c_int32), ("reserved_", C.c_int32)]


def prior_options(**kw) -> PriorOptions:
    o = PriorOptions()
    lib().ptz_prior_options_default.restype = None
    lib().ptz_prior_options_default(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError(f"unknown prior option {k}")
        setattr(o, k, float(v) if k == "radius_px" else int(v))
    return o


def reloc_prior_pairs(ref_cams, prior_cams, query_wh, factor_type=0, ref_R=None, prior_R=None, device_id=0, **options):
    """ptz_reloc_prior_pairs: the references worth matching for queries whose cameras are roughly known, and the homography of every
    listed pair (b ~ H a, a in the reference image: what match_descriptors_guided takes).  ref_cams [n_ref, 15], prior_cams
    [n_query, 15], query_wh [n_query, 2]; ref_R / prior_R: reloc_ref_rotations of the respective cameras unless given.
    options: max_refs (8), min_overlap (8, of 128), radius_px (not used here).  Returns dict(shortlist [n_query, max_refs] with -1 in
    unused slots, n_short [n_query], overlap [n_query, n_ref], H_slot [n_query, max_refs, 9], device_ms)."""
    cams = np.ascontiguousarray(ref_cams, dtype=np.float64).reshape(-1, 15)
    pri = np.ascontiguousarray(prior_cams, dtype=np.float64).reshape(-1, 15)
    wh = np.ascontiguousarray(query_wh, dtype=np.int32).reshape(-1, 2)
    Rr = reloc_ref_rotations(cams) if ref_R is None else np.ascontiguousarray(ref_R, dtype=np.float64).reshape(-1, 9)
    Rq = reloc_ref_rotations(pri) if prior_R is None else np.ascontiguousarray(prior_R, dtype=np.float64).reshape(-1, 9)
    if len(wh) != len(pri) or len(Rr) != len(cams) or len(Rq) != len(pri):
        raise ValueError("query_wh: one size per query, ref_R / prior_R: one matrix per camera")
    o = prior_options(**options)
    n, R = len(pri), max(int(o.max_refs), 1)
    sl = np.full((n, R), -1, dtype=np.int32)
    ns = np.zeros(n, dtype=np.int32)
    ov = np.zeros((n, len(cams)), dtype=np.int32)
    Hs = np.zeros((n, R, 9))
    ms = C.c_double()
    _check(lib().ptz_reloc_prior_pairs(len(cams), _p(cams) if len(cams) else None, _p(Rr) if len(cams) else None, n, _p(pri) if n else None,
                                       _p(Rq) if n else None, _p(wh) if n else None, int(factor_type), C.byref(o), int(device_id),
                                       _p(sl) if n else None, _p(ns) if n else None, _p(ov) if ov.size else None, _p(Hs) if n else None,
                                       C.byref(ms)), "ptz_reloc_prior_pairs")
    return dict(shortlist=sl, n_short=ns, overlap=ov, H_slot=Hs, device_ms=ms.value)


def reloc_prior_pairs_device(n_ref, d_ref_cams, d_ref_R, n_query, d_prior_cams, d_prior_R, d_query_wh, d_shortlist, d_n_short, d_overlap,
                             d_H_slot, factor_type=0, stream=None, **options):
    """ptz_reloc_prior_pairs_device: every d_* is a device buffer (torch tensor or integer address), all required.  Enqueues on
    `stream` and returns without synchronising."""
    o = prior_options(**options)
    _check(lib().ptz_reloc_prior_pairs_device(int(n_ref), _dptr(d_ref_cams), _dptr(d_ref_R), int(n_query), _dptr(d_prior_cams), _dptr(d_prior_R),
                                              _dptr(d_query_wh), int(factor_type), C.byref(o), _dptr(d_shortlist), _dptr(d_n_short),
                                              _dptr(d_overlap), _dptr(d_H_slot), C.c_void_p(stream) if stream else None),
           "ptz_reloc_prior_pairs_device")


# ---- landmark map (csrc/ptz_landmark.h) ---------------------------------------------------------------------------------------------
class _BorrowedDescSet:
    """The map's descriptor set as match_descriptors takes it: one image of n_lm features, owned by the map."""

    def __init__(self, handle, D, device_id):
        self.handle, self.D, self.device_id, self.n_img, self.has_kp = handle, D, device_id, 1, True


class LandmarkMap:
    """ptz_landmark_map: one unit ray and one aggregated descriptor per track of the reference images.  ref_set: the references'
    DescSet with key points (image m is camera m of ref_cams [n_ref, 15]); tracks as CSR: trk_ptr [n_track + 1], trk_img / trk_feat
    (the feature's index inside its image).  A track becomes a landmark with at least min_views valid views and a finite ray."""

    def __init__(self, ref_set, ref_cams, trk_ptr, trk_img, trk_feat, factor_type=0, min_views=1, device_id=None):
        self.ref_cams = np.ascontiguousarray(ref_cams, dtype=np.float64).reshape(-1, 15)
        ptr = np.ascontiguousarray(trk_ptr, dtype=np.int64)
        img = np.ascontiguousarray(trk_img, dtype=np.int32)
        feat = np.ascontiguousarray(trk_feat, dtype=np.int32)
        if len(ptr) < 1 or len(img) != len(feat) or (len(ptr) > 1 and int(ptr[-1]) != len(img)):
            raise ValueError("trk_ptr, trk_img and trk_feat disagree on the number of views")
        self.device_id = ref_set.device_id if device_id is None else int(device_id)
        self.D, self.factor_type = ref_set.D, int(factor_type)
        self.handle = C.c_void_p()
        L = lib()
        L.ptz_landmark_map_destroy.restype = None
        L.ptz_landmark_map_build_ms.restype = C.c_double
        L.ptz_landmark_map_desc_set.restype = C.c_void_p
        _check(L.ptz_landmark_map_create(ref_set.handle, _p(self.ref_cams), len(self.ref_cams), len(ptr) - 1, _p(ptr), _p(img) if len(img) else None,
                                         _p(feat) if len(feat) else None, self.factor_type, int(min_views), self.device_id, C.byref(self.handle)),
               "ptz_landmark_map_create")
        self.n_landmarks = int(L.ptz_landmark_map_n_landmarks(self.handle))
        self.build_ms = float(L.ptz_landmark_map_build_ms(self.handle))

    @classmethod
    def from_tracks(cls, ref_set, ref_cams, tracks, factor_type=0, min_views=1):
        """ptz_landmark_map_create_from_tracks: the same map from the device arrays of a Tracks of ref_set; lm_track indexes its order."""
        self = cls.__new__(cls)
        self.ref_cams = np.ascontiguousarray(ref_cams, dtype=np.float64).reshape(-1, 15)
        self.device_id, self.D, self.factor_type = ref_set.device_id, ref_set.D, int(factor_type)
        self.handle = C.c_void_p()
        L = lib()
        L.ptz_landmark_map_destroy.restype = None
        L.ptz_landmark_map_build_ms.restype = C.c_double
        L.ptz_landmark_map_desc_set.restype = C.c_void_p
        _check(L.ptz_landmark_map_create_from_tracks(ref_set.handle, _p(self.ref_cams), len(self.ref_cams), tracks.handle, self.factor_type,
                                                     int(min_views), C.byref(self.handle)), "ptz_landmark_map_create_from_tracks")
        self.n_landmarks = int(L.ptz_landmark_map_n_landmarks(self.handle))
        self.build_ms = float(L.ptz_landmark_map_build_ms(self.handle))
        return self

    def arrays(self):
        """dict of numpy arrays: lm_track / lm_home / lm_views [n_lm], lm_ray [n_lm, 3], lm_desc [n_lm, D]."""
        n = self.n_landmarks
        trk, home, views = (np.zeros(n, dtype=np.int32) for _ in range(3))
        ray, desc = np.zeros((n, 3)), np.zeros((n, self.D), dtype=np.uint8)
        _check(lib().ptz_landmark_map_download(self.handle, _p(trk), _p(ray), _p(home), _p(views), _p(desc)), "ptz_landmark_map_download")
        return dict(lm_track=trk, lm_ray=ray, lm_home=home, lm_views=views, lm_desc=desc)

    def desc_set(self):
        """The map's descriptors as the set_a of match_descriptors (img_a = 0); the map's until it is closed."""
        return _BorrowedDescSet(C.c_void_p(lib().ptz_landmark_map_desc_set(self.handle)), self.D, self.device_id)

    def home_set(self):
        """The HOME SET (csrc/ptz_landmark_shortlist.h) as a set of n_ref images: image r holds the landmarks with home r in
        ascending landmark index.  Built on the first request; the map's until it is closed."""
        lib().ptz_landmark_map_home_set.restype = C.c_void_p
        h = lib().ptz_landmark_map_home_set(self.handle)
        if not h:
            raise PtzError(-3, "ptz_landmark_map_home_set")
        return _ViewDescSet(C.c_void_p(h), self.D, self.device_id, self.home_groups()["home_ptr"])

    def home_groups(self):
        """dict of home_ptr [n_ref + 1], home_lm [n_lm]: the landmarks of home r are home_lm[home_ptr[r]:home_ptr[r + 1]]."""
        ptr, lm = np.zeros(len(self.ref_cams) + 1, dtype=np.int64), np.zeros(self.n_landmarks, dtype=np.int32)
        _check(lib().ptz_landmark_map_home_groups(self.handle, _p(ptr), _p(lm) if len(lm) else None), "ptz_landmark_map_home_groups")
        return dict(home_ptr=ptr, home_lm=lm)

    def close(self):
        if self.handle:
            lib().ptz_landmark_map_destroy(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Tracks:
    """ptz_tracks: the feature tracks of a match table, resident on the device until closed (csrc/ptz_tracks.h): tracks in
    ascending smallest node, the views of a track in ascending image."""

    def __init__(self, handle):
        self.handle = handle
        L = lib()
        L.ptz_tracks_destroy.restype = None
        L.ptz_tracks_n_views.restype = C.c_int64
        L.ptz_tracks_device_ms.restype = C.c_double
        self.n_tracks = int(L.ptz_tracks_n_tracks(handle))
        self.n_views = int(L.ptz_tracks_n_views(handle))
        self.device_ms = float(L.ptz_tracks_device_ms(handle))

    def download(self):
        """(trk_ptr [n_track + 1], trk_img, trk_feat, trk_node [n_view], trk_uv [n_view, 2])."""
        ptr = np.zeros(self.n_tracks + 1, dtype=np.int64)
        img, feat, node = (np.zeros(self.n_views, dtype=np.int32) for _ in range(3))
        uv = np.zeros((self.n_views, 2), dtype=np.float32)
        _check(lib().ptz_tracks_download(self.handle, _p(ptr), _p(img), _p(feat), _p(node), _p(uv)), "ptz_tracks_download")
        return ptr, img, feat, node, uv

    def counts(self):
        """int64 [4]: matched nodes, components, components dropped for a repeated image, components dropped as short."""
        c = np.zeros(4, dtype=np.int64)
        _check(lib().ptz_tracks_counts(self.handle, _p(c)), "ptz_tracks_counts")
        return c

    def device_ptrs(self):
        """Integer device addresses (trk_ptr, trk_img, trk_feat, trk_node, trk_uv), the tracks' until they are closed."""
        p = [C.c_void_p() for _ in range(5)]
        _check(lib().ptz_tracks_device_ptrs(self.handle, *[C.byref(x) for x in p]), "ptz_tracks_device_ptrs")
        return tuple(x.value for x in p)

    def close(self):
        if self.handle:
            lib().ptz_tracks_destroy(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def tracks_build(feat_ptr, img_a, img_b, match_ptr, idx_a, idx_b, min_len=2, device_id=0) -> Tracks:
    """ptz_tracks_build: the tracks of the match table (img_a / img_b [n_pair], match_ptr [n_pair + 1], idx_a / idx_b [n_match]) over
    the images of feat_ptr [n_img + 1], from host arrays.  An index out of range is PTZ_EINVAL."""
    fp = np.ascontiguousarray(feat_ptr, dtype=np.int64)
    ia, ib = np.ascontiguousarray(img_a, dtype=np.int32), np.ascontiguousarray(img_b, dtype=np.int32)
    ptr = np.ascontiguousarray(match_ptr, dtype=np.int64)
    xa, xb = np.ascontiguousarray(idx_a, dtype=np.int32), np.ascontiguousarray(idx_b, dtype=np.int32)
    if len(fp) < 1 or ia.shape != ib.shape or xa.shape != xb.shape or (len(ia) and (len(ptr) != len(ia) + 1 or int(ptr[-1]) != len(xa))):
        raise ValueError("feat_ptr, the pair lists, match_ptr and the index lists disagree on their extents")
    h = C.c_void_p()
    _check(lib().ptz_tracks_build(len(fp) - 1, _p(fp), len(ia), _p(ia) if len(ia) else None, _p(ib) if len(ib) else None,
                                  _p(ptr) if len(ia) else None, _p(xa) if len(xa) else None, _p(xb) if len(xb) else None, int(min_len),
                                  int(device_id), C.byref(h)), "ptz_tracks_build")
    return Tracks(h)


def tracks_from_matches(desc_set, matches, img_a, img_b, min_len=2) -> Tracks:
    """ptz_tracks_from_matches: the tracks of a resident table (match_descriptors(set, set, img_a, img_b, resident=True)) of the set's
    images among themselves; nothing but the sizes comes back to the host."""
    ia, ib = np.ascontiguousarray(img_a, dtype=np.int32), np.ascontiguousarray(img_b, dtype=np.int32)
    if ia.shape != ib.shape or ia.ndim != 1 or len(ia) != matches.n_pairs:
        raise ValueError("img_a and img_b: the table's pair lists")
    h = C.c_void_p()
    _check(lib().ptz_tracks_from_matches(desc_set.handle, matches.handle, _p(ia) if len(ia) else None, _p(ib) if len(ib) else None, int(min_len),
                                         C.byref(h)), "ptz_tracks_from_matches")
    return Tracks(h)


def tracks_workspace_bytes(n_feat) -> int:
    lib().ptz_tracks_workspace_bytes.restype = C.c_int64
    return int(lib().ptz_tracks_workspace_bytes(C.c_int64(n_feat)))


def tracks_build_device(n_img, d_feat_ptr, n_feat, d_kp, n_pair, d_img_a, d_img_b, d_match_ptr, n_match, d_idx_a, d_idx_b, min_len, d_trk_ptr,
                        d_trk_img, d_trk_feat, d_trk_node, d_trk_uv, d_sizes, d_workspace, workspace_bytes, stream=None):
    """ptz_tracks_build_device: raw device buffers (torch tensors or addresses), enqueued on `stream`, nothing waited for."""
    _check(lib().ptz_tracks_build_device(int(n_img), _dptr(d_feat_ptr), C.c_int64(n_feat), _dptr(d_kp), int(n_pair), _dptr(d_img_a), _dptr(d_img_b),
                                         _dptr(d_match_ptr), C.c_int64(n_match), _dptr(d_idx_a), _dptr(d_idx_b), int(min_len), _dptr(d_trk_ptr),
                                         _dptr(d_trk_img), _dptr(d_trk_feat), _dptr(d_trk_node), _dptr(d_trk_uv), _dptr(d_sizes),
                                         _dptr(d_workspace), C.c_int64(workspace_bytes), _dptr(stream)), "ptz_tracks_build_device")


def landmark_assemble_workspace_bytes(n_query, n_match) -> int:
    lib().ptz_landmark_assemble_workspace_bytes.restype = C.c_int64
    return int(lib().ptz_landmark_assemble_workspace_bytes(int(n_query), C.c_int64(int(n_match))))


def landmark_assemble(lmap, match_ptr, idx_a, uv_b, query_wh, ref_R=None):
    """ptz_landmark_assemble: from the match CSR of the (map, query) pairs -- match_ptr [n_query + 1], idx_a (landmark index), uv_b
    (query pixel) -- to the solve's inputs.  Returns a dict: anchor_ref [n_query] (-1: no match votes), match_ptr [n_query + 1],
    uv_ref / uv_cur [n_kept, 2], src [n_kept] (index in the input arrays), cam_ref / cam_init [n_query, 15], device_ms."""
    ptr = np.ascontiguousarray(match_ptr, dtype=np.int64)
    ia = np.ascontiguousarray(idx_a, dtype=np.int32)
    b = np.ascontiguousarray(uv_b, dtype=np.float32).reshape(-1, 2)
    wh = np.ascontiguousarray(query_wh, dtype=np.int32).reshape(-1, 2)
    R = reloc_ref_rotations(lmap.ref_cams) if ref_R is None else np.ascontiguousarray(ref_R, dtype=np.float64).reshape(-1, 9)
    nq, nm = len(ptr) - 1, len(ia)
    if len(wh) != nq or len(b) != nm or len(R) != len(lmap.ref_cams):
        raise ValueError("query_wh: one size per query, uv_b: one pixel per match, ref_R: one matrix per reference")
    anchor = np.full(nq, -1, dtype=np.int32)
    optr = np.zeros(nq + 1, dtype=np.int64)
    oa, ob = np.zeros((nm, 2), dtype=np.float32), np.zeros((nm, 2), dtype=np.float32)
    osrc = np.zeros(nm, dtype=np.int32)
    cref, ccur = np.zeros((nq, 15)), np.zeros((nq, 15))
    ms = C.c_double()
    _check(lib().ptz_landmark_assemble(lmap.handle, nq, _p(ptr), _p(ia) if nm else None, _p(b) if nm else None, _p(lmap.ref_cams), _p(R), _p(wh),
                                       lmap.factor_type, _p(anchor), _p(optr), _p(oa) if nm else None, _p(ob) if nm else None,
                                       _p(osrc) if nm else None, _p(cref), _p(ccur), C.byref(ms)), "ptz_landmark_assemble")
    k = int(optr[-1])
    return dict(anchor_ref=anchor, match_ptr=optr, uv_ref=oa[:k], uv_cur=ob[:k], src=osrc[:k], cam_ref=cref, cam_init=ccur, device_ms=ms.value)


def landmark_assemble_device(lmap, n_query, n_match, d_match_ptr, d_idx_a, d_uv_b, d_ref_cams, d_ref_R, d_query_wh, d_anchor_ref, d_out_ptr,
                             d_out_uv_ref, d_out_uv_cur, d_out_src, d_cam_ref, d_cam_cur, d_workspace, workspace_bytes, stream=None):
    """ptz_landmark_assemble_device: every d_* is a device buffer (torch tensor or integer address); d_workspace needs
    landmark_assemble_workspace_bytes(n_query, n_match) bytes.  Enqueues on `stream` and returns without synchronising."""
    _check(lib().ptz_landmark_assemble_device(lmap.handle, int(n_query), C.c_int64(int(n_match)), _dptr(d_match_ptr), _dptr(d_idx_a), _dptr(d_uv_b),
                                              _dptr(d_ref_cams), _dptr(d_ref_R), _dptr(d_query_wh), lmap.factor_type, _dptr(d_anchor_ref),
                                              _dptr(d_out_ptr), _dptr(d_out_uv_ref), _dptr(d_out_uv_cur), _dptr(d_out_src), _dptr(d_cam_ref),
                                              _dptr(d_cam_cur), _dptr(d_workspace), C.c_int64(int(workspace_bytes)),
                                              C.c_void_p(stream) if stream else None), "ptz_landmark_assemble_device")


# ---- landmark view: the map from a prior camera (csrc/ptz_landmark_prior.h) ----------------------------------------------------------
class LandmarkPriorOptions(C.Structure):
    _fields_ = [("radius_px", C.c_double), ("max_view_bytes", C.c_int64)]


def landmark_prior_options(**kw) -> LandmarkPriorOptions:
    o = LandmarkPriorOptions()
    lib().ptz_landmark_prior_options_default.restype = None
    lib().ptz_landmark_prior_options_default(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError(f"unknown landmark prior option {k}")
        setattr(o, k, float(v) if k == "radius_px" else int(v))
    return o


class _ViewDescSet(_BorrowedDescSet):
    """A view's gathered descriptor set as match_descriptors_guided takes it: image q holds the landmarks query q sees."""

    def __init__(self, handle, D, device_id, feat_ptr):
        super().__init__(handle, D, device_id)
        self.feat_ptr, self.n_img = feat_ptr, len(feat_ptr) - 1


class LandmarkView:
    """ptz_landmark_view: per query the landmarks of a map its prior camera sees (ascending landmark index) and their predicted
    pixels, with their descriptors gathered into a set of n_query images.  Made by landmark_visible."""

    def __init__(self, handle, n_query, D, device_id):
        self.handle, self.n_query, self.D, self.device_id = handle, int(n_query), int(D), int(device_id)
        L = lib()
        L.ptz_landmark_view_n_visible.restype = C.c_int64
        L.ptz_landmark_view_device_ms.restype = C.c_double
        L.ptz_landmark_view_desc_set.restype = C.c_void_p
        L.ptz_landmark_view_destroy.restype = None
        self.n_visible = int(L.ptz_landmark_view_n_visible(handle))
        self.device_ms = float(L.ptz_landmark_view_device_ms(handle))
        self.kind = int(L.ptz_landmark_view_kind(handle))  # VIEW_PRIOR or VIEW_HOMES

    def arrays(self):
        """dict of numpy arrays: vis_ptr [n_query + 1], vis_lm [n_vis], vis_uv [n_vis, 2]."""
        n = self.n_visible
        ptr, lm, uv = np.zeros(self.n_query + 1, dtype=np.int64), np.zeros(n, dtype=np.int32), np.zeros((n, 2), dtype=np.float32)
        _check(lib().ptz_landmark_view_download(self.handle, _p(ptr), _p(lm) if n else None, _p(uv) if n else None), "ptz_landmark_view_download")
        return dict(vis_ptr=ptr, vis_lm=lm, vis_uv=uv)

    def desc_set(self):
        """The gathered set as the set_a of match_descriptors_guided (img_a = q, H = identity); the view's until it is closed."""
        return _ViewDescSet(C.c_void_p(lib().ptz_landmark_view_desc_set(self.handle)), self.D, self.device_id, self.arrays()["vis_ptr"])

    def device_ptrs(self):
        """Integer device addresses (vis_ptr, vis_lm, vis_uv), the view's until it is closed."""
        p = [C.c_void_p() for _ in range(3)]
        _check(lib().ptz_landmark_view_device_ptrs(self.handle, *[C.byref(x) for x in p]), "ptz_landmark_view_device_ptrs")
        return tuple(x.value for x in p)

    def close(self):
        if self.handle:
            lib().ptz_landmark_view_destroy(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def landmark_visible(lmap, prior_cams, query_wh, factor_type=0, prior_R=None, **opt):
    """ptz_landmark_visible: the LandmarkView of a prior camera per query -- prior_cams [n_query, 15], query_wh [n_query, 2]; prior_R:
    reloc_ref_rotations of the priors unless given.  opt: radius_px (40), max_view_bytes (2 GiB)."""
    pri = np.ascontiguousarray(prior_cams, dtype=np.float64).reshape(-1, 15)
    wh = np.ascontiguousarray(query_wh, dtype=np.int32).reshape(-1, 2)
    o = landmark_prior_options(**opt)
    if len(wh) != len(pri):
        raise ValueError("query_wh: one size per query")
    n = len(pri)
    if prior_R is None:
        R = reloc_ref_rotations(pri)
    else:
        R = np.ascontiguousarray(prior_R, dtype=np.float64).reshape(-1, 9)
    if len(R) != n:
        raise ValueError("prior_R: one matrix per prior")
    h = C.c_void_p()
    _check(lib().ptz_landmark_visible(lmap.handle, n, _p(pri) if n else None, _p(R) if n else None, _p(wh) if n else None, int(factor_type),
                                      C.byref(o), C.byref(h)), "ptz_landmark_visible")
    return LandmarkView(h, n, lmap.D, lmap.device_id)


# ---- landmark shortlist: probe votes for the map's homes (csrc/ptz_landmark_shortlist.h) --------------------------------------------
VIEW_PRIOR, VIEW_HOMES = 0, 1


def landmark_shortlist(lmap, query_set, query_img=None, **options):
    """ptz_landmark_shortlist: desc_shortlist with the map's home set as the reference set -- the homes (cells of the map) worth
    matching for each query image.  Options and the returned dict are desc_shortlist's; shortlist holds home indices."""
    qi = np.arange(query_set.n_img, dtype=np.int32) if query_img is None else np.ascontiguousarray(query_img, dtype=np.int32)
    if qi.ndim != 1:
        raise ValueError("query_img: one image index per query")
    sl = _shortlist_split(options)
    options.setdefault("device_id", lmap.device_id)
    o = desc_options(**options)
    n, R, n_ref = len(qi), max(int(sl.max_refs), 1), len(lmap.ref_cams)
    out = np.full((n, R), -1, dtype=np.int32)
    ns = np.zeros(n, dtype=np.int32)
    votes = np.zeros((n, n_ref), dtype=np.int32)
    ms = C.c_double()
    _check(lib().ptz_landmark_shortlist(lmap.handle, query_set.handle, n, _p(qi) if n else None, C.byref(o), C.byref(sl), _p(out) if n else None,
                                        _p(ns) if n else None, _p(votes) if votes.size else None, C.byref(ms)), "ptz_landmark_shortlist")
    return dict(shortlist=out, n_short=ns, votes=votes, device_ms=ms.value)


def landmark_shortlist_workspace_bytes(lmap, query_set, n_query, **sl) -> int:
    lib().ptz_landmark_shortlist_workspace_bytes.restype = C.c_int64
    o = shortlist_options(**sl)
    return int(lib().ptz_landmark_shortlist_workspace_bytes(lmap.handle, query_set.handle, int(n_query), C.byref(o)))


def landmark_shortlist_device(lmap, query_set, n_query, d_shortlist, d_n_short, d_workspace, workspace_bytes, d_query_img=None, d_votes=None,
                              stream=None, **options):
    """ptz_landmark_shortlist_device: desc_shortlist_device over the map's home set; d_workspace needs
    landmark_shortlist_workspace_bytes(...) bytes.  Enqueues on `stream` and returns without synchronising."""
    sl = _shortlist_split(options)
    options.setdefault("device_id", lmap.device_id)
    o = desc_options(**options)
    _check(lib().ptz_landmark_shortlist_device(lmap.handle, query_set.handle, int(n_query), _dptr(d_query_img), C.byref(o), C.byref(sl),
                                               _dptr(d_shortlist), _dptr(d_n_short), _dptr(d_votes), _dptr(d_workspace),
                                               C.c_int64(int(workspace_bytes)), C.c_void_p(stream) if stream else None),
           "ptz_landmark_shortlist_device")


def landmark_view_from_homes(lmap, shortlist, max_view_bytes=2 << 30, device=False, n_query=None, max_refs=None, stream=None):
    """ptz_landmark_view_from_homes: the LandmarkView (kind VIEW_HOMES) of per-query lists of homes -- shortlist [n_query, R] with -1
    in unused slots: every landmark whose home is on a query's list, in ascending landmark index; vis_uv is zeros.
    device=True: ptz_landmark_view_from_homes_device -- shortlist is a device buffer (torch tensor or integer address) of
    [n_query, max_refs] int32 written on `stream`; entries out of range are ignored there, and a ValueError / PTZ_EINVAL here."""
    h = C.c_void_p()
    if device:
        n, R = int(n_query), int(max_refs)
        _check(lib().ptz_landmark_view_from_homes_device(lmap.handle, n, R, _dptr(shortlist), C.c_int64(int(max_view_bytes)),
                                                         C.c_void_p(stream) if stream else None, C.byref(h)), "ptz_landmark_view_from_homes_device")
    else:
        sl = np.ascontiguousarray(shortlist, dtype=np.int32)
        if sl.ndim != 2 or sl.shape[1] < 1:
            raise ValueError("shortlist: [n_query, R] with R >= 1")
        n, R = sl.shape
        _check(lib().ptz_landmark_view_from_homes(lmap.handle, n, R, _p(sl) if n else None, C.c_int64(int(max_view_bytes)), C.byref(h)),
               "ptz_landmark_view_from_homes")
    return LandmarkView(h, n, lmap.D, lmap.device_id)


def landmark_visible_workspace_bytes(n_lm, n_query) -> int:
    lib().ptz_landmark_visible_workspace_bytes.restype = C.c_int64
    return int(lib().ptz_landmark_visible_workspace_bytes(int(n_lm), int(n_query)))


def landmark_visible_device(n_lm, d_ray, n_query, d_prior_cams, d_prior_R, d_query_wh, d_vis_ptr, d_vis_lm, d_vis_uv, capacity, d_workspace,
                            workspace_bytes, factor_type=0, radius_px=40.0, stream=None):
    """ptz_landmark_visible_device: every d_* is a device buffer (torch tensor or integer address); d_ray [n_lm, 3] are arbitrary
    rays; d_vis_ptr [n_query + 1] is always complete, d_vis_lm / d_vis_uv take at most `capacity` entries; d_workspace needs
    landmark_visible_workspace_bytes(n_lm, n_query) bytes.  Enqueues on `stream` and returns without synchronising."""
    _check(lib().ptz_landmark_visible_device(int(n_lm), _dptr(d_ray), int(n_query), _dptr(d_prior_cams), _dptr(d_prior_R), _dptr(d_query_wh),
                                             int(factor_type), C.c_double(float(radius_px)), _dptr(d_vis_ptr), _dptr(d_vis_lm), _dptr(d_vis_uv),
                                             C.c_int64(int(capacity)), _dptr(d_workspace), C.c_int64(int(workspace_bytes)),
                                             C.c_void_p(stream) if stream else None), "ptz_landmark_visible_device")


# ---- the resident serving loop (ptz_relocalizer_*) ---------------------------------------------------------------------------------
class RelocOptions(C.Structure):
    _fields_ = [("match", DescOptions), ("guided_radius", C.c_double), ("ransac_thresh", C.c_double), ("min_inliers", C.c_int32),
                ("inlier_matches", C.c_int32), ("trim", C.c_int32), ("uncertainty", C.c_int32), ("trim_options", KrtTrimOptions),
                ("max_refs", C.c_int32), ("factor_type", C.c_int32), ("max_reproj_error", C.c_double), ("gate_max_pair_matches", C.c_int32),
                ("guided_grid", C.c_int32), ("lm", LmOptions)]


class RelocResult(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("cam", "accepted", "summaries", "sel_ref", "n_sel", "n_matches", "n_inliers", "trim_report", "cov",
                                          "sigma0", "cov_status")] + [("stage_ms", C.c_double * 6)]


class ShortlistResult(C.Structure):
    _fields_ = [("shortlist", C.c_void_p), ("n_short", C.c_void_p), ("votes", C.c_void_p), ("shortlist_ms", C.c_double)]


class PriorResult(C.Structure):
    _fields_ = [("shortlist", C.c_void_p), ("n_short", C.c_void_p), ("overlap", C.c_void_p), ("prior_ms", C.c_double)]


class LandmarkViewResult(C.Structure):
    _fields_ = [("n_visible", C.c_void_p), ("view_ms", C.c_double)]


class Relocalizer:
    """ptz_relocalizer: relocalization from features with the references resident on the device.  ref_set: a DescSet with key points
    (kept alive by this object), ref_cams [n_ref, 15] (image m of the set is camera m)."""

    def __init__(self, ref_set, ref_cams, device_id=None):
        self.ref_set = ref_set
        self.ref_cams = np.ascontiguousarray(ref_cams, dtype=np.float64).reshape(-1, 15)
        self.device_id = ref_set.device_id if device_id is None else int(device_id)
        self.handle = C.c_void_p()
        lib().ptz_relocalizer_destroy.restype = None
        lib().ptz_relocalizer_n_matches.restype = C.c_int64
        _check(lib().ptz_relocalizer_create(ref_set.handle, _p(self.ref_cams), len(self.ref_cams), self.device_id, C.byref(self.handle)),
               "ptz_relocalizer_create")

    def run(self, query_set, query_wh, max_refs=1, factor_type=0, guided_radius=0.0, ransac_thresh=4.0, min_inliers=6, inlier_matches=False,
            trim=None, uncertainty=False, max_reproj_error=100.0, gate_max_pair_matches=2048, match=None, shortlist=None, prior=None, guided_grid=False, landmarks=None, landmark_prior=None,
            landmark_shortlist=None, gate_model=0, gate_iters=128, **lm):
        """One run over the images of query_set (a DescSet with key points; query_wh [n_query, 2]).  trim: None, or a dict of
        krt_trim_options fields; match: a dict of desc_options fields; lm: LmOptions fields.  Returns a dict of per-query numpy
        arrays: cam, accepted, summaries (list of dicts), sel_ref [n, K], n_sel, n_matches, n_inliers, trim_report (list of dicts or
        None), cov / sigma0 / cov_status (or None), stage_ms [6].
        shortlist: None (every reference of every query), or a dict of shortlist_options fields (max_refs, n_probes, min_votes; {} for
        the defaults): ptz_relocalizer_run_shortlisted -- only the references the vote pass keeps are matched, and the result gains
        shortlist [n, R], n_short [n], votes [n, n_ref] and shortlist_ms.
        prior: None, or a dict with cams [n, 15] (a prior camera per query) and optionally radius_px (40), max_refs (8), min_overlap
        (8): ptz_relocalizer_run_tracked -- the references that overlap the prior are matched under the predicted homography alone
        (no dense pass; guided_radius is ignored), the solve starts from the prior, and the gate on the assembled query is always on.
        The result gains shortlist [n, R], n_short [n], overlap [n, n_ref] and prior_ms.  Exclusive with shortlist.
        guided_grid: every guided pass of the run (guided_radius > 0, prior=) goes through the grid-binned kernel: the same outputs.
        landmarks: None, or a LandmarkMap built from this relocalizer's references: ptz_relocalizer_run_landmarks -- every query is
        matched against the map's one image, not against reference images; max_refs is ignored, sel_ref [n, 1] is the anchor and
        n_sel is 0 or 1; guided_radius > 0 is PTZ_EUNSUPPORTED.  Exclusive with shortlist and prior.
        landmark_prior (with landmarks): None, or a dict with cams [n, 15] (a prior camera per query) and optionally radius_px (40),
        max_view_bytes: ptz_relocalizer_run_landmarks_tracked -- only the landmarks the prior sees are matched, by the guided matcher
        around their predicted pixels (guided_grid selects the kernel; guided_radius is ignored), the solve starts from the prior and
        the gate on the assembled query is always on.  The result gains n_visible [n] and view_ms; view() downloads the view.
        landmark_shortlist (with landmarks): None, or a dict of shortlist_options fields (max_refs, n_probes, min_votes; {} for the
        defaults): ptz_relocalizer_run_landmarks_shortlisted -- probe features vote for the map's homes, and the dense matcher sees
        only the landmarks of the listed homes; the gate is not forced on.  The result gains shortlist [n, R] (home indices),
        n_short [n], votes [n, n_ref], votes_ms, n_visible [n] and view_ms; view() downloads the view.  Exclusive with
        landmark_prior, shortlist and prior.
        gate_model: 0, the homography gate on the assembled queries; 1, the rotation-and-focal gate (RotFocalGate) with gate_iters
        samples (1 .. 4096), in every kind of run; set on the relocalizer before the run (ptz_relocalizer_set_gate_model) -- gate_max_pair_matches does not bound a query then, and gate_models() downloads f and R."""
        if landmark_shortlist is not None and landmarks is None:
            raise ValueError("landmark_shortlist= votes for the homes of a map: it needs landmarks=")
        if landmark_shortlist is not None and landmark_prior is not None:
            raise ValueError("landmark_shortlist= and landmark_prior= are two ways to pick a query's landmarks: give one")
        if landmark_prior is not None and landmarks is None:
            raise ValueError("landmark_prior= predicts the landmarks of a map: it needs landmarks=")
        if prior is not None and shortlist is not None:
            raise ValueError("prior= and shortlist= are two ways to pick a query's references: give one")
        if landmarks is not None and (prior is not None or shortlist is not None):
            raise ValueError("landmarks= matches against the map, not against reference images: exclusive with shortlist= and prior=")
        if landmarks is not None:
            max_refs = 1
        wh = np.ascontiguousarray(query_wh, dtype=np.int32).reshape(-1, 2)
        n, K = len(wh), int(max_refs)
        o = RelocOptions()
        lib().ptz_reloc_options_default(C.byref(o))
        for k, v in dict(match or {}, device_id=self.device_id).items():
            setattr(o.match, k, v)
        for k, v in (trim or {}).items():
            setattr(o.trim_options, k, v)
        for k, v in lm.items():
            setattr(o.lm, k, v)
        o.guided_radius, o.ransac_thresh, o.min_inliers, o.inlier_matches = float(guided_radius), float(ransac_thresh), int(min_inliers), int(bool(inlier_matches))
        o.trim, o.uncertainty, o.max_refs, o.factor_type = int(trim is not None), int(bool(uncertainty)), K, int(factor_type)
        o.max_reproj_error, o.gate_max_pair_matches = float(max_reproj_error), int(gate_max_pair_matches)
        o.guided_grid = int(guided_grid)
        _check(lib().ptz_relocalizer_set_gate_model(self.handle, int(gate_model), int(gate_iters)), "ptz_relocalizer_set_gate_model")
        nf = krt_free_dim(factor_type)
        cam, acc = np.zeros((n, 15)), np.zeros(n, dtype=np.int32)
        summ, rep = (LmSummary * max(n, 1))(), (KrtTrimReport * max(n, 1))()
        sel = np.full((n, max(K, 1)), -1, dtype=np.int32)
        nsel, nmat, ninl = (np.zeros(n, dtype=np.int32) for _ in range(3))
        cov, s0, cst = np.zeros((n, nf, nf)), np.zeros(n), np.full(n, -1, dtype=np.int32)
        r = RelocResult()
        vp = lambda a: a.ctypes.data_as(C.c_void_p).value
        r.cam, r.accepted, r.sel_ref, r.n_sel, r.n_matches, r.n_inliers = vp(cam), vp(acc), vp(sel), vp(nsel), vp(nmat), vp(ninl)
        r.summaries, r.trim_report = C.addressof(summ), C.addressof(rep)
        r.cov, r.sigma0, r.cov_status = vp(cov), vp(s0), vp(cst)
        extra = {}
        if prior is not None:
            po = dict(prior)
            pc = np.ascontiguousarray(po.pop("cams"), dtype=np.float64).reshape(-1, 15)
            if len(pc) != n:
                raise ValueError("prior['cams']: one camera per query")
            po = prior_options(**po)
            pr = PriorResult()
            sl = np.full((n, max(int(po.max_refs), 1)), -1, dtype=np.int32)
            ns, ov = np.zeros(n, dtype=np.int32), np.zeros((n, len(self.ref_cams)), dtype=np.int32)
            pr.shortlist, pr.n_short, pr.overlap = vp(sl), vp(ns), vp(ov)
            _check(lib().ptz_relocalizer_run_tracked(self.handle, query_set.handle, n, _p(wh), _p(pc) if n else None, C.byref(o), C.byref(po),
                                                     C.byref(r), C.byref(pr)), "ptz_relocalizer_run_tracked")
            extra = dict(shortlist=sl, n_short=ns, overlap=ov, prior_ms=pr.prior_ms)
        elif landmarks is not None and landmark_prior is not None:
            po = dict(landmark_prior)
            pc = np.ascontiguousarray(po.pop("cams"), dtype=np.float64).reshape(-1, 15)
            if len(pc) != n:
                raise ValueError("landmark_prior['cams']: one camera per query")
            po = landmark_prior_options(**po)
            vr = LandmarkViewResult()
            nvis = np.zeros(n, dtype=np.int32)
            vr.n_visible = vp(nvis)
            _check(lib().ptz_relocalizer_run_landmarks_tracked(self.handle, landmarks.handle, query_set.handle, n, _p(wh), _p(pc) if n else None,
                                                               C.byref(o), C.byref(po), C.byref(r), C.byref(vr)),
                   "ptz_relocalizer_run_landmarks_tracked")
            extra = dict(n_visible=nvis, view_ms=vr.view_ms)
        elif landmarks is not None and landmark_shortlist is not None:
            so = shortlist_options(**landmark_shortlist)
            sr, vr = ShortlistResult(), LandmarkViewResult()
            sl = np.full((n, max(int(so.max_refs), 1)), -1, dtype=np.int32)
            ns, votes, nvis = np.zeros(n, dtype=np.int32), np.zeros((n, len(self.ref_cams)), dtype=np.int32), np.zeros(n, dtype=np.int32)
            sr.shortlist, sr.n_short, sr.votes, vr.n_visible = vp(sl), vp(ns), vp(votes), vp(nvis)
            _check(lib().ptz_relocalizer_run_landmarks_shortlisted(self.handle, landmarks.handle, query_set.handle, n, _p(wh), C.byref(o), C.byref(so),
                                                                   C.byref(r), C.byref(sr), C.byref(vr)), "ptz_relocalizer_run_landmarks_shortlisted")
            extra = dict(shortlist=sl, n_short=ns, votes=votes, votes_ms=sr.shortlist_ms, n_visible=nvis, view_ms=vr.view_ms)
        elif landmarks is not None:
            _check(lib().ptz_relocalizer_run_landmarks(self.handle, landmarks.handle, query_set.handle, n, _p(wh), C.byref(o), C.byref(r)),
                   "ptz_relocalizer_run_landmarks")
        elif shortlist is None:
            _check(lib().ptz_relocalizer_run(self.handle, query_set.handle, n, _p(wh), C.byref(o), C.byref(r)), "ptz_relocalizer_run")
        else:
            so = shortlist_options(**shortlist)
            sr = ShortlistResult()
            sl = np.full((n, max(int(so.max_refs), 1)), -1, dtype=np.int32)
            ns, votes = np.zeros(n, dtype=np.int32), np.zeros((n, len(self.ref_cams)), dtype=np.int32)
            sr.shortlist, sr.n_short, sr.votes = vp(sl), vp(ns), vp(votes)
            _check(lib().ptz_relocalizer_run_shortlisted(self.handle, query_set.handle, n, _p(wh), C.byref(o), C.byref(so), C.byref(r), C.byref(sr)),
                   "ptz_relocalizer_run_shortlisted")
            extra = dict(shortlist=sl, n_short=ns, votes=votes, shortlist_ms=sr.shortlist_ms)
        self._last_n = n
        return dict(extra, cam=cam, accepted=acc, summaries=[summ[i].as_dict() for i in range(n)], sel_ref=sel, n_sel=nsel, n_matches=nmat, n_inliers=ninl,
                    trim_report=[rep[i].as_dict() for i in range(n)] if trim is not None else None, cov=cov if uncertainty else None,
                    sigma0=s0 if uncertainty else None, cov_status=cst if uncertainty else None, stage_ms=np.array(list(r.stage_ms)))

    def pairs(self):
        """The last run's pair list: dict of pair_ref [n_pair] (reference image of each pair), query_ptr [n_query + 1]."""
        k = C.c_int32()
        _check(lib().ptz_relocalizer_pairs(self.handle, C.byref(k), None, None), "ptz_relocalizer_pairs")
        ref, ptr = np.zeros(k.value, dtype=np.int32), np.zeros(self._last_n + 1, dtype=np.int64)
        _check(lib().ptz_relocalizer_pairs(self.handle, None, _p(ref) if k.value else None, _p(ptr)), "ptz_relocalizer_pairs")
        return dict(pair_ref=ref, query_ptr=ptr)

    def table(self):
        """The last run's match table of its pairs (the relocalizer's own; downloaded): match_ptr, idx_a, idx_b, dist2, uv_a, uv_b."""
        L = lib()
        L.ptz_relocalizer_table.restype = C.c_void_p
        L.ptz_desc_matches_n_matches.restype = C.c_int64
        t = C.c_void_p(L.ptz_relocalizer_table(self.handle))
        if not t:
            raise ValueError("no run yet")
        n, npair = int(L.ptz_desc_matches_n_matches(t)), int(L.ptz_desc_matches_n_pairs(t))
        ptr = np.zeros(npair + 1, dtype=np.int64)
        ia, ib, d2 = (np.zeros(n, dtype=np.int32) for _ in range(3))
        ua, ub = (np.zeros((n, 2), dtype=np.float32) for _ in range(2))
        _check(L.ptz_desc_matches_download(t, _p(ptr), _p(ia), _p(ib), _p(d2), _p(ua) if n else None, _p(ub) if n else None), "ptz_desc_matches_download")
        return dict(match_ptr=ptr, idx_a=ia, idx_b=ib, dist2=d2, uv_a=ua, uv_b=ub)

    def view(self):
        """The view of the last run, if it had landmark_prior= or landmark_shortlist=: dict of vis_ptr [n + 1], vis_lm [n_vis], vis_uv [n_vis, 2]."""
        k = C.c_int64()
        _check(lib().ptz_relocalizer_view(self.handle, C.byref(k), None, None, None), "ptz_relocalizer_view")
        ptr, lm, uv = np.zeros(self._last_n + 1, dtype=np.int64), np.zeros(k.value, dtype=np.int32), np.zeros((k.value, 2), dtype=np.float32)
        _check(lib().ptz_relocalizer_view(self.handle, None, _p(ptr), _p(lm) if k.value else None, _p(uv) if k.value else None), "ptz_relocalizer_view")
        return dict(vis_ptr=ptr, vis_lm=lm, vis_uv=uv)

    def gate_models(self):
        """The models of the last run's gate on the assembled queries, if it ran with gate_model=1: dict of model [n, 10] (f, R row-major;
        zeros where found != 1) and found [n]."""
        n = self._last_n
        model, found = np.zeros((n, 10)), np.zeros(n, dtype=np.int32)
        _check(lib().ptz_relocalizer_gate_models(self.handle, _p(model), _p(found)), "ptz_relocalizer_gate_models")
        return dict(model=model, found=found)

    def matches(self):
        """The last run's assembled matches (tests): dict of match_ptr, uv_ref, uv_cur, src."""
        k = int(lib().ptz_relocalizer_n_matches(self.handle))
        n = self._last_n
        ptr = np.zeros(n + 1, dtype=np.int64)
        a, b, s = np.zeros((k, 2), dtype=np.float32), np.zeros((k, 2), dtype=np.float32), np.zeros(k, dtype=np.int32)
        _check(lib().ptz_relocalizer_matches(self.handle, _p(ptr), _p(a) if k else None, _p(b) if k else None, _p(s) if k else None),
               "ptz_relocalizer_matches")
        return dict(match_ptr=ptr, uv_ref=a, uv_cur=b, src=s)

    def close(self):
        if self.handle:
            lib().ptz_relocalizer_destroy(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
