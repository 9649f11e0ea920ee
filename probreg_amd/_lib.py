"""ctypes binding of ``csrc/libprobreg_hip.so`` (the C ABI of include/probreg_hip.h).

The shared library is the product: there is no Python / NumPy fallback for anything it
computes.  If it is missing or fails to load, importing this module raises ``ImportError``
with the build command, and every wrapper raises on a non-zero status.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# PROBREG_HIP_LIB: an alternative build of the same library (instrumented / experimental), for tools only
LIB_PATH = os.environ.get("PROBREG_HIP_LIB") or os.path.join(_HERE, "csrc", "libprobreg_hip.so")

PRG_OK = 0
PRG_ERR_INVALID = -1
PRG_ERR_HIP = -2
PRG_ERR_STATE = -3
PRG_ERR_NOMEM = -4

PRG_TF_RIGID = 0
PRG_TF_AFFINE = 1
PRG_TF_NONRIGID = 2

PRG_NMOMENTS = 32
PRG_NPARAMS = 32
PRG_COMM_ID_BYTES = 128


class ProbregHipError(RuntimeError):
    """A libprobreg_hip call failed (HIP runtime error or call-order violation)."""


def _load():
    # PyTorch ships its own copy of the HIP runtime (torch/lib/libamdhip64.so) and the dynamic loader keeps whichever copy
    # of that soname is loaded FIRST.  If ours came first (the system's /opt/rocm runtime), torch.cuda would later find
    # "no GPUs" in the same process - and with it RCCL; loading torch first makes both sides share torch's runtime,
    # whatever the import order of the caller.  torch stays optional.
    try:
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch absent, or present with broken shared libraries (OSError): stay usable
        pass
    if not os.path.isfile(LIB_PATH):
        raise ImportError(
            "probreg_amd: %s not found. Build it with `python __graft_entry__.py build` "
            "(or `make -C probreg_amd/csrc`); there is no CPU fallback." % LIB_PATH
        )
    try:
        return ctypes.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover - depends on the ROCm install
        raise ImportError("probreg_amd: cannot load %s: %s" % (LIB_PATH, e))


lib = _load()

_c = ctypes
_vp, _i, _i64, _d = _c.c_void_p, _c.c_int, _c.c_int64, _c.c_double
_pp = _c.POINTER(_c.c_void_p)

# name -> argtypes; every function returns int except prg_last_error.  This table is the Python
# mirror of include/probreg_hip.h and tests/test_abi.py checks the two against each other.
SIGNATURES = {
    "prg_version": [],
    "prg_device_count": [_c.POINTER(_i)],
    "prg_cpd_create": [_pp, _i, _vp],
    "prg_cpd_destroy": [_vp],
    "prg_spatial_order": [_vp, _i64, _i, _i, _vp],
    "prg_cpd_set_options": [_vp, _i, _i, _i],
    "prg_cpd_set_dense_engine": [_vp, _i, _d],
    "prg_cpd_last_estep_engine": [_vp, _c.POINTER(_i)],
    "prg_cpd_set_sparse_engine": [_vp, _i],
    "prg_cpd_engine_bounds": [_i64, _i64, _c.POINTER(_d), _c.POINTER(_d)],
    "prg_cpd_last_estep_lean": [_vp, _c.POINTER(_i)],
    "prg_cpd_set_lean_factor": [_vp, _d],
    "prg_cpd_set_stream_mode": [_vp, _i],
    "prg_cpd_last_estep_engines": [_vp, _c.POINTER(_i), _c.POINTER(_i)],
    "prg_cpd_set_source": [_vp, _vp, _i64, _i],
    "prg_cpd_set_target": [_vp, _vp, _i64, _i, _i64],
    "prg_cpd_bind_moments": [_vp, _vp],
    "prg_cpd_moments_ptr": [_vp, _pp],
    "prg_cpd_params_ptr": [_vp, _pp],
    "prg_comm_available": [_c.POINTER(_i)],
    "prg_comm_unique_id": [_vp],
    "prg_comm_create": [_pp, _vp, _i, _i, _i],
    "prg_comm_adopt": [_pp, _vp, _i],
    "prg_comm_info": [_vp, _c.POINTER(_i), _c.POINTER(_i), _c.POINTER(_i64)],
    "prg_comm_destroy": [_vp],
    "prg_comm_all_reduce_f64": [_vp, _vp, _i64, _vp],
    "prg_cpd_set_comm": [_vp, _vp],
    "prg_cpd_iterate": [_vp, _i, _i, _d, _i],
    "prg_cpd_set_moments_only": [_vp, _i],
    "prg_cpd_batch_tile_shape": [_c.POINTER(_i), _c.POINTER(_i)],
    "prg_topk_sweep": [_i, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i, _d, _i, _i, _vp, _vp],
    "prg_cpd_correspond": [_vp, _i, _i, _vp, _vp, _vp],
    "prg_cpd_correspond_tile_shape": [_c.POINTER(_i), _c.POINTER(_i)],
    "prg_cpd_batch_tile_table": [_i, _vp, _vp, _vp, _i64, _c.POINTER(_i64)],
    "prg_cpd_batch_create": [_pp, _i, _vp, _i, _i, _vp, _vp, _vp, _vp],
    "prg_cpd_batch_destroy": [_vp],
    "prg_cpd_batch_init": [_vp, _vp],
    "prg_cpd_batch_iterate": [_vp, _i, _i, _vp, _vp, _i],
    "prg_cpd_batch_active": [_vp, _c.POINTER(_i)],
    "prg_cpd_batch_get_params": [_vp, _vp, _vp],
    "prg_cpd_last_estep_fused": [_vp, _c.POINTER(_i)],
    "prg_cpd_set_fused_factor": [_vp, _d],
    "prg_cpd_set_resid_sweep": [_vp, _i],
    "prg_cpd_init_sums": [_vp],
    "prg_cpd_init_params": [_vp, _vp],
    "prg_cpd_estep": [_vp, _d],
    "prg_cpd_estep_timed": [_vp, _d, _vp],
    "prg_cpd_pair_counts": [_vp, _c.POINTER(_d), _c.POINTER(_d)],
    "prg_cpd_mstep": [_vp, _i, _i],
    "prg_cpd_get_params": [_vp, _vp],
    "prg_cpd_set_params": [_vp, _vp],
    "prg_cpd_get_moments": [_vp, _vp],
    "prg_cpd_get_estep": [_vp, _vp, _vp, _vp],
    "prg_cpd_get_tsource": [_vp, _vp],
    "prg_cpd_moments_from_estep": [_vp, _vp, _vp, _vp],
    "prg_cpd_set_tuning": [_vp, _i, _i, _i, _i],
    "prg_cpd_nonrigid_build_g": [_vp, _d],
    "prg_cpd_nonrigid_set_solver": [_vp, _i, _i, _d],
    "prg_cpd_nonrigid_rank": [_vp, _c.POINTER(_i)],
    "prg_cpd_nonrigid_get_g": [_vp, _vp],
    "prg_cpd_nonrigid_set_w": [_vp, _vp],
    "prg_cpd_nonrigid_get_w": [_vp, _vp],
    "prg_cpd_nonrigid_apply": [_vp, _vp],
    "prg_cpd_nonrigid_set_priors": [_vp, _vp, _vp, _d],
    "prg_cpd_rowacc_ptr": [_vp, _pp, _c.POINTER(_i64)],
    "prg_cpd_mstep_nonrigid": [_vp, _d],
    "prg_cpd_set_source_weights": [_vp, _vp, _d],
    "prg_cpd_bcpd_build_g": [_vp, _d],
    "prg_cpd_bcpd_set_solver": [_vp, _i, _i, _d],
    "prg_cpd_bcpd_solve": [_vp, _d, _d, _vp, _vp, _vp, _vp],
    "prg_gauss_transform_direct": [_i, _vp, _vp, _i64, _vp, _i64, _i, _vp, _i, _d, _vp],
    "prg_gauss_transform_direct_f64": [_i, _vp, _vp, _i64, _vp, _i64, _i, _vp, _i, _d, _vp],
    "prg_squared_kernel_sum": [_i, _vp, _vp, _i64, _vp, _i64, _i, _c.POINTER(_d)],
    "prg_rbf_kernel": [_i, _vp, _vp, _i64, _vp, _i64, _i, _d, _vp],
    "prg_inverse_multiquadric_kernel": [_i, _vp, _vp, _i64, _vp, _i64, _i, _d, _vp],
    "prg_nn_mean_distance": [_i, _vp, _vp, _i64, _vp, _i64, _i, _c.POINTER(_d)],
    "prg_lattice_set_splat_mode": [_i],
    "prg_ph_create": [_pp, _i, _vp],
    "prg_ph_destroy": [_vp],
    "prg_ph_init": [_vp, _vp, _i64, _i, _i],
    "prg_ph_lattice_size": [_vp, _c.POINTER(_i)],
    "prg_ph_filter": [_vp, _vp, _i, _vp],
    "prg_fr_create": [_pp, _i, _vp],
    "prg_fr_destroy": [_vp],
    "prg_fr_set_source": [_vp, _vp, _i64, _i],
    "prg_fr_set_target": [_vp, _vp, _i64, _i],
    "prg_fr_set_state": [_vp, _vp, _vp, _d],
    "prg_fr_estep": [_vp, _d, _c.POINTER(_i), _c.POINTER(_i)],
    "prg_fr_get_estep": [_vp, _vp, _vp, _vp],
    "prg_fr_mstep": [_vp, _d, _i, _d, _vp],
    "prg_fr_get_state": [_vp, _vp],
    "prg_fr_last_route": [_vp, _c.POINTER(_i)],
    "prg_fr_set_target_normals": [_vp, _vp],
    "prg_fr_get_nx": [_vp, _vp],
    "prg_fr_mstep_pt2pl": [_vp, _d, _i, _d, _vp],
    "prg_fr_mstep_from_arrays": [_i, _vp, _vp, _i64, _i, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _d, _d, _vp],
    "prg_dq_skin": [_i, _vp, _vp, _i64, _vp, _vp, _vp, _i, _vp],
    "prg_fr_set_skinning": [_vp, _vp, _vp, _i64, _i, _c.POINTER(_i)],
    "prg_fr_set_dualquats": [_vp, _vp, _i],
    "prg_fr_get_dualquats": [_vp, _vp, _i],
    "prg_fr_kinematic_estep": [_vp, _d, _d, _c.POINTER(_i), _c.POINTER(_i)],
    "prg_fr_kinematic_set_arrays": [_vp, _vp, _vp, _vp, _vp, _i64],
    "prg_fr_kinematic_normal_sums": [_vp, _d, _d, _i, _i, _vp],
    "prg_fr_kinematic_grad_sums": [_vp, _vp, _i, _i, _vp],
    "prg_fr_kinematic_sums_from_arrays": [_i, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i, _d, _d, _i, _vp, _i,
                                          _vp, _vp],
    "prg_kabsch_weighted": [_i, _vp, _vp, _vp, _vp, _i64, _i, _vp, _vp],
    "prg_gmm_create": [_pp, _i, _vp],
    "prg_gmm_destroy": [_vp],
    "prg_gmm_build": [_vp, _vp, _i64, _i, _vp, _d, _d, _i, _vp, _vp, _vp],
    "prg_gmm_set_nodes": [_vp, _vp, _i],
    "prg_gmm_get_nodes": [_vp, _vp],
    "prg_gmm_set_target": [_vp, _vp, _i64],
    "prg_gmm_reg_estep": [_vp, _vp, _vp, _d, _d, _vp, _vp],
    "prg_gmmfit_create": [_pp, _i, _vp],
    "prg_gmmfit_destroy": [_vp],
    "prg_gmmfit_set_data": [_vp, _vp, _i64, _i],
    "prg_gmmfit_seed": [_vp, _i, _vp, _i],
    "prg_gmmfit_get_seeds": [_vp, _vp],
    "prg_gmmfit_lloyd": [_vp, _i, _d, _c.POINTER(_i)],
    "prg_gmmfit_init_from_labels": [_vp, _d],
    "prg_gmmfit_set_params": [_vp, _i, _vp, _vp, _vp],
    "prg_gmmfit_em": [_vp, _d, _i, _d, _c.POINTER(_i), _c.POINTER(_i), _vp],
    "prg_gmmfit_get_params": [_vp, _vp, _vp, _vp],
    "prg_ocsvm_create": [_pp, _i, _vp],
    "prg_ocsvm_destroy": [_vp],
    "prg_ocsvm_working_set_size": [_c.POINTER(_i)],
    "prg_ocsvm_set_data": [_vp, _vp, _i64, _i],
    "prg_ocsvm_solve": [_vp, _d, _d, _d, _i, _i, _c.POINTER(_i), _c.POINTER(_i), _c.POINTER(_i), _c.POINTER(_d)],
    "prg_ocsvm_get_solution": [_vp, _vp, _c.POINTER(_d), _c.POINTER(_d), _c.POINTER(_i)],
    "prg_ocsvm_get_support": [_vp, _vp],
    "prg_ocsvm_decision": [_vp, _vp, _i64, _vp],
    "prg_ocsvm_set_profile": [_vp, _i],
    "prg_ocsvm_get_profile": [_vp, _vp],
    "prg_fpfh_create": [_pp, _i, _vp],
    "prg_fpfh_destroy": [_vp],
    "prg_fpfh_max_nn": [_c.POINTER(_i)],
    "prg_fpfh_set_data": [_vp, _vp, _i64],
    "prg_fpfh_search": [_vp, _i, _d, _i],
    "prg_fpfh_get_neighbours": [_vp, _i, _vp, _vp, _vp],
    "prg_fpfh_normals": [_vp],
    "prg_fpfh_set_normals": [_vp, _vp],
    "prg_fpfh_get_normals": [_vp, _vp],
    "prg_fpfh_spfh": [_vp],
    "prg_fpfh_get_spfh": [_vp, _vp],
    "prg_fpfh_fpfh": [_vp],
    "prg_fpfh_get_fpfh": [_vp, _vp],
    "prg_feature_match": [_i, _vp, _vp, _i64, _vp, _i64, _i, _i, _vp, _vp],
    "prg_feature_match_mutual": [_i, _vp, _vp, _i64, _vp, _i64, _i, _i, _vp, _vp, _vp],
    "prg_ransac_create": [_pp, _i, _vp],
    "prg_ransac_destroy": [_vp],
    "prg_ransac_set_correspondences": [_vp, _vp, _vp, _i64],
    "prg_ransac_build": [_vp, _c.c_uint64, _c.c_uint64, _i64, _d],
    "prg_ransac_get_hypotheses": [_vp, _vp, _vp, _vp],
    "prg_ransac_set_hypotheses": [_vp, _vp, _vp, _i64],
    "prg_ransac_score": [_vp, _d],
    "prg_ransac_get_scores": [_vp, _vp, _vp],
    "prg_ransac_best": [_vp, _c.POINTER(_i64), _c.POINTER(_i), _c.POINTER(_d), _vp],
    "prg_ransac_refine": [_vp, _d, _i, _vp, _c.POINTER(_i), _c.POINTER(_d), _vp],
    "prg_voxel_create": [_pp, _i, _vp],
    "prg_voxel_destroy": [_vp],
    "prg_voxel_set_data": [_vp, _vp, _i64, _i],
    "prg_voxel_set_channels": [_vp, _vp, _i],
    "prg_voxel_run": [_vp, _d],
    "prg_voxel_count": [_vp, _c.POINTER(_i64)],
    "prg_voxel_get_means": [_vp, _vp],
    "prg_voxel_get_channel_means": [_vp, _vp],
    "prg_voxel_get_counts": [_vp, _vp],
    "prg_voxel_get_first": [_vp, _vp],
    "prg_voxel_get_inverse": [_vp, _vp],
    "prg_voxel_get_keys": [_vp, _vp],
    "prg_voxel_get_order": [_vp, _vp],
    "prg_voxel_get_rows": [_vp, _vp],
    "prg_icp_create": [_pp, _i, _vp],
    "prg_icp_destroy": [_vp],
    "prg_icp_set_target": [_vp, _vp, _vp, _i64, _d],
    "prg_icp_get_grid": [_vp, _c.POINTER(_d), _vp, _c.POINTER(_i), _c.POINTER(_i)],
    "prg_icp_set_source": [_vp, _vp, _i64],
    "prg_icp_set_pose": [_vp, _vp],
    "prg_icp_get_pose": [_vp, _vp],
    "prg_icp_search": [_vp, _d],
    "prg_icp_get_matches": [_vp, _vp, _vp],
    "prg_icp_sums": [_vp, _i, _vp],
    "prg_icp_step": [_vp, _i],
    "prg_icp_iterate": [_vp, _i, _d, _i, _d, _d, _i],
    "prg_icp_get_state": [_vp, _vp, _c.POINTER(_i64), _c.POINTER(_d), _c.POINTER(_i), _c.POINTER(_i), _c.POINTER(_i)],
    "prg_icp_set_covariances": [_vp, _i, _vp, _i64],
    "prg_icp_set_covariances_from_normals": [_vp, _i, _vp, _i64, _d],
    "prg_icp_get_covariances": [_vp, _i, _vp],
    "prg_icp_max_k": [_c.POINTER(_i)],
    "prg_icp_knn": [_vp, _i, _d],
    "prg_icp_get_knn": [_vp, _vp, _vp, _vp],
    "prg_icp_radius_count": [_vp, _d],
    "prg_icp_get_counts": [_vp, _vp],
    "prg_icp_outlier_statistical": [_vp, _i, _d],
    "prg_icp_outlier_radius": [_vp, _d, _i],
    "prg_icp_get_outlier": [_vp, _vp, _vp, _vp],
    "prg_icp_dbscan": [_vp, _d, _i],
    "prg_icp_get_dbscan": [_vp, _vp, _vp, _vp, _vp],
    "prg_field_create": [_pp, _i, _vp],
    "prg_field_destroy": [_vp],
    "prg_field_set_control": [_vp, _vp, _vp, _i64, _i, _i, _i, _d],
    "prg_field_evaluate": [_vp, _vp, _i64, _vp],
    "prg_plane_create": [_pp, _i, _vp],
    "prg_plane_destroy": [_vp],
    "prg_plane_set_points": [_vp, _vp, _vp, _i64],
    "prg_plane_count": [_vp, _c.POINTER(_i64)],
    "prg_plane_build": [_vp, _c.c_uint64, _c.c_uint64, _i64],
    "prg_plane_get_hypotheses": [_vp, _vp, _vp, _vp],
    "prg_plane_set_hypotheses": [_vp, _vp, _vp, _i64],
    "prg_plane_score": [_vp, _d, _d],
    "prg_plane_get_scores": [_vp, _vp, _vp],
    "prg_plane_best": [_vp, _c.POINTER(_i64), _c.POINTER(_i64), _c.POINTER(_i), _c.POINTER(_d), _vp],
    "prg_plane_refine": [_vp, _d, _d, _i, _vp, _vp],
    "prg_plane_classify": [_vp, _vp, _d, _d, _vp, _vp, _c.POINTER(_i), _c.POINTER(_d)],
    "prg_plane_remove": [_vp, _c.POINTER(_i64)],
    "prg_fgr_create": [_pp, _i, _vp],
    "prg_fgr_destroy": [_vp],
    "prg_fgr_set_clouds": [_vp, _vp, _i64, _vp, _i64],
    "prg_fgr_set_correspondences": [_vp, _vp, _i64],
    "prg_fgr_normalise": [_vp, _i, _vp, _vp, _c.POINTER(_d)],
    "prg_fgr_set_chunk": [_vp, _i64],
    "prg_fgr_tuples": [_vp, _c.c_uint64, _d, _i64, _c.POINTER(_i64), _c.POINTER(_i64)],
    "prg_fgr_set_used": [_vp, _vp, _i64],
    "prg_fgr_get_used": [_vp, _vp],
    "prg_fgr_set_state": [_vp, _vp, _d],
    "prg_fgr_sums": [_vp, _vp],
    "prg_fgr_step": [_vp, _i, _d, _d],
    "prg_fgr_iterate": [_vp, _i, _i, _d, _d],
    "prg_fgr_get_state": [_vp, _i, _vp, _c.POINTER(_d), _c.POINTER(_i64), _c.POINTER(_i), _c.POINTER(_d)],
    "prg_fgr_get_weights": [_vp, _vp],
}

for _name, _args in SIGNATURES.items():
    _fn = getattr(lib, _name)  # AttributeError here = the library does not export a declared symbol
    _fn.argtypes = _args
    _fn.restype = _i
lib.prg_last_error.argtypes = []
lib.prg_last_error.restype = _c.c_char_p


def last_error():
    msg = lib.prg_last_error()
    return msg.decode("utf-8", "replace") if msg else ""


def check(status):
    """Map a prg_status to the exception the reference raises in the same situation."""
    if status == PRG_OK:
        return
    msg = last_error()
    if status == PRG_ERR_INVALID:
        raise ValueError(msg)
    if status == PRG_ERR_NOMEM:
        raise MemoryError(msg)
    raise ProbregHipError("libprobreg_hip status %d: %s" % (status, msg))


def device_count():
    n = _i(0)
    st = lib.prg_device_count(_c.byref(n))
    if st != PRG_OK:
        return 0
    return int(n.value)


def require_gpu():
    n = device_count()
    if n <= 0:
        raise ProbregHipError(
            "probreg_amd needs an AMD GPU (gfx950): hipGetDeviceCount reported none (%s). "
            "There is no CPU fallback." % last_error()
        )
    return n


def ptr(a):
    """Raw pointer of a C-contiguous numpy array or of a torch tensor (host or device)."""
    if a is None:
        return None
    if hasattr(a, "data_ptr"):
        return _vp(a.data_ptr())
    return _vp(a.ctypes.data)


def _current_device_and_stream(device=None):
    """(device index, hipStream_t as int) of the calling process; torch is optional plumbing."""
    try:
        import torch

        if torch.cuda.is_available():
            dev = torch.cuda.current_device() if device is None else int(device)
            return dev, int(torch.cuda.current_stream(dev).cuda_stream)
    except ImportError:  # pragma: no cover
        pass
    return (0 if device is None else int(device)), 0


class Handle(object):
    """Life cycle of one opaque handle of the library: ``create(&h, device, stream, *create_args)`` on the
    calling process's device and stream unless told otherwise, ``close()`` any number of times, and a ``__del__`` that is
    safe while the interpreter shuts down.  The plan classes derive from it and add what their handle computes."""

    def __init__(self, create, destroy, device=None, stream=None, *create_args):
        count = require_gpu()
        if device is not None and not 0 <= int(device) < count:  # (before torch is asked for that device's stream)
            raise ValueError("device %d out of range (%d devices)" % (int(device), count))
        self.device, self.stream = _current_device_and_stream(device)
        if stream is not None:
            self.stream = int(stream)
        self._destroy = destroy
        self._h = ctypes.c_void_p()
        check(create(ctypes.byref(self._h), self.device, ctypes.c_void_p(self.stream), *create_args))

    def close(self):
        if getattr(self, "_h", None):
            self._destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # pragma: no cover - interpreter shutdown
            pass


def as_points(x):
    """ndarray or Open3D PointCloud (duck-typed ``.points``) -> float64 ndarray, unchecked (the reference's cpd.py:444);
    None stays None."""
    if x is None:
        return None
    if hasattr(x, "points") and not isinstance(x, np.ndarray):
        x = x.points
    return np.asarray(x, dtype=np.float64)


def as_cloud(data, name, dims, min_points=1):
    """C-contiguous float64 (n, d) of an array or of anything with ``.points``, d in ``dims``; ValueError, naming the
    argument, for another shape, fewer than ``min_points`` rows, or a value that is not finite."""
    pts = np.ascontiguousarray(as_points(data))
    if pts.ndim != 2 or pts.shape[1] not in dims:
        raise ValueError("%s must be %s, got shape %s" % (name, " or ".join("(n, %d)" % d for d in dims), pts.shape))
    if pts.shape[0] < min_points:
        raise ValueError("%s must hold at least %s" % (name, "one point" if min_points == 1 else "%d points" % min_points))
    if not np.all(np.isfinite(pts)):
        raise ValueError("%s contains NaN or infinity" % name)
    return pts
