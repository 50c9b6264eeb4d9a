"""ctypes binding of libekfslam.so -- exactly the symbols include/ekfslam.h declares.

There is no CPU or PyTorch fallback: if the shared library is missing this raises, and on a machine
without a HIP device ``ekf_create`` returns EKF_ERR_NO_DEVICE (surfaced as ``EkfError``).
"""
import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("EKF_LIB_PATH") or os.path.join(_HERE, "libekfslam.so")   # override: A/B builds

EKF_OK = 0
EKF_ERR_INVALID_ARG, EKF_ERR_NO_DEVICE, EKF_ERR_HIP, EKF_ERR_CAPACITY = 1, 2, 3, 4
EKF_ERR_INDEX, EKF_ERR_LOOKUP, EKF_ERR_STATE, EKF_ERR_COMM = 5, 6, 7, 8
EKF_MODE_KNOWN, EKF_MODE_UC = 0, 1
EKF_COMM_ID_BYTES = 128
EKF_MERGE_BATCH_MAX = 32
EKF_FRAME_MAP, EKF_FRAME_ROBOT = 0, 1                  # ekf_extract_map, ekf_transform_map: the map's own frame / the robot's
EKF_STORE_F64, EKF_STORE_F32 = 0, 1
EKF_ARITH_F64, EKF_ARITH_F32, EKF_ARITH_SPLIT3 = 0, 1, 2
(EKF_KERNEL_DOWNDATE, EKF_KERNEL_GATHER, EKF_KERNEL_PREDICT, EKF_KERNEL_ASSOCIATE, EKF_KERNEL_APPEND,
 EKF_KERNEL_ROWPANEL, EKF_KERNEL_EXCHANGE, EKF_KERNEL_COMPACT, EKF_KERNEL_COUNT) = range(9)

_d = ctypes.c_double
_dp = ctypes.POINTER(ctypes.c_double)
_i32 = ctypes.c_int32
_i64 = ctypes.c_int64
_vp = ctypes.c_void_p


class EkfConfig(ctypes.Structure):
    """struct ekf_config (include/ekfslam.h)."""
    _fields_ = [("C", _d), ("Rc", _d * 2), ("s_cost", _d), ("s_thresh", _d), ("w_pos", _d),
                ("capacity_landmarks", _i64), ("mode", _i32), ("storage", _i32), ("device", _i32),
                ("tile", _i32), ("rank", _i32), ("world", _i32), ("batch", _i32), ("async_flush", _i32), ("device_assoc", _i32),
                ("pass_direction", _i32), ("force_sharded", _i32), ("pass_arith", _i32), ("reserved", _i32 * 2)]


class EkfLinearObs(ctypes.Structure):
    """struct ekf_linear_obs (include/ekfslam.h)."""
    _fields_ = [("z", _d * 2), ("R", _d * 4), ("Hr", _d * 6), ("lm", _i64 * 2), ("Hl", (_d * 4) * 2), ("gate", _d),
                ("wrap_deg", _i32 * 2), ("rows", _i32)]


class EkfLinearResult(ctypes.Structure):
    """struct ekf_linear_result (include/ekfslam.h)."""
    _fields_ = [("nu", _d * 2), ("S", _d * 4), ("d2", _d), ("outcome", _i32)]


EKF_LINEAR_IRREGULAR, EKF_LINEAR_APPLIED, EKF_LINEAR_GATED = 0, 1, 2
EKF_LINEAR_UNASSIGNED = 3                             # a step of ekf_observe_model_assigned whose observation was left out


class EkfModelObs(ctypes.Structure):
    """struct ekf_model_obs (include/ekfslam.h)."""
    _fields_ = [("model", _i32), ("reserved", _i32), ("z", _d * 2), ("R", _d * 4), ("lm", _i64 * 2), ("anchor", _d * 2), ("gate", _d)]


EKF_MODEL_RANGE_BEARING, EKF_MODEL_RANGE, EKF_MODEL_BEARING, EKF_MODEL_RELATIVE_XY, EKF_MODEL_LANDMARK_RANGE = 1, 2, 3, 4, 5
EKF_MODEL_ROWS = {1: 2, 2: 1, 3: 1, 4: 2, 5: 1}       # rows of z each model reads

EKF_MODEL_ITER_MAX = 16


class EkfIteratedResult(ctypes.Structure):
    """struct ekf_iterated_result (include/ekfslam.h)."""
    _fields_ = [("S", _d * 4), ("nu", _d * 2), ("used", _i32), ("converged", _i32), ("last_step", _d), ("x_local", _d * 7)]


EKF_APPEND_MODEL_MAX = 32


class EkfModelInit(ctypes.Structure):
    """struct ekf_model_init (include/ekfslam.h)."""
    _fields_ = [("model", _i32), ("reserved", _i32), ("z", _d * 2), ("R", _d * 4), ("signature", _d)]


EKF_ASSOCIATE_MODEL_MAX = 32


class EkfModelMatch(ctypes.Structure):
    """struct ekf_model_match (include/ekfslam.h)."""
    _fields_ = [("best", _i64), ("second", _i64), ("d2_best", _d), ("d2_second", _d), ("within_gate", _i64), ("irregular", _i64)]


EKF_ASSIGN_MODEL_MAX = 32
EKF_ASSIGN_CANDIDATES = 32


class EkfModelAssigned(ctypes.Structure):
    """struct ekf_model_assigned (include/ekfslam.h)."""
    _fields_ = [("landmark", _i64), ("d2", _d), ("ncand", _i64), ("reserved", _i64)]


EKF_JOINT_MAX = 32
EKF_JOINT_HYP_MAX = 256


class EkfJointResult(ctypes.Structure):
    """struct ekf_joint_result (include/ekfslam.h)."""
    _fields_ = [("d2", _d), ("dof", _i32), ("pairings", _i32), ("outcome", _i32), ("first_irregular", _i32)]


EKF_JOINT_SEARCH_CAND = 4
EKF_JOINT_SEARCH_BEAM_MAX = 64


class EkfJointSearchResult(ctypes.Structure):
    """struct ekf_joint_search_result (include/ekfslam.h)."""
    _fields_ = [("lm", _i64 * EKF_JOINT_MAX), ("d2", _d), ("dof", _i32), ("pairings", _i32), ("truncated", _i32), ("nalive", _i32),
                ("irregular", _i32), ("tested", _i32 * EKF_JOINT_MAX), ("survived", _i32 * EKF_JOINT_MAX)]


EKF_JOINT_ITER_MAX = EKF_MODEL_ITER_MAX
EKF_JOINT_SUB_MAX = 3 + 2 * EKF_JOINT_MAX


class EkfJointIterResult(ctypes.Structure):
    """struct ekf_joint_iter_result (include/ekfslam.h)."""
    _fields_ = [("used", _i32), ("converged", _i32), ("last_step", _d), ("d2_last", _d), ("irregular_at", _i32), ("irregular_obs", _i32),
                ("ns", _i32), ("reserved", _i32), ("x_sub", _d * EKF_JOINT_SUB_MAX)]


EKF_MOTION_TURN_DRIVE, EKF_MOTION_ARC, EKF_MOTION_POSE_DELTA = 1, 2, 3
EKF_MOTION_INPUTS = {1: 2, 2: 2, 3: 3}                # entries of u (and rows of M) each motion model reads
EKF_PREDICT_MODEL_MAX = 32


class EkfMotion(ctypes.Structure):
    """struct ekf_motion (include/ekfslam.h)."""
    _fields_ = [("model", _i32), ("reserved", _i32), ("u", _d * 3), ("M", _d * 9)]


EKF_DENSE_MAX = 16                                    # rows of one ekf_observe_dense call: one chunk of ekf_multiply_map


class EkfObserveDenseResult(ctypes.Structure):
    """struct ekf_observe_dense_result (include/ekfslam.h)."""
    _fields_ = [("d2", _d), ("rows", _i32), ("outcome", _i32), ("bad_row", _i32)]


EKF_FACTOR_REF_MAX = 8                                # reference states of one ekf_factor_map call


class EkfFactorInfo(ctypes.Structure):
    """struct ekf_factor_info (include/ekfslam.h)."""
    _fields_ = [("n", _i64), ("definite", _i32), ("bad_index", _i64), ("bad_pivot", _d), ("logdet", _d), ("logdet_map", _d),
                ("min_pivot", _d), ("max_pivot", _d)]


# name -> (restype, argtypes); every symbol of include/ekfslam.h
SIGNATURES = {
    "ekf_abi_version": (_i32, []),
    "ekf_status_string": (ctypes.c_char_p, [_i32]),
    "ekf_config_default": (_i32, [ctypes.POINTER(EkfConfig), _i32]),
    "ekf_create": (_i32, [ctypes.POINTER(EkfConfig), ctypes.POINTER(_vp)]),
    "ekf_destroy": (_i32, [_vp]),
    "ekf_last_error": (ctypes.c_char_p, [_vp]),
    "ekf_set_stream": (_i32, [_vp, _vp]),
    "ekf_sync": (_i32, [_vp]),
    "ekf_flush": (_i32, [_vp]),
    "ekf_pending": (_i32, [_vp, ctypes.POINTER(_i32)]),
    "ekf_set_params": (_i32, [_vp, _d, _dp, _d, _d, _d]),
    "ekf_predict": (_i32, [_vp, _dp]),
    "ekf_motion_model": (_i32, [_dp, _i64, _dp, _dp, _dp]),
    "ekf_append": (_i32, [_vp, _dp, _dp, _dp, _d]),
    "ekf_correct": (_i32, [_vp, _dp, _dp, _i64]),
    "ekf_associate": (_i32, [_vp, _dp, _dp, ctypes.POINTER(_i32), ctypes.POINTER(_i64), _dp, _dp]),
    "ekf_associate_begin": (_i32, [_vp, _dp, _dp, _i32]),
    "ekf_associate_finish": (_i32, [_vp, ctypes.POINTER(_i32), ctypes.POINTER(_i64), _dp, _dp]),
    "ekf_measure": (_i32, [_vp, _dp, _i64, _dp, _dp, _dp, _i64]),
    "ekf_comm_unique_id": (_i32, [ctypes.c_char_p]),
    "ekf_comm_init": (_i32, [_vp, ctypes.c_char_p]),
    "ekf_hint_next": (_i32, [_vp, _i64]),
    "ekf_correct_begin": (_i32, [_vp, _dp, _dp, _i64]),
    "ekf_correct_finish": (_i32, [_vp]),
    "ekf_prefetch_rows": (_i32, [_vp, ctypes.POINTER(_i64), _i32]),
    "ekf_prefetch_next": (_i32, [_vp, ctypes.POINTER(_i64), _i32]),
    "ekf_prefetch_begin": (_i32, [_vp, ctypes.POINTER(_i64), _i32]),
    "ekf_prefetch_finish": (_i32, [_vp]),
    "ekf_exchange_info": (_i32, [_vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_i64),
                                 ctypes.POINTER(_i64)]),
    "ekf_exchange_set_buffers": (_i32, [_vp, _vp, _vp]),
    "ekf_exchange_local": (_i32, [ctypes.POINTER(_vp), _i32]),
    "ekf_exchange_set_hook": (_i32, [_vp, _vp, _vp]),
    "ekf_shard_owner": (_i32, [_i32, _i64, _i64]),
    "ekf_shard_slot": (_i64, [_i32, _i64, _i64]),
    "ekf_shard_panel_source": (_i32, [_i32, _i64, _i64, ctypes.POINTER(_i32), ctypes.POINTER(_i64)]),
    "ekf_num_landmarks": (_i32, [_vp, ctypes.POINTER(_i64)]),
    "ekf_get_x": (_i32, [_vp, _dp]),
    "ekf_set_x": (_i32, [_vp, _dp, _i64]),
    "ekf_get_s": (_i32, [_vp, _dp]),
    "ekf_set_s": (_i32, [_vp, _dp, _i64]),
    "ekf_remove_landmarks": (_i32, [_vp, ctypes.POINTER(_i64), _i64]),
    "ekf_constrain_landmarks": (_i32, [_vp, _i64, _i64, _dp, _dp]),
    "ekf_merge_landmarks": (_i32, [_vp, _i64, _i64, _dp]),
    "ekf_merge_landmarks_batch": (_i32, [_vp, ctypes.POINTER(_i64), ctypes.POINTER(_i64), _i64, _dp, _dp]),
    "ekf_landmark_distance": (_i32, [_vp, _i64, _i64, _dp, _dp, _dp, _dp]),
    "ekf_nearest_landmarks": (_i32, [_vp, _dp, _dp, ctypes.POINTER(_i64)]),
    "ekf_observe_linear": (_i32, [_vp, ctypes.POINTER(EkfLinearObs), ctypes.POINTER(EkfLinearResult)]),
    "ekf_linear_innovation": (_i32, [_vp, ctypes.POINTER(EkfLinearObs), ctypes.POINTER(EkfLinearResult)]),
    "ekf_linear_rejections": (_i32, [_vp, ctypes.POINTER(_i64), ctypes.POINTER(_i64)]),
    "ekf_observe_model": (_i32, [_vp, ctypes.POINTER(EkfModelObs), ctypes.POINTER(EkfLinearResult)]),
    "ekf_model_innovation": (_i32, [_vp, ctypes.POINTER(EkfModelObs), ctypes.POINTER(EkfLinearResult)]),
    "ekf_model_evaluate": (_i32, [_i32, _dp, _dp, _dp, _dp, _dp]),
    "ekf_observe_model_iterated": (_i32, [_vp, ctypes.POINTER(EkfModelObs), _i32, _d, ctypes.POINTER(EkfLinearResult),
                                          ctypes.POINTER(EkfIteratedResult)]),
    "ekf_model_innovation_iterated": (_i32, [_vp, ctypes.POINTER(EkfModelObs), _i32, _d, ctypes.POINTER(EkfLinearResult),
                                             ctypes.POINTER(EkfIteratedResult)]),
    "ekf_model_iterate": (_i32, [_i32, _dp, _dp, _i32, _dp, _dp, _d, _i32, _d, ctypes.POINTER(EkfLinearResult),
                                 ctypes.POINTER(EkfIteratedResult)]),
    "ekf_append_model": (_i32, [_vp, ctypes.POINTER(EkfModelInit), _i64, ctypes.POINTER(_i64)]),
    "ekf_model_invert": (_i32, [_i32, _dp, _dp, _dp, _dp, _dp]),
    "ekf_join_map": (_i32, [_vp, _vp, _d, ctypes.POINTER(_i64)]),
    "ekf_extract_map": (_i32, [_vp, ctypes.POINTER(_i64), _i64, _i32, _vp]),
    "ekf_transform_map": (_i32, [_vp, _i32, _dp, _dp]),
    "ekf_factor_map": (_i32, [_vp, _dp, _i32, ctypes.POINTER(EkfFactorInfo), _dp]),
    "ekf_sample_map": (_i32, [_vp, _dp, _i64, _dp, ctypes.POINTER(EkfFactorInfo)]),
    "ekf_solve_map": (_i32, [_vp, _i32, _dp, _i64, _dp, ctypes.POINTER(EkfFactorInfo)]),
    "ekf_multiply_map": (_i32, [_vp, _dp, _i64, _dp]),
    "ekf_observe_dense": (_i32, [_vp, _dp, _i64, _dp, _dp, ctypes.POINTER(_i32), _d, ctypes.POINTER(EkfObserveDenseResult), _dp, _dp]),
    "ekf_observe_dense_innovation": (_i32, [_vp, _dp, _i64, _dp, _dp, ctypes.POINTER(_i32), ctypes.POINTER(EkfObserveDenseResult), _dp, _dp]),
    "ekf_associate_model": (_i32, [_vp, ctypes.POINTER(EkfModelObs), _i64, ctypes.POINTER(EkfModelMatch), _dp]),
    "ekf_assign_model": (_i32, [_vp, ctypes.POINTER(EkfModelObs), _i64, ctypes.POINTER(EkfModelAssigned), ctypes.POINTER(EkfModelMatch),
                                ctypes.POINTER(_i64), _dp, _dp]),
    "ekf_observe_model_assigned": (_i32, [_vp, ctypes.POINTER(EkfModelObs), _i64]),
    "ekf_assigned_scan_result": (_i32, [_vp, ctypes.POINTER(_i64), ctypes.POINTER(EkfModelAssigned), ctypes.POINTER(EkfLinearResult), _dp]),
    "ekf_joint_innovation": (_i32, [_vp, ctypes.POINTER(EkfModelObs), _i64, ctypes.POINTER(_i64), _i64, ctypes.POINTER(EkfJointResult), _dp, _dp,
                                    _dp]),
    "ekf_joint_search": (_i32, [_vp, ctypes.POINTER(EkfModelObs), _i64, _dp, _i32, ctypes.POINTER(EkfJointSearchResult),
                                ctypes.POINTER(EkfModelMatch), ctypes.POINTER(_i64), _dp, ctypes.POINTER(_i64), _dp]),
    "ekf_observe_model_joint": (_i32, [_vp, ctypes.POINTER(EkfModelObs), _i64, ctypes.POINTER(_i64), _d, ctypes.POINTER(EkfJointResult), _dp, _dp]),
    "ekf_observe_model_joint_iterated": (_i32, [_vp, ctypes.POINTER(EkfModelObs), _i64, ctypes.POINTER(_i64), _d, _i32, _d,
                                                ctypes.POINTER(EkfJointResult), ctypes.POINTER(EkfJointIterResult), _dp, _dp]),
    "ekf_joint_iterate": (_i32, [_dp, _dp, ctypes.POINTER(EkfModelObs), _i64, _i32, _d, ctypes.POINTER(EkfJointIterResult), _dp, _dp]),
    "ekf_predict_model": (_i32, [_vp, ctypes.POINTER(EkfMotion), _i64]),
    "ekf_motion_evaluate": (_i32, [_i32, _dp, _dp, _dp, _dp, _dp]),
    "ekf_diag_poke_device_signature": (_i32, [_vp, _i64, _d]),
    "ekf_get_P": (_i32, [_vp, _dp]),
    "ekf_set_P": (_i32, [_vp, _dp, _i64]),
    "ekf_get_P_block": (_i32, [_vp, _i64, _i64, _i64, _i64, _dp]),
    "ekf_get_P_diag_blocks": (_i32, [_vp, _dp]),
    "ekf_get_Q": (_i32, [_vp, _dp]),
    "ekf_load_lowrank_state": (_i32, [_vp, _i64, _dp, _dp, _dp, _dp, _i64]),
    "ekf_checkpoint_save": (_i32, [_vp, ctypes.c_char_p]),
    "ekf_checkpoint_load": (_i32, [_vp, ctypes.c_char_p]),
    "ekf_P_digest": (_i32, [_vp, _dp]),
    "ekf_device_bytes": (_i32, [_vp, ctypes.POINTER(_i64)]),
    "ekf_kernel_timing_enable": (_i32, [_vp, _i32, _i32]),
    "ekf_kernel_timing_read": (_i32, [_vp, _i32, ctypes.POINTER(_i64), _dp]),
    "ekf_downdate_kernel_name": (ctypes.c_char_p, [_vp, ctypes.POINTER(_i32)]),
    "ekf_downdate_algorithmic_bytes": (_i32, [_vp, ctypes.POINTER(_i64)]),
}

_LIB = None


class EkfError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("libekfslam status %d: %s" % (status, message))
        self.status = status


def build():
    """Compile libekfslam.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(_HERE, "csrc")])


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libekfslam.so is not built (%s); run __graft_entry__.build() or "
                              "`make -C ekf_slam_amd/csrc` -- there is no fallback path" % LIB_PATH)
        # One HIP runtime per process: the PyTorch-ROCm wheel bundles its own libamdhip64 / librccl (sonames
        # libamdhip64.so.7 / librccl.so.1).  If torch is going to be used in this process (streams,
        # torch.distributed) it must be loaded FIRST so that libekfslam's NEEDED libamdhip64.so.7 and its
        # dlopen("librccl.so.1") bind to the copies torch already mapped; loading /opt/rocm's copy first and
        # torch's second leaves two runtimes fighting over the device ("No HIP GPUs are available").
        if os.environ.get("EKF_NO_TORCH", "0") != "1":
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)       # AttributeError if the library lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _LIB = L
    return _LIB

EXCHANGE_HOOK = ctypes.CFUNCTYPE(ctypes.c_int32, ctypes.c_void_p)      # int32_t (*)(void *ctx): ekf_exchange_set_hook
