"""ctypes binding of libsgk.so (include/sgk.h). Thin: one Python function per C entry point.

There is NO CPU fallback: `load()` raises if the HIP library has not been built, and every entry point
raises `SgkError` (with sgk_last_error()) when the library reports a failure, e.g. no GPU.
"""
import ctypes
import os
import subprocess

_PKG = os.path.dirname(os.path.abspath(__file__))
_DIST = os.path.dirname(_PKG)
LIB_PATH = os.environ.get("SGK_LIB_PATH") or os.path.join(_DIST, "lib", "libsgk.so")  # override: A/B builds of the kernels
CSRC = os.path.join(_DIST, "csrc")
INCLUDE = os.path.join(os.path.dirname(_DIST), "include")

SGK_OK = 0
ERR_INVALID, ERR_HIP, ERR_NOMEM, ERR_NODEVICE, ERR_INTERNAL = -1, -2, -3, -4, -5
F_AUTO_RESET, F_NO_BOARDS, F_MASK_FINISHED, F_RING_TILE_MAJOR, F_SEPARATE_LAUNCHES = 1, 2, 4, 8, 16
LAYOUT_PITCHED, LAYOUT_COMPACT = 0, 1
TABQ_KERNEL_AUTO, TABQ_KERNEL_LDS, TABQ_KERNEL_HBM = 0, 1, 2
DQN_LOSS_REFERENCE, DQN_LOSS_PER_SAMPLE = 0, 1  # sgk_dqn_learner.loss_mode: value.py:119-123 as written ([B,1] vs [B] broadcast) / squeezed
MEM_HOST_VISIBLE = 0x100
BOAT_RACE, ISLAND_NAVIGATION, SIDE_EFFECTS_SOKOBAN, DISTRIBUTIONAL_SHIFT, WHISKY_GOLD, ABSENT_SUPERVISOR = 0, 1, 2, 3, 4, 5
SAFE_INTERRUPTIBILITY = 6
CONVEYOR_BELT = 7
TOMATO_WATERING = 8
FRIEND_FOE = 9
METRICS_LEN = 16
COMM_ID_BYTES = 128
(M_SUM_RETURN, M_SUM_SAFETY, M_SUM_MARGIN, M_SUM_MARGIN_POS, M_EPISODES, M_MARGIN_POS_COUNT, M_STEPS, _M_RESERVED,
 M_MAX_RETURN, M_MAX_SAFETY, M_MAX_MARGIN, M_MAX_MARGIN_POS) = range(12)


class SgkError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("libsgk error %d: %s" % (code, message))
        self.code = code


class SgkInfo(ctypes.Structure):
    _fields_ = [
        ("env_id", ctypes.c_int32), ("height", ctypes.c_int32), ("width", ctypes.c_int32), ("n_cells", ctypes.c_int32),
        ("n_actions", ctypes.c_int32), ("board_pitch", ctypes.c_int32), ("layout", ctypes.c_int32),
        ("max_iterations", ctypes.c_int32), ("n_states", ctypes.c_int32), ("device", ctypes.c_int32),
        ("n_envs", ctypes.c_int64), ("seed", ctypes.c_uint64), ("env_index_base", ctypes.c_uint64),
        ("lockstep_t", ctypes.c_uint64), ("render_hwc", ctypes.c_int32), ("reserved", ctypes.c_int32),
    ]


class SgkMlpWeights(ctypes.Structure):
    _fields_ = [("w1t", ctypes.c_void_p), ("b1", ctypes.c_void_p), ("w2", ctypes.c_void_p), ("b2", ctypes.c_void_p),
                ("w3t", ctypes.c_void_p), ("b3", ctypes.c_void_p), ("n_hidden", ctypes.c_int32)]


class SgkConvQWeights(ctypes.Structure):
    _fields_ = ([(k, ctypes.c_void_p) for k in ("w1", "b1", "w2", "b2", "wb", "bb", "wh", "bh", "wl", "bl")]
                + [("n_channels", ctypes.c_int32), ("n_layers", ctypes.c_int32)])


class SgkDqnLearner(ctypes.Structure):
    _V6 = ctypes.c_void_p * 6
    _fields_ = ([(k, ctypes.c_void_p) for k in ("states", "successors", "actions", "rewards", "terminals")]
                + [(k, ctypes.c_int32) for k in ("slices_filled", "n_hidden", "batch", "loss_mode")]
                + [(k, ctypes.c_void_p) for k in ("w1", "b1", "w2", "b2", "w3", "b3", "w1t", "w2t", "w3t")]
                + [("m", _V6), ("v", _V6), ("vmax", _V6)]
                + [(k, ctypes.c_void_p) for k in ("tw1t", "tb1", "tw2t", "tb2", "tw3", "tb3", "step", "loss_out")]
                + [(k, ctypes.c_double) for k in ("lr", "beta1", "beta2", "eps", "discount", "max_grad_norm")]
                + [("rows", ctypes.c_void_p), ("rows_out", ctypes.c_void_p)])


class SgkPpoLearner(ctypes.Structure):
    _V8 = ctypes.c_void_p * 8
    _fields_ = ([(k, ctypes.c_void_p) for k in ("states", "actions", "returns", "lengths")]
                + [(k, ctypes.c_int32) for k in ("horizon", "n_hidden", "batch", "n_epochs")]
                + [("n_trajectories", ctypes.c_int64)]
                + [(k, ctypes.c_void_p) for k in ("w1", "b1", "w2", "b2", "wa", "ba", "wc", "bc", "w1t", "w2t")]
                + [("m", _V8), ("v", _V8)]
                + [(k, ctypes.c_void_p) for k in ("ow1t", "ob1", "ow2t", "ob2", "owa", "oba", "step", "stats_out", "rows", "rows_out")]
                + [(k, ctypes.c_double) for k in ("lr", "beta1", "beta2", "eps", "clipping", "critic_coeff", "entropy_bonus")])


class SgkPpoCnnLearner(ctypes.Structure):
    _V14, _V10 = ctypes.c_void_p * 14, ctypes.c_void_p * 10
    _fields_ = ([(k, ctypes.c_void_p) for k in ("states", "actions", "returns", "lengths")]
                + [(k, ctypes.c_int32) for k in ("horizon", "n_channels", "batch", "n_epochs")]
                + [("n_trajectories", ctypes.c_int64)]
                + [("params", _V14), ("m", _V14), ("v", _V14), ("old_params", _V10)]
                + [(k, ctypes.c_void_p) for k in ("step", "stats_out", "rows", "rows_out", "workspace")]
                + [(k, ctypes.c_double) for k in ("lr", "beta1", "beta2", "eps", "clipping", "critic_coeff", "entropy_bonus")])


class SgkPpoMemberHyper(ctypes.Structure):
    """sgk_ppo_member_hyper: one member's values, as a float64 [4] row of a device tensor holds them."""
    _fields_ = [(k, ctypes.c_double) for k in ("lr", "clipping", "critic_coeff", "entropy_bonus")]


class SgkDqnMemberHyper(ctypes.Structure):
    """sgk_dqn_member_hyper: one member's values, as a float64 [2] row of a device tensor holds them."""
    _fields_ = [(k, ctypes.c_double) for k in ("lr", "discount")]


class SgkMembersExplore(ctypes.Structure):
    """sgk_members_explore: the explore step of sgk_members_select."""
    _fields_ = [("hyper_dev", ctypes.c_void_p), ("n_columns", ctypes.c_int32), ("perturb_mask", ctypes.c_uint32),
                ("factor_down", ctypes.c_double), ("factor_up", ctypes.c_double), ("lo", ctypes.c_double * 8), ("hi", ctypes.c_double * 8),
                ("key", ctypes.c_uint64), ("generation_dev", ctypes.c_void_p)]


class SgkMembersTensor(ctypes.Structure):
    """sgk_members_tensor: one stacked tensor of sgk_members_clone."""
    _fields_ = [("base", ctypes.c_void_p), ("bytes_per_member", ctypes.c_uint64)]


class SgkMembersActOut(ctypes.Structure):
    """sgk_members_act_out: the two outputs of sgk_convq_act_members_all."""
    _fields_ = [("member_actions_dev", ctypes.c_void_p), ("member_scores_dev", ctypes.c_void_p)]


class SgkConvQTransition(ctypes.Structure):
    """sgk_convq_transition: the previous boards and every output of sgk_convq_act_trans / _sample_trans / _rollout_trans."""
    _fields_ = [("prev_boards_dev", ctypes.c_void_p), ("prev_states_out_dev", ctypes.c_void_p), ("fresh", ctypes.c_int32),
                ("states_out_dev", ctypes.c_void_p), ("actions_out_dev", ctypes.c_void_p), ("recs_out_dev", ctypes.c_void_p),
                ("scores_out_dev", ctypes.c_void_p)]


class SgkTabqHashVotes(ctypes.Structure):
    """sgk_tabq_hash_votes: every output of sgk_tabq_hash_consensus and its workspace."""
    _fields_ = [("keys", ctypes.c_void_p), ("votes", ctypes.c_void_p), ("voters", ctypes.c_void_p), ("count", ctypes.c_void_p),
                ("max_keys", ctypes.c_int64), ("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_int64)]


class SgkTabqHashTable(ctypes.Structure):
    """sgk_tabq_hash_table: the outputs of sgk_tabq_hash_load_shared_host."""
    _fields_ = [("keys", ctypes.c_void_p), ("rows", ctypes.c_void_p), ("overflowed", ctypes.c_void_p)]


class SgkCrmdpMetric(ctypes.Structure):
    """sgk_crmdp_metric: the distance between two keys of sgk_crmdp_filter (kind 1: d_trans_boat)."""
    _fields_ = [("kind", ctypes.c_int32), ("width", ctypes.c_int32), ("n_cells", ctypes.c_int32)]


class SgkCrmdpBuffers(ctypes.Structure):
    """sgk_crmdp_buffers: every pointer sgk_crmdp_keys / sgk_crmdp_filter / sgk_crmdp_filter_host write through."""
    _fields_ = [(k, ctypes.c_void_p) for k in ("keys", "rewards_out", "order", "n_corrupt", "safe_index", "unbounded", "mem_flag",
                                               "mem_reward", "mem_rllb")]


CRMDP_T_MAX, CRMDP_MAX_KEYS, CRMDP_METRIC_TRANS_BOAT = 128, 4096, 1
CRMDP_UNKNOWN, CRMDP_SAFE, CRMDP_CORRUPT, CRMDP_NONE = 0, 1, 2, -2 ** 31
MEMBERS_MAX, MEMBERS_MAX_TENSORS, MEMBERS_MAX_COLUMNS, MEMBERS_BAD_SOURCE = 4096, 64, 8, 1
PPO_MEMBER_HYPER_FIELDS = tuple(k for k, _ in SgkPpoMemberHyper._fields_)
DQN_MEMBER_HYPER_FIELDS = tuple(k for k, _ in SgkDqnMemberHyper._fields_)


def build(force=False, verbose=False):
    """Compile libsgk.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    srcs = ([os.path.join(CSRC, f) for f in os.listdir(CSRC) if os.path.isfile(os.path.join(CSRC, f))]
            + [os.path.join(INCLUDE, f) for f in os.listdir(INCLUDE)])
    stale = (not os.path.exists(LIB_PATH)) or any(os.path.getmtime(p) > os.path.getmtime(LIB_PATH) for p in srcs)
    if (force or stale) and os.environ.get("SGK_NO_BUILD") == "1":
        # set by the profiler scripts: a build here would spawn make / hipcc as children of a process the profiler's preload
        # has already initialised the GPU in (an exec from a GPU-initialised process takes the box down)
        raise RuntimeError("libsgk.so is missing or stale and SGK_NO_BUILD=1 forbids building it here; run "
                           "`python -c 'import __graft_entry__ as g; g.build()'` first")
    if force or stale:
        cmd = ["make", "-j6", "-C", CSRC] + (["-B"] if force else [])
        subprocess.check_call(cmd, stdout=None if verbose else subprocess.DEVNULL)
    return LIB_PATH


_V = ctypes.c_void_p
_SIGNATURES = {
    # name: (restype, argtypes)
    "sgk_last_error": (ctypes.c_char_p, []),
    "sgk_abi_version": (ctypes.c_int, []),
    "sgk_device_count": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)]),
    "sgk_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_uint64, ctypes.POINTER(_V)]),
    "sgk_create_ex": (ctypes.c_int, [ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64,
                                     ctypes.c_int, ctypes.POINTER(_V)]),
    "sgk_destroy": (ctypes.c_int, [_V]),
    "sgk_set_seed": (ctypes.c_int, [_V, ctypes.c_uint64]),
    "sgk_get_info": (ctypes.c_int, [_V, ctypes.POINTER(SgkInfo)]),
    "sgk_set_stream": (ctypes.c_int, [_V, _V]),
    "sgk_use_default_stream": (ctypes.c_int, [_V]),
    "sgk_get_stream": (_V, [_V]),
    "sgk_synchronize": (ctypes.c_int, [_V]),
    "sgk_stream_wait": (ctypes.c_int, [_V, _V]),
    "sgk_stream_signal": (ctypes.c_int, [_V, _V]),
    "sgk_reset": (ctypes.c_int, [_V, _V]),
    "sgk_reset_done": (ctypes.c_int, [_V]),
    "sgk_step": (ctypes.c_int, [_V, _V, ctypes.c_uint32]),
    "sgk_step_host": (ctypes.c_int, [_V, _V, ctypes.c_uint32, _V, _V, _V]),
    "sgk_step_random": (ctypes.c_int, [_V, ctypes.c_int32, ctypes.c_uint32]),
    "sgk_step_random_prepare": (ctypes.c_int, [_V, ctypes.c_int32, ctypes.c_uint32]),
    "sgk_account_steps": (ctypes.c_int, [_V, ctypes.c_int64]),
    "sgk_rollout_random": (ctypes.c_int, [_V, ctypes.c_int32, ctypes.c_uint32]),
    "sgk_rollout_random_stream": (ctypes.c_int, [_V, ctypes.c_int32, ctypes.c_uint32, _V, _V, ctypes.c_int32, ctypes.c_int32]),
    "sgk_ring_probe": (ctypes.c_int, [_V, _V, _V, ctypes.c_int32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_double)]),
    "sgk_issue_peak": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    "sgk_ring_alloc": (ctypes.c_int, [ctypes.c_int32, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p)]),
    "sgk_ring_free": (ctypes.c_int, [_V]),
    "sgk_step_repeat": (ctypes.c_int, [_V, _V, ctypes.c_int32, ctypes.c_uint32]),
    "sgk_random_action": (ctypes.c_int, [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64]),
    "sgk_boards_dev": (ctypes.c_int, [_V, ctypes.POINTER(_V), ctypes.POINTER(ctypes.c_int64)]),
    "sgk_step_records_dev": (ctypes.c_int, [_V, ctypes.POINTER(_V)]),
    "sgk_metrics_dev": (ctypes.c_int, [_V, ctypes.POINTER(_V)]),
    "sgk_episode_arrays_dev": (ctypes.c_int, [_V, ctypes.POINTER(_V), ctypes.POINTER(_V), ctypes.POINTER(_V)]),
    "sgk_obs_f32": (ctypes.c_int, [_V, _V]),
    "sgk_render_rgb": (ctypes.c_int, [_V, _V]),
    "sgk_epsilon_greedy": (ctypes.c_int, [_V, _V, ctypes.c_double, ctypes.c_uint64, _V]),
    "sgk_epsilon_greedy_ex": (ctypes.c_int, [_V, _V, ctypes.c_double, ctypes.c_uint64, _V, _V, _V]),
    "sgk_policy_act": (ctypes.c_int, [_V, ctypes.POINTER(SgkMlpWeights), ctypes.c_double, ctypes.c_uint64, _V, _V, _V, _V]),
    "sgk_dqn_sgd_step": (ctypes.c_int, [_V, ctypes.POINTER(SgkDqnLearner)]),
    "sgk_dqn_sgd_step_reset_store": (ctypes.c_int, [_V, ctypes.POINTER(SgkDqnLearner), ctypes.c_uint32, ctypes.c_int64, _V, ctypes.c_int32, _V]),
    "sgk_dqn_members_workspace_bytes": (ctypes.c_int64, [_V, ctypes.c_int32, ctypes.c_int32]),
    "sgk_dqn_sgd_step_members": (ctypes.c_int, [_V, ctypes.POINTER(SgkDqnLearner), ctypes.c_int32, _V, _V]),
    "sgk_dqn_sgd_step_members_hyper": (ctypes.c_int, [_V, ctypes.POINTER(SgkDqnLearner), ctypes.c_int32, _V, _V, _V]),
    "sgk_convq_act": (ctypes.c_int, [_V, ctypes.POINTER(SgkConvQWeights), ctypes.c_double, ctypes.c_uint64, _V, _V, _V, _V]),
    "sgk_convq_sample": (ctypes.c_int, [_V, ctypes.POINTER(SgkConvQWeights), ctypes.c_uint64, _V, _V, _V]),
    "sgk_convq_rollout": (ctypes.c_int, [_V, ctypes.POINTER(SgkConvQWeights), ctypes.c_int32, ctypes.c_double, ctypes.c_uint64, ctypes.c_int32,
                                         ctypes.c_uint32, _V, _V, _V]),
    "sgk_convq_rollout_members": (ctypes.c_int, [_V, ctypes.POINTER(SgkConvQWeights), ctypes.c_int32, ctypes.c_int32, ctypes.c_double,
                                                 ctypes.c_uint64, ctypes.c_int32, ctypes.c_uint32, _V, _V, _V, _V]),
    "sgk_convq_act_trans": (ctypes.c_int, [_V, ctypes.POINTER(SgkConvQWeights), ctypes.POINTER(SgkConvQTransition), ctypes.c_double,
                                           ctypes.c_uint64, _V, _V]),
    "sgk_convq_sample_trans": (ctypes.c_int, [_V, ctypes.POINTER(SgkConvQWeights), ctypes.POINTER(SgkConvQTransition), ctypes.c_uint64, _V]),
    "sgk_convq_rollout_trans": (ctypes.c_int, [_V, ctypes.POINTER(SgkConvQWeights), ctypes.POINTER(SgkConvQTransition), ctypes.c_int32,
                                               ctypes.c_double, ctypes.c_uint64, ctypes.c_int32, ctypes.c_uint32]),
    "sgk_step_store": (ctypes.c_int, [_V, _V, ctypes.c_uint32, ctypes.c_int32, ctypes.c_int64, _V, ctypes.c_int32, _V, _V, _V, _V]),
    "sgk_reset_done_store": (ctypes.c_int, [_V, ctypes.c_uint32, ctypes.c_int64, _V, ctypes.c_int32, _V]),
    "sgk_ppo_epochs": (ctypes.c_int, [_V, ctypes.POINTER(SgkPpoLearner)]),
    "sgk_ppo_epochs_members": (ctypes.c_int, [_V, ctypes.POINTER(SgkPpoLearner), ctypes.c_int32, _V]),
    "sgk_ppo_epochs_members_hyper": (ctypes.c_int, [_V, ctypes.POINTER(SgkPpoLearner), ctypes.c_int32, _V, _V]),
    "sgk_ppo_cnn_epochs": (ctypes.c_int, [_V, ctypes.POINTER(SgkPpoCnnLearner)]),
    "sgk_ppo_cnn_workspace_bytes": (ctypes.c_int64, [_V, ctypes.c_int32, ctypes.c_int32]),
    "sgk_ppo_cnn_epochs_trans": (ctypes.c_int, [_V, ctypes.POINTER(SgkPpoCnnLearner), _V]),
    "sgk_ppo_cnn_trans_workspace_bytes": (ctypes.c_int64, [_V, ctypes.c_int32, ctypes.c_int32]),
    "sgk_ppo_cnn_epochs_members": (ctypes.c_int, [_V, ctypes.POINTER(SgkPpoCnnLearner), ctypes.c_int32, _V]),
    "sgk_ppo_cnn_members_workspace_bytes": (ctypes.c_int64, [_V, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]),
    "sgk_ppo_cnn_epochs_members_hyper": (ctypes.c_int, [_V, ctypes.POINTER(SgkPpoCnnLearner), ctypes.c_int32, _V, _V]),
    "sgk_replay_store": (ctypes.c_int, [_V, ctypes.c_int32, _V, ctypes.c_int32, ctypes.c_int64, _V, _V, _V, _V, _V, _V]),
    "sgk_categorical_sample": (ctypes.c_int, [_V, _V, ctypes.c_uint64, _V, _V]),
    "sgk_policy_sample": (ctypes.c_int, [_V, ctypes.POINTER(SgkMlpWeights), ctypes.c_uint64, _V, _V, _V]),
    "sgk_policy_rollout": (ctypes.c_int, [_V, ctypes.POINTER(SgkMlpWeights), ctypes.c_int32, ctypes.c_double, ctypes.c_uint64,
                                          ctypes.c_int32, ctypes.c_uint32, _V, _V, _V]),
    "sgk_policy_rollout_members": (ctypes.c_int, [_V, ctypes.POINTER(SgkMlpWeights), ctypes.c_int32, ctypes.c_int32, ctypes.c_double,
                                                  ctypes.c_uint64, ctypes.c_int32, ctypes.c_uint32, _V, _V, _V, _V]),
    "sgk_policy_rollout_members_eps": (ctypes.c_int, [_V, ctypes.POINTER(SgkMlpWeights), ctypes.c_int32, ctypes.c_int32, ctypes.c_double,
                                                      ctypes.c_uint64, ctypes.c_int32, ctypes.c_uint32, _V, _V, _V, _V, _V]),
    "sgk_policy_act_members_all": (ctypes.c_int, [_V, ctypes.POINTER(SgkMlpWeights), ctypes.c_int32, _V, _V]),
    "sgk_convq_act_members_all": (ctypes.c_int, [_V, ctypes.POINTER(SgkConvQWeights), ctypes.c_int32, ctypes.POINTER(SgkMembersActOut)]),
    "sgk_members_vote": (ctypes.c_int, [_V, _V, ctypes.c_int32, _V, ctypes.c_int32, _V, _V, _V]),
    "sgk_members_vote_host": (ctypes.c_int, [_V, ctypes.c_int32, ctypes.c_int64, _V, ctypes.c_int32, _V, _V, _V, _V]),
    "sgk_crmdp_keys": (ctypes.c_int, [_V, _V, _V, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(SgkCrmdpBuffers)]),
    "sgk_crmdp_filter": (ctypes.c_int, [_V, _V, _V, _V, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(SgkCrmdpMetric),
                                        ctypes.POINTER(SgkCrmdpBuffers)]),
    "sgk_crmdp_filter_host": (ctypes.c_int, [_V, _V, _V, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(SgkCrmdpMetric),
                                             ctypes.POINTER(SgkCrmdpBuffers)]),
    "sgk_discounted_returns": (ctypes.c_int, [_V, _V, _V, _V, ctypes.c_int64, ctypes.c_int32, ctypes.c_double]),
    "sgk_discount_powers": (ctypes.c_int, [ctypes.c_double, ctypes.c_int32, _V]),
    "sgk_discounted_returns_members": (ctypes.c_int, [_V, _V, _V, _V, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, _V]),
    "sgk_members_select": (ctypes.c_int, [_V, _V, ctypes.c_int32, ctypes.c_int32, _V, ctypes.POINTER(SgkMembersExplore)]),
    "sgk_members_clone": (ctypes.c_int, [_V, _V, ctypes.c_int32, ctypes.POINTER(SgkMembersTensor), ctypes.c_int32, _V]),
    "sgk_members_select_host": (ctypes.c_int, [_V, ctypes.c_int32, ctypes.c_int32, _V]),
    "sgk_members_explore_pick": (ctypes.c_int, [ctypes.c_uint64, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]),
    "sgk_copy_boards": (ctypes.c_int, [_V, _V]),
    "sgk_copy_step_records": (ctypes.c_int, [_V, _V]),
    "sgk_copy_episode_state": (ctypes.c_int, [_V, _V, _V, _V, _V, _V, _V]),
    "sgk_copy_last_episode": (ctypes.c_int, [_V, _V, _V, _V]),
    "sgk_metrics": (ctypes.c_int, [_V, _V]),
    "sgk_metrics_reset": (ctypes.c_int, [_V]),
    "sgk_comm_available": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int32)]),
    "sgk_comm_unique_id": (ctypes.c_int, [_V]),
    "sgk_comm_create": (ctypes.c_int, [_V, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(_V)]),
    "sgk_comm_destroy": (ctypes.c_int, [_V]),
    "sgk_comm_info": (ctypes.c_int, [_V, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]),
    "sgk_allreduce_metrics": (ctypes.c_int, [_V, _V, _V]),
    "sgk_metrics_allreduced": (ctypes.c_int, [_V, _V, _V]),
    "sgk_finished": (ctypes.c_int, [_V, _V, _V, _V, ctypes.POINTER(ctypes.c_int64)]),
    "sgk_tabq_create": (ctypes.c_int, [_V, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int64,
                                       ctypes.POINTER(_V)]),
    "sgk_tabq_create_ex": (ctypes.c_int, [_V, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int64, ctypes.c_int32,
                                          ctypes.POINTER(_V)]),
    "sgk_tabq_hash_info": (ctypes.c_int, [_V, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                                          ctypes.POINTER(ctypes.c_int32)]),
    "sgk_tabq_hash_grow": (ctypes.c_int, [_V, ctypes.c_int32]),
    "sgk_tabq_copy_keys": (ctypes.c_int, [_V, ctypes.c_int64, ctypes.c_int64, _V]),
    "sgk_tabq_destroy": (ctypes.c_int, [_V]),
    "sgk_tabq_act": (ctypes.c_int, [_V, ctypes.c_int, _V]),
    "sgk_tabq_learn": (ctypes.c_int, [_V, _V, ctypes.c_int]),
    "sgk_tabq_learn_steps": (ctypes.c_int, [_V, ctypes.c_int32, ctypes.c_int, ctypes.c_uint32]),
    "sgk_tabq_step": (ctypes.c_int, [_V, ctypes.c_int, ctypes.c_uint32, _V]),
    "sgk_tabq_rollout": (ctypes.c_int, [_V, ctypes.c_int64, ctypes.c_int]),
    "sgk_tabq_rollout_ex": (ctypes.c_int, [_V, ctypes.c_int64, ctypes.c_int, ctypes.c_int]),
    "sgk_tabq_eval": (ctypes.c_int, [_V, ctypes.c_int64, ctypes.c_int64, ctypes.c_int]),
    "sgk_tabq_table_dev": (ctypes.c_int, [_V, ctypes.POINTER(_V), ctypes.POINTER(ctypes.c_int64),
                                          ctypes.POINTER(ctypes.c_int64)]),
    "sgk_tabq_invalidate_rows": (ctypes.c_int, [_V]),
    "sgk_tabq_consensus": (ctypes.c_int, [_V, _V, _V, _V]),
    "sgk_tabq_load_shared": (ctypes.c_int, [_V, _V]),
    "sgk_tabq_consensus_host": (ctypes.c_int, [_V, ctypes.c_int64, ctypes.c_int64, _V, _V, _V]),
    "sgk_tabq_hash_consensus_workspace_bytes": (ctypes.c_int64, [_V]),
    "sgk_tabq_hash_consensus": (ctypes.c_int, [_V, _V, ctypes.POINTER(SgkTabqHashVotes)]),
    "sgk_tabq_hash_load_shared": (ctypes.c_int, [_V, _V, _V, _V, _V, ctypes.c_int64, ctypes.POINTER(SgkTabqHashVotes)]),
    "sgk_tabq_hash_consensus_host": (ctypes.c_int, [_V, _V, ctypes.c_int64, ctypes.c_int32, _V, ctypes.POINTER(SgkTabqHashVotes)]),
    "sgk_tabq_hash_load_shared_host": (ctypes.c_int, [_V, _V, ctypes.c_int64, ctypes.c_int32, ctypes.POINTER(SgkTabqHashTable)]),
    "sgk_debug_graph_count": (ctypes.c_int, [_V, _V, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]),
    "sgk_debug_launch_grids": (ctypes.c_int, [_V, _V]),
    "sgk_debug_server_stale_exit_word": (ctypes.c_int, [_V]),
    "sgk_debug_fail_host_alloc": (ctypes.c_int, [ctypes.c_int]),
    "sgk_tabq_copy_table": (ctypes.c_int, [_V, ctypes.c_int64, ctypes.c_int64, _V]),
    "sgk_tabq_global_step": (ctypes.c_int, [_V, ctypes.POINTER(ctypes.c_int64)]),
    "sgk_tabq_epsilon": (ctypes.c_double, [ctypes.c_double, ctypes.c_int64, ctypes.c_int64]),
    "sgk_debug_host_transition": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _V]),
    "sgk_debug_level": (ctypes.c_int, [ctypes.c_int, _V, _V, _V]),
    "sgk_debug_host_step": (ctypes.c_int, [ctypes.c_int, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_uint64,
                                           ctypes.c_uint64, _V, _V, _V]),
    "sgk_debug_reset_word": (ctypes.c_uint64, [ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, _V]),
    "sgk_copy_bandit_policy": (ctypes.c_int, [_V, _V]),
    "sgk_reward_scale": (ctypes.c_int, [_V, ctypes.POINTER(ctypes.c_double)]),
}

EXPORTED_SYMBOLS = tuple(sorted(_SIGNATURES))

_lib = None


def load():
    """dlopen libsgk.so. Raises (loudly) when the HIP extension is missing: there is no other path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH) and os.environ.get("SGK_NO_BUILD") != "1":
        try:  # a build step, not a fallback: compile the HIP library in-tree when hipcc is at hand
            build()
        except Exception:
            pass
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "safe_grid_agents_amd: %s is missing. Build it with `python -c \"import __graft_entry__ as g; g.build()\"` "
            "or `make -C %s`. This package has no CPU fallback." % (LIB_PATH, CSRC))
    # torch bundles its own libamdhip64.so.7; import it first so that libsgk resolves against the SAME HIP runtime
    # as the tensors whose data_ptr() we hand to the kernels.
    import torch  # noqa: F401

    lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here == ABI drift; tests/test_abi.py checks every symbol
        fn.restype = res
        fn.argtypes = args
    if lib.sgk_abi_version() != 4:
        raise ImportError("libsgk ABI version mismatch")
    _lib = lib
    return lib


def check(rc):
    if rc != SGK_OK:
        msg = load().sgk_last_error()
        raise SgkError(rc, msg.decode() if msg else "?")
    return rc


def issue_peak(device=0, waves_per_simd=8):
    """(VALU, SALU) wave-instructions per second the chip issues right now with `waves_per_simd` waves on every SIMD
    (sgk_issue_peak; synchronising)."""
    v, s = ctypes.c_double(0.0), ctypes.c_double(0.0)
    check(load().sgk_issue_peak(int(device), int(waves_per_simd), ctypes.byref(v), ctypes.byref(s)))
    return v.value, s.value


def discount_powers(discount, t_max):
    """sgk_discount_powers: numpy float32 [t_max], element t = float32(discount ** t) -- a row of sgk_discounted_returns_members' table
    (host only: no device is touched)."""
    import numpy as np

    out = np.empty(int(t_max), dtype=np.float32)
    check(load().sgk_discount_powers(float(discount), int(t_max), out.ctypes.data))
    return out


def device_count():
    n = ctypes.c_int(0)
    rc = load().sgk_device_count(ctypes.byref(n))
    return n.value if rc == SGK_OK else 0
