"""ctypes binding of libmgx.so (the C ABI declared in include/mgx.h).

This is the reference-side binding a Python caller uses; no torch types cross
the ABI (device pointers are plain integers).  torch MUST be imported before
the library is loaded so that libmgx binds to the HIP runtime torch already
loaded (both carry SONAME libamdhip64.so.7) -- one runtime per process.
"""
import ctypes
import os

import torch  # before the library is loaded (see module docstring: load order matters)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MGX_LIB_PATH", os.path.join(HERE, "libmgx.so"))   # override: diagnostic builds

MGX_OK = 0
GAE_SCRATCH_WORDS = 512  # == MGX_GAE_SCRATCH_WORDS (include/mgx.h)
ABI_VERSION = 9        # == MGX_ABI_VERSION (include/mgx.h)
PROBLEMS = {"multi": 0, "full": 1, "gto": 2, "gtg": 3, "opn": 4, "pkp": 5, "drp": 6, "mov": 7}
TERMINAL = {"none": 0, "truncated": 1, "all": 2}
DEVERR = {1: "MT19937 ring: a cursor left the window of the stream the device holds", 2: "action outside 0..6 (ValueError: Unknown action)",
          4: "PCG64 rejection loop bound exceeded", 8: "object list exhausted (AssertionError / IndexError in the reference)",
          16: "episode ring ran dry (engine invariant broken)"}

# Every entry point include/mgx.h declares (checked by tests/test_abi.py).
EXPORTS = ("mgx_last_error", "mgx_abi_version", "mgx_create", "mgx_destroy", "mgx_reset", "mgx_step",
           "mgx_join", "mgx_get_config", "mgx_set_seed", "mgx_gae", "mgx_gae_dones", "mgx_poll_error", "mgx_stats", "mgx_debug_counters", "mgx_dump_state", "mgx_mission_text",
           "mgx_step_compact", "mgx_rollout_compact", "mgx_rollout_compact_gae", "mgx_observe_compact", "mgx_gather",
           "mgx_gather_ring", "mgx_scene", "mgx_set_clock", "mgx_clock_words", "mgx_clock_groups",
           "mgx_ring_levels", "mgx_random_actions", "mgx_set_random_policy", "mgx_policy_blob_words",
           "mgx_policy_act", "mgx_policy_bootstrap", "mgx_policy_grad_scratch_words", "mgx_policy_backward",
           "mgx_mission_workspace_words", "mgx_mission_forward", "mgx_mission_backward",
           "mgx_ppo_loss_scratch_words", "mgx_ppo_loss", "mgx_adam_scratch_words", "mgx_adam_step",
           "mgx_mission_forward_rows", "mgx_mission_backward_rows", "mgx_adam_schedule", "mgx_adam_step_sched",
           "mgx_eval_record", "mgx_policy_moe_scratch_words", "mgx_policy_act_moe", "mgx_expert_act")
CLOCK_CLASSES = 4   # == MGX_CLOCK_CLASSES (include/mgx.h)
MOE_MAX_EXPERTS = 8     # == MGX_MOE_MAX_EXPERTS (include/mgx.h)
MOE_RECORD_WORDS = 32   # == MGX_MOE_RECORD_WORDS (include/mgx.h)


class MgxConfig(ctypes.Structure):
    _fields_ = [
        ("problem", ctypes.c_int32), ("mission", ctypes.c_int32), ("size", ctypes.c_int32),
        ("num_objects", ctypes.c_int32), ("see_through_walls", ctypes.c_int32),
        ("all_doors_open", ctypes.c_int32), ("obstacles", ctypes.c_int32), ("n_stack", ctypes.c_int32),
        ("n_envs", ctypes.c_int64), ("base_seed", ctypes.c_int64), ("env_index_offset", ctypes.c_int64),
        ("livelock_words", ctypes.c_int32), ("terminal_mode", ctypes.c_int32),
        ("mission_int64", ctypes.c_int32), ("refill_cap", ctypes.c_int32), ("mt_table_words", ctypes.c_int64),
        ("ring_depth", ctypes.c_int32), ("refill_every", ctypes.c_int32),
        ("percent_obstacles", ctypes.c_double), ("manual", ctypes.c_int32), ("reserved0", ctypes.c_int32),
    ]


class MgxObs(ctypes.Structure):
    _fields_ = [("image_dev", ctypes.c_void_p), ("direction_dev", ctypes.c_void_p),
                ("mission_dev", ctypes.c_void_p)]


class MgxStepOut(ctypes.Structure):
    _fields_ = [
        ("obs", MgxObs), ("terminal", MgxObs),
        ("reward_dev", ctypes.c_void_p), ("reward64_dev", ctypes.c_void_p),
        ("terminated_dev", ctypes.c_void_p), ("truncated_dev", ctypes.c_void_p), ("done_dev", ctypes.c_void_p),
        ("ep_return_dev", ctypes.c_void_p), ("ep_len_dev", ctypes.c_void_p), ("livelock_dev", ctypes.c_void_p),
    ]


class MgxCompactOut(ctypes.Structure):
    _fields_ = [
        ("row_dev", ctypes.c_void_p), ("mission_id_dev", ctypes.c_void_p), ("terminal_row_dev", ctypes.c_void_p),
        ("reward_dev", ctypes.c_void_p), ("reward64_dev", ctypes.c_void_p),
        ("terminated_dev", ctypes.c_void_p), ("truncated_dev", ctypes.c_void_p), ("done_dev", ctypes.c_void_p),
        ("ep_return_dev", ctypes.c_void_p), ("ep_len_dev", ctypes.c_void_p), ("livelock_dev", ctypes.c_void_p),
    ]


class MgxRolloutOut(ctypes.Structure):
    _fields_ = [
        ("rows_dev", ctypes.c_void_p), ("mission_ids_dev", ctypes.c_void_p), ("terminal_row_dev", ctypes.c_void_p),
        ("rewards_dev", ctypes.c_void_p), ("rewards64_dev", ctypes.c_void_p), ("terminated_dev", ctypes.c_void_p),
        ("truncated_dev", ctypes.c_void_p), ("dones_dev", ctypes.c_void_p), ("ep_return_dev", ctypes.c_void_p),
        ("ep_len_dev", ctypes.c_void_p), ("livelock_dev", ctypes.c_void_p),
    ]


class MgxGaeArgs(ctypes.Structure):
    _fields_ = [
        ("values_dev", ctypes.c_void_p), ("last_values_dev", ctypes.c_void_p), ("gamma", ctypes.c_float),
        ("gamma_lambda", ctypes.c_float), ("advantages_dev", ctypes.c_void_p), ("returns_dev", ctypes.c_void_p),
        ("adv_stats_dev", ctypes.c_void_p), ("stats_scratch_dev", ctypes.c_void_p),
    ]


class MgxPolicy(ctypes.Structure):
    _fields_ = [
        ("blob_dev", ctypes.c_void_p), ("mission_feat_dev", ctypes.c_void_p), ("mode", ctypes.c_int32),
        ("reserved0", ctypes.c_int32), ("seed", ctypes.c_uint64), ("counter_dev", ctypes.c_void_p),
    ]


class MgxActOut(ctypes.Structure):
    _fields_ = [
        ("actions_dev", ctypes.c_void_p), ("values_dev", ctypes.c_void_p), ("log_probs_dev", ctypes.c_void_p),
        ("logits_dev", ctypes.c_void_p),
    ]


class MgxPolicyMoe(ctypes.Structure):
    _fields_ = [
        ("n_experts", ctypes.c_int32), ("mode", ctypes.c_int32),
        ("blob_dev", ctypes.c_void_p * MOE_MAX_EXPERTS), ("mission_feat_dev", ctypes.c_void_p * MOE_MAX_EXPERTS),
        ("route_dev", ctypes.c_void_p), ("seed", ctypes.c_uint64), ("counter_dev", ctypes.c_void_p),
        ("scratch_dev", ctypes.c_void_p), ("scratch_words", ctypes.c_int64),
    ]


class MgxBootstrap(ctypes.Structure):
    _fields_ = [
        ("truncated_dev", ctypes.c_void_p), ("terminated_dev", ctypes.c_void_p), ("rewards_dev", ctypes.c_void_p),
        ("gamma", ctypes.c_float), ("reserved0", ctypes.c_int32), ("list_dev", ctypes.c_void_p),
        ("count_dev", ctypes.c_void_p), ("values_dev", ctypes.c_void_p),
    ]


class MgxPolicyGrad(ctypes.Structure):
    _fields_ = [
        ("blob_dev", ctypes.c_void_p), ("mission_feat_dev", ctypes.c_void_p), ("g_logits_dev", ctypes.c_void_p),
        ("g_values_dev", ctypes.c_void_p), ("grad_blob_dev", ctypes.c_void_p),
        ("grad_mission_feat_dev", ctypes.c_void_p), ("scratch_dev", ctypes.c_void_p),
        ("scratch_words", ctypes.c_int64), ("max_groups", ctypes.c_int32), ("reserved0", ctypes.c_int32),
    ]


class MgxMissionParams(ctypes.Structure):
    _fields_ = [("embedding_dev", ctypes.c_void_p), ("w_ih_dev", ctypes.c_void_p), ("w_hh_dev", ctypes.c_void_p),
                ("b_ih_dev", ctypes.c_void_p), ("b_hh_dev", ctypes.c_void_p)]


class MgxMissionGrads(ctypes.Structure):
    _fields_ = MgxMissionParams._fields_


class MgxPpoLossArgs(ctypes.Structure):
    _fields_ = [
        ("logits_dev", ctypes.c_void_p), ("values_dev", ctypes.c_void_p), ("sel_dev", ctypes.c_void_p),
        ("actions_dev", ctypes.c_void_p), ("old_values_dev", ctypes.c_void_p), ("old_log_probs_dev", ctypes.c_void_p),
        ("advantages_dev", ctypes.c_void_p), ("returns_dev", ctypes.c_void_p), ("adv_stats_dev", ctypes.c_void_p),
        ("g_logits_dev", ctypes.c_void_p), ("g_values_dev", ctypes.c_void_p), ("stats_dev", ctypes.c_void_p),
        ("scratch_dev", ctypes.c_void_p), ("scratch_words", ctypes.c_int64),
        ("clip_range", ctypes.c_double), ("clip_range_vf", ctypes.c_double), ("ent_coef", ctypes.c_double),
        ("vf_coef", ctypes.c_double), ("adv_mode", ctypes.c_int32), ("reserved0", ctypes.c_int32),
    ]


class MgxAdamArgs(ctypes.Structure):
    _fields_ = [
        ("lr", ctypes.c_double), ("beta1", ctypes.c_double), ("beta2", ctypes.c_double), ("eps", ctypes.c_double),
        ("step", ctypes.c_int64), ("max_grad_norm", ctypes.c_double), ("grad_scale", ctypes.c_double),
    ]


class MgxAdamSched(ctypes.Structure):
    _fields_ = [("step_size", ctypes.c_float), ("bc2_sqrt", ctypes.c_float)]


class MgxEvalRecordArgs(ctypes.Structure):
    _fields_ = [
        ("done_dev", ctypes.c_void_p), ("reward64_dev", ctypes.c_void_p), ("ep_return_dev", ctypes.c_void_p),
        ("ep_len_dev", ctypes.c_void_p), ("mission_id_dev", ctypes.c_void_p), ("base_dev", ctypes.c_void_p),
        ("counts_dev", ctypes.c_void_p), ("rewards_dev", ctypes.c_void_p), ("lengths_dev", ctypes.c_void_p),
        ("when_dev", ctypes.c_void_p), ("missions_dev", ctypes.c_void_p), ("remaining_dev", ctypes.c_void_p),
    ]


class MgxError(RuntimeError):
    pass


_lib = None


def load():
    """Load libmgx.so; fails loudly when the HIP extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MgxError("libmgx.so not found at %s -- run `python __graft_entry__.py build` "
                       "(the engine has no CPU fallback)" % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH)
    P, I, I64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    L.mgx_last_error.restype = ctypes.c_char_p
    L.mgx_abi_version.restype = I
    L.mgx_create.argtypes = [ctypes.POINTER(MgxConfig), I, ctypes.POINTER(P)]
    L.mgx_destroy.argtypes = [P]
    L.mgx_reset.argtypes = [P, ctypes.POINTER(MgxObs), P, P]
    L.mgx_step.argtypes = [P, P, I, ctypes.POINTER(MgxStepOut), P]
    L.mgx_join.argtypes = [P, P]
    L.mgx_set_seed.argtypes = [P, I64]
    L.mgx_get_config.argtypes = [P, ctypes.POINTER(MgxConfig)]
    L.mgx_gae.argtypes = [P, P, P, P, P, I64, I64, ctypes.c_float, ctypes.c_float, P, P, P, P, P]
    L.mgx_gae_dones.argtypes = [P, P, P, P, I64, I64, ctypes.c_float, ctypes.c_float, P, P, P, P, P]
    L.mgx_poll_error.argtypes = [P, P, ctypes.POINTER(ctypes.c_uint32)]
    L.mgx_stats.argtypes = [P, P, ctypes.POINTER(ctypes.c_uint64)]
    L.mgx_ring_levels.argtypes = [P, P, P]
    L.mgx_random_actions.argtypes = [P, I64, I, ctypes.c_uint64, P, P]
    L.mgx_set_random_policy.argtypes = [P, I, ctypes.c_uint64]
    L.mgx_debug_counters.argtypes = [P, P, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]
    L.mgx_dump_state.argtypes = [P, P] + [P] * 10
    L.mgx_mission_text.argtypes = [I, ctypes.c_char_p, ctypes.c_size_t]
    L.mgx_step_compact.argtypes = [P, P, I, ctypes.POINTER(MgxCompactOut), P]
    L.mgx_observe_compact.argtypes = [P, P, P, P]
    L.mgx_rollout_compact.argtypes = [P, P, I, ctypes.POINTER(MgxRolloutOut), P]
    L.mgx_rollout_compact_gae.argtypes = [P, P, I, ctypes.POINTER(MgxRolloutOut), ctypes.POINTER(MgxGaeArgs), P]
    L.mgx_gather.argtypes = [P, P, P, P, I64, P, I64, P, P, I, P, I, P, P]
    L.mgx_gather_ring.argtypes = [P, P, P, P, I64, I64, P, I64, P, P, I, P, I, P, P]
    L.mgx_policy_blob_words.argtypes = [I]
    L.mgx_policy_blob_words.restype = I64
    L.mgx_policy_act.argtypes = [P, P, P, P, I64, I64, P, I64, P, ctypes.POINTER(MgxPolicy), ctypes.POINTER(MgxActOut), P]
    L.mgx_policy_bootstrap.argtypes = [P, P, P, P, I64, I64, I64, P, ctypes.POINTER(MgxPolicy),
                                       ctypes.POINTER(MgxBootstrap), P]
    L.mgx_policy_moe_scratch_words.argtypes = [I64, I]
    L.mgx_policy_moe_scratch_words.restype = I64
    L.mgx_policy_act_moe.argtypes = [P, P, P, P, I64, I64, P, I64, P, ctypes.POINTER(MgxPolicyMoe),
                                     ctypes.POINTER(MgxActOut), P]
    L.mgx_policy_grad_scratch_words.argtypes = [I, I64, I]
    L.mgx_policy_grad_scratch_words.restype = I64
    L.mgx_policy_backward.argtypes = [P, P, P, P, I64, I64, P, I64, ctypes.POINTER(MgxPolicyGrad), P]
    L.mgx_mission_workspace_words.argtypes = [I64, I]
    L.mgx_mission_workspace_words.restype = I64
    L.mgx_mission_forward.argtypes = [P, I64, I, ctypes.POINTER(MgxMissionParams), P, P, I64, P]
    L.mgx_mission_backward.argtypes = [P, I64, I, ctypes.POINTER(MgxMissionParams), P, P, I64,
                                       ctypes.POINTER(MgxMissionGrads), P]
    L.mgx_mission_forward_rows.argtypes = [P, I64, I, ctypes.POINTER(MgxMissionParams), P, P, I64, P, I64, P]
    L.mgx_mission_backward_rows.argtypes = [P, I64, I, ctypes.POINTER(MgxMissionParams), P, P, I64, P, I64,
                                            ctypes.POINTER(MgxMissionGrads), P]
    L.mgx_ppo_loss_scratch_words.argtypes = [I64]
    L.mgx_ppo_loss_scratch_words.restype = I64
    L.mgx_ppo_loss.argtypes = [I64, ctypes.POINTER(MgxPpoLossArgs), P]
    L.mgx_adam_scratch_words.argtypes = [I64]
    L.mgx_adam_scratch_words.restype = I64
    L.mgx_adam_step.argtypes = [P, P, P, P, I64, ctypes.POINTER(MgxAdamArgs), P, P, I64, P]
    L.mgx_adam_schedule.argtypes = [ctypes.POINTER(MgxAdamArgs), ctypes.POINTER(ctypes.c_double), I64, ctypes.c_int32,
                                    ctypes.POINTER(MgxAdamSched)]
    L.mgx_adam_step_sched.argtypes = [P, P, P, P, I64, ctypes.POINTER(MgxAdamArgs), P, ctypes.c_int32, P, P, P, I64, P]
    L.mgx_eval_record.argtypes = [I64, I64, I64, I64, ctypes.POINTER(MgxEvalRecordArgs), P]
    L.mgx_expert_act.argtypes = [P, P, I, P, P]
    L.mgx_set_clock.argtypes = [P, P, I, ctypes.POINTER(I)]
    L.mgx_clock_words.argtypes = [P, I]
    L.mgx_clock_words.restype = I64
    L.mgx_clock_groups.argtypes = [P, I]
    L.mgx_scene.argtypes = [P, I64, ctypes.POINTER(ctypes.c_uint32), P]
    for name in EXPORTS:
        getattr(L, name).restype = getattr(L, name).restype or I
    if L.mgx_abi_version() != ABI_VERSION:
        raise MgxError("libmgx ABI mismatch")
    _lib = L
    return L


def check(status, what=""):
    if status != MGX_OK:
        raise MgxError("%s failed (status %d): %s" % (what, status, load().mgx_last_error().decode()))


def check_tensor(t, what, dtype, numel, device=None):
    """`t`, if it is a contiguous tensor of `dtype` with `numel` elements (None: any number) on `device` (None: any):
    what a library call's wrapper asks of a tensor it passes.  ValueError naming the argument otherwise or if None."""
    if t is None or t.dtype != dtype or not t.is_contiguous() or numel not in (None, t.numel()) or \
            (device is not None and t.device != torch.device(device)):
        raise ValueError("%s must be a contiguous %s tensor%s%s" %
                         (what, dtype, "" if numel is None else " of %d elements" % numel,
                          "" if device is None else " on %s" % (device,)))
    return t


def mission_text(mission_id):
    buf = ctypes.create_string_buffer(64)
    check(load().mgx_mission_text(int(mission_id), buf, 64), "mgx_mission_text")
    return buf.value.decode()


# TokenizeVocabWrapper's vocabulary (environment.py:75-81): ' ' '\n' '-' ':' ',' '.' then a..z
_VOCAB = {c: i for i, c in enumerate(" \n-:,." + "abcdefghijklmnopqrstuvwxyz")}


def tokenize(text):
    """TokenizeVocabWrapper.observation (environment.py:91-112): lower-cased mission text ->
    32 vocabulary indices, zero-padded."""
    out = [0] * 32
    for i, c in enumerate(text.lower()[:32]):
        out[i] = _VOCAB.get(c, 0)
    return out


def mission_tokens():
    """u8 [256][32]: the tokens of every mission id (rows of unused ids are zeros) -- what the
    engine's compact rows carry as one mission-id byte."""
    import numpy as np
    tab = np.zeros((256, 32), np.uint8)
    buf = ctypes.create_string_buffer(64)
    L = load()
    for mid in range(256):
        if L.mgx_mission_text(mid, buf, 64) == MGX_OK:
            tab[mid] = tokenize(buf.value.decode())
    return tab
