"""ctypes binding of include/vsmpc.h.  Loading fails loudly when libvsmpc.so is missing: there is
no CPU fallback anywhere in the product path."""
from __future__ import annotations

import ctypes
import os

from .layout import CConfig

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libvsmpc.so")

vp = dp = fp = ctypes.c_void_p   # handles and streams, arrays of double, arrays of float
ip, c_int, c_double, c_float = ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_double, ctypes.c_float
cfgp, outp = ctypes.POINTER(CConfig), ctypes.POINTER(ctypes.c_void_p)
_SOLVE = [vp, dp, c_int, dp, dp, vp, vp, vp]                         # h, in, batch, x, first_move, status, iters, stream
_ADJOINT = [vp, dp, dp, dp, dp, c_int, dp, dp, vp, vp, dp, dp, vp, vp]   # h, in, tunables, xbar, fmbar, batch, x, first_move,
#                                                                          status, iters, grad_x0, grad_cfg, active, adj_flags

# every symbol include/vsmpc.h and include/vsmpc_jet.h declare: its argument types, and its result type where that is not int
SIGNATURES = {
    "vsmpc_create": [cfgp, c_int, c_int, outp],
    "vsmpc_create_ex": [cfgp, c_int, c_int, ctypes.c_uint, outp],
    "vsmpc_destroy": ([vp], None),
    "vsmpc_num_variables": [vp], "vsmpc_num_constraints": [vp], "vsmpc_input_doubles": [vp], "vsmpc_max_batch": [vp],
    "vsmpc_condensed_dim": [vp], "vsmpc_num_throttle_unknowns": [vp],
    "vsmpc_solve_batch": _SOLVE, "vsmpc_solve_batch_device": _SOLVE,
    "vsmpc_pack_tunables": [vp, cfgp, c_int, dp],
    # h, in, tunables, batch, x, first_move, status, iters, stream
    "vsmpc_solve_batch_tuned": [vp, dp, dp, c_int, dp, dp, vp, vp, vp],
    "vsmpc_solve_batch_tuned_device": [vp, dp, dp, c_int, dp, dp, vp, vp, vp],
    "vsmpc_rollout_set_tunables": [vp, dp],
    "vsmpc_rollout_set_noise": [vp, vp],                                 # r, vsmpc_noise* (layout.CNoise) or NULL
    "vsmpc_rollout_noise_draws": [vp, c_int, c_int, dp, vp],             # r, tick0, ticks, z, words
    # h, in, x, tunables, batch, y, cert (, stream)
    "vsmpc_certify_batch": [vp, dp, dp, dp, c_int, dp, dp], "vsmpc_certify_batch_device": [vp, dp, dp, dp, c_int, dp, dp, vp],
    # h, in, batch, x, first_move, status, iters, dx_dx0, dfm_dx0, active, sens_flags, stream
    "vsmpc_sensitivity_batch": [vp, dp, c_int, dp, dp, vp, vp, dp, dp, vp, vp, vp],
    "vsmpc_sensitivity_batch_device": [vp, dp, c_int, dp, dp, vp, vp, dp, dp, vp, vp, vp],
    "vsmpc_adjoint_batch": _ADJOINT + [vp], "vsmpc_adjoint_batch_device": _ADJOINT + [vp],          # ..., stream
    "vsmpc_adjoint_record_batch": _ADJOINT + [dp, dp, vp],                                          # ..., grad_in, grad_model, stream
    "vsmpc_adjoint_record_batch_device": _ADJOINT + [dp, dp, vp],
    "vsmpc_linearize_batch": [vp, dp, c_int, dp, dp, dp, dp, dp],
    "vsmpc_assemble_dense": [vp, dp, dp, dp, dp, dp, dp],
    "vsmpc_debug_condensed": [vp, dp, dp, dp],
    "vsmpc_kinematics_batch": [vp, dp, c_int, dp, dp],
    "vsmpc_debug_phase_cycles": [vp, dp, c_int, vp],
    "vsmpc_timing_begin": [vp, vp],
    "vsmpc_timing_end": [vp, vp, c_int, ctypes.POINTER(c_float)],
    "vsmpc_rollout_create": [vp, c_int, dp, dp, c_int, dp, c_int, c_double, outp],
    "vsmpc_rollout_destroy": ([vp], None),
    "vsmpc_rollout_reset": [vp, dp, dp],
    "vsmpc_rollout_run": [vp, c_int, dp, vp],
    "vsmpc_rollout_get_state": [vp, dp], "vsmpc_rollout_get_records": [vp, dp],
    "vsmpc_rollout_run_taped": [vp, c_int, dp, vp],
    # r, log_bar, state_bar, grad_state0, grad_cfg, flags, stream
    "vsmpc_rollout_backward": [vp, dp, dp, dp, dp, vp, vp], "vsmpc_rollout_backward_device": [vp, dp, dp, dp, dp, vp, vp],
    # r, log_bar, state_bar, grad_state0, grad_cfg, grad_params, grad_traj, flags, stream
    "vsmpc_rollout_backward_full": [vp, dp, dp, dp, dp, dp, dp, vp, vp],
    "vsmpc_rollout_backward_full_device": [vp, dp, dp, dp, dp, dp, dp, vp, vp],
    "vsmpc_rollout_traj_grad_size": [vp],
    # r, log_bar, state_bar, grad_state0, grad_cfg, grad_params, grad_traj, grad_att, flags, stream
    "vsmpc_rollout_backward_attitude": [vp, dp, dp, dp, dp, dp, dp, dp, vp, vp],
    "vsmpc_rollout_backward_attitude_device": [vp, dp, dp, dp, dp, dp, dp, dp, vp, vp],
    "vsmpc_rollout_att_grad_size": [vp],
    "vsmpc_rollout_set_trajectories": [vp, dp, dp, dp],
    "vsmpc_alloc_host": ([ctypes.c_size_t], vp),
    "vsmpc_free_host": ([vp], None),
    "vsmpc_set_kernel_form": [vp, c_int], "vsmpc_set_small_batch_kernel": [vp, c_int], "vsmpc_small_batch_kernel_for": [vp, c_int],
    "vsmpc_small_batch_lds_bytes": ([c_int, c_int, c_int], ctypes.c_size_t),
    "vsmpc_set_kinematics_options": [vp, ip, c_int],
    "vsmpc_provider_batch": [vp, vp, dp, c_int, dp, dp, dp],
    # h, tree, q, thrust, batch, terms, jac (, stream)
    "vsmpc_tree_jacobian_batch": [vp, vp, dp, dp, c_int, dp, dp], "vsmpc_tree_jacobian_batch_device": [vp, vp, dp, dp, c_int, dp, dp, vp],
    "vsmpc_rollout_set_attitude_tracks": [vp, dp, dp],
    "vsmpc_rollout_set_attitude_tracks_ex": [vp, dp, dp, ctypes.c_uint],
    "vsmpc_rollout_set_tree": [vp, vp],
    "vsmpc_rollout_set_tree_ex": [vp, vp, ctypes.c_uint],
    "vsmpc_tick": [vp, dp, dp, c_int, dp, dp, vp, vp, vp],
    "vsmpc_rollout_set_jet_plant": [vp, vp, dp, dp],
    "vsmpc_strerror": ([c_int], ctypes.c_char_p),
    "vsmpc_kernel_name": ([vp], ctypes.c_char_p),
    # include/vsmpc_jet.h
    "vsmpc_jet_create": [fp, fp, fp, fp, fp, fp, dp, c_int, c_int, c_int, outp],
    "vsmpc_jet_destroy": ([vp], None),
    "vsmpc_jet_nn_step": [vp, fp, fp, c_int, c_float, fp, fp, fp, fp],
    "vsmpc_jet_nn_sequence": [vp, fp, c_int, c_int, c_float, fp, fp, fp, fp],
    "vsmpc_jet_ekf_update": [vp, dp, dp, dp, dp, c_int, c_double, dp, dp],
    "vsmpc_jet_plant_run": [vp, fp, dp, dp, fp, c_int, c_int, c_int, c_double, dp, dp, dp],
    "vsmpc_jet_plant_run_device": [vp, fp, dp, dp, fp, c_int, c_int, c_int, c_double, dp, dp, dp, vp],
}
EXPORTS = tuple(SIGNATURES)

_lib = None


class VsmpcError(RuntimeError):
    pass


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise VsmpcError(
            f"{LIB_PATH} is missing: build it with `python __graft_entry__.py` (hipcc --offload-arch=gfx950). "
            "The batched MPC path has no CPU fallback.")
    try:  # share torch's HIP runtime (same SONAME) when torch is in the process
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch is optional for the C-ABI itself
        pass
    lib = ctypes.CDLL(LIB_PATH)
    for name, sig in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = (list(sig[0]), sig[1]) if isinstance(sig, tuple) else (list(sig), c_int)
    _lib = lib
    return lib


def check(code: int, what: str = "vsmpc"):
    if code != 0:
        msg = load().vsmpc_strerror(code).decode()
        raise VsmpcError(f"{what} failed ({code}): {msg}")
