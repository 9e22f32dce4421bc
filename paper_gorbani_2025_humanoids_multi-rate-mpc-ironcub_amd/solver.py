"""Host-side mirror of the reference's operator surface for the MPC path, on top of the C-ABI.

`BatchedVSMPC`            the batch driver (what bench.py and the parity tests call).
`VariableSamplingMPC`     one instance with the reference's method names
                          (momentum-based-linear-mpc-lib/bindings/python/MPCPyBindings.cpp:22-90,
                          include/variableSamplingMPC/variableSamplingMPC.h:15-41): configure / update /
                          solveMPC / get*Reference, including "consume the solution only if Solved"
                          (variableSamplingMPC.cpp:91) and the joint accumulator (:104-108).

All numerics run in libvsmpc.so (HIP).  There is no CPU path here.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from . import layout as L
from .jet_model import JetModel


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _dptr(t):
    """the device pointer of a torch tensor, or NULL for None"""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(t, stream):
    """the stream argument of a device entry: `stream`, or torch's current stream on the device of `t`"""
    import torch
    s = stream if stream is not None else torch.cuda.current_stream(t.device)
    return ctypes.c_void_p(s.cuda_stream)


def _assert_f64_device(*tensors):
    """the inputs of a device entry: contiguous float64 CUDA tensors (None: an optional one that is not given)"""
    import torch
    for t in tensors:
        assert t is None or (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous())


KERNEL_FORM_AUTO, KERNEL_FORM_STRUCTURED, KERNEL_FORM_SYRK = 0, 1, 2
# columns of the certificate of BatchedVSMPC.certify (VSMPC_CERT_* in include/vsmpc.h)
CERT_STATIONARITY, CERT_STAT_SCALE, CERT_PRIMAL = L.CERT_STATIONARITY, L.CERT_STAT_SCALE, L.CERT_PRIMAL
CERT_COMPLEMENTARITY, CERT_OBJECTIVE, CERT_DUAL_MAX = L.CERT_COMPLEMENTARITY, L.CERT_OBJECTIVE, L.CERT_DUAL_MAX
CERT_SIZE = L.CERT_SIZE


def certified(cert: np.ndarray, x_scale, tol: float = 1e-9) -> np.ndarray:
    """Per instance: does the certificate `cert` [batch, CERT_SIZE] of BatchedVSMPC.certify pass the three relative tests
    STATIONARITY <= tol STAT_SCALE, PRIMAL <= tol max(1, x_scale), COMPLEMENTARITY <= tol max(1, DUAL_MAX)?  `x_scale`
    is |x|_inf per instance (or the primals [batch, n_var] themselves).  A NaN field (non-finite data) fails."""
    cert = np.asarray(cert, dtype=np.float64)
    xs = np.asarray(x_scale, dtype=np.float64)
    if xs.ndim == 2:
        xs = np.abs(xs).max(axis=1)
    with np.errstate(invalid="ignore"):
        return ((cert[:, CERT_STATIONARITY] <= tol * cert[:, CERT_STAT_SCALE])
                & (cert[:, CERT_PRIMAL] <= tol * np.maximum(1.0, xs))
                & (cert[:, CERT_COMPLEMENTARITY] <= tol * np.maximum(1.0, cert[:, CERT_DUAL_MAX])))


def pack_tunables(handle_or_solver, configs) -> np.ndarray:
    """vsmpc_pack_tunables: the per-instance rows [len(configs), L.TUNE_SIZE] of `configs` (MPCConfig objects) for a
    handle (a BatchedVSMPC, or its raw handle).  A row is opaque: the weights and the throttle box in the form the kernels
    keep them in.  A configuration that differs from the handle's in a structural field (horizon sizes, periods,
    use_jet_dynamic) or fails the value checks raises VsmpcError naming the field."""
    h = getattr(handle_or_solver, "_h", handle_or_solver)
    configs = list(configs)
    arr = (L.CConfig * max(1, len(configs)))(*[c.to_c() for c in configs])
    out = np.empty((len(configs), L.TUNE_SIZE))
    _lib.check(_lib.load().vsmpc_pack_tunables(h, arr, len(configs), _ptr(out)), "vsmpc_pack_tunables")
    return out


class BatchedVSMPC:
    """`max_batch` independent MPC instances on one GPU (one workgroup per instance)."""

    def __init__(self, cfg: L.MPCConfig | None = None, device: int = 0, max_batch: int = 256, runtime: str = "never",
                 sensitivity: bool = False, tunables: bool = False, certify: bool = False, adjoint: bool = False,
                 adjoint_record: bool = False):
        """runtime: "never" -- the tuned kernel of a tabled horizon, other horizons are refused (vsmpc_create);
        "fallback" -- the runtime-sized kernel where the table has no instantiation; "always" -- the runtime-sized kernel
        for every horizon (vsmpc_create_ex, include/vsmpc.h).  sensitivity: also allocate what solve_sensitivity needs
        (VSMPC_CREATE_SENSITIVITY).  tunables: also allocate the staging of solve(records, configs=...), one row of
        weights and throttle box per instance (VSMPC_CREATE_TUNABLES).  certify: also allocate the staging of
        certify(records, x) (VSMPC_CREATE_CERTIFY).  adjoint: also allocate what solve_adjoint needs (VSMPC_CREATE_ADJOINT).
        adjoint_record: also allocate what solve_adjoint_record needs (VSMPC_CREATE_ADJOINT_RECORD; it includes `adjoint`)."""
        if runtime not in L.RUNTIME_MODES:
            raise ValueError(f"runtime must be one of {sorted(L.RUNTIME_MODES)}, not {runtime!r}")
        self.cfg = cfg or L.paper_config()
        self.lib = _lib.load()
        self._ccfg = self.cfg.to_c()
        self._h = ctypes.c_void_p()
        self.adjoint_record = bool(adjoint_record)
        if runtime == "never" and not sensitivity and not tunables and not certify and not adjoint and not adjoint_record:
            _lib.check(self.lib.vsmpc_create(ctypes.byref(self._ccfg), device, max_batch, ctypes.byref(self._h)),
                       "vsmpc_create")
        else:
            flags = (L.RUNTIME_MODES[runtime] | (L.CREATE_SENSITIVITY if sensitivity else 0)
                     | (L.CREATE_TUNABLES if tunables else 0) | (L.CREATE_CERTIFY if certify else 0)
                     | (L.CREATE_ADJOINT if adjoint else 0) | (L.CREATE_ADJOINT_RECORD if adjoint_record else 0))
            _lib.check(self.lib.vsmpc_create_ex(ctypes.byref(self._ccfg), device, max_batch, flags, ctypes.byref(self._h)),
                       "vsmpc_create_ex")
        self.device = device
        self.max_batch = max_batch
        self.n_var = self.lib.vsmpc_num_variables(self._h)
        self.n_con = self.lib.vsmpc_num_constraints(self._h)
        self.n_in = self.lib.vsmpc_input_doubles(self._h)
        self.n_p = self.lib.vsmpc_condensed_dim(self._h)
        self.n_v = self.lib.vsmpc_num_throttle_unknowns(self._h)
        assert self.n_var == self.cfg.n_var and self.n_in == self.cfg.n_in and self.n_con == self.cfg.n_con

    def set_kernel_form(self, form: int) -> int:
        """vsmpc_set_kernel_form (include/vsmpc.h): how this handle's solve kernel condenses the QP (structured
        forward / adjoint recursions, or sensitivity recursion + SYRK); returns the previous setting."""
        prev = self.lib.vsmpc_set_kernel_form(self._h, int(form))
        if prev < 0:
            raise ValueError(f"kernel form {form}: {self.lib.vsmpc_strerror(prev).decode()}")
        return prev

    SMALL_BATCH_MODES = {"auto": 0, "never": 1, "always": 2}

    def set_small_batch_kernel(self, mode) -> int:
        """vsmpc_set_small_batch_kernel (include/vsmpc.h): which kernel serves batches that do not exceed the device's
        CUs -- "auto" (0) the small-batch kind there, "never" (1), "always" (2) where the horizon has the kind; returns
        the previous setting (0..2)."""
        prev = self.lib.vsmpc_set_small_batch_kernel(self._h, int(self.SMALL_BATCH_MODES.get(mode, mode)))
        if prev < 0:
            raise ValueError(f"small-batch kernel mode {mode}: {self.lib.vsmpc_strerror(prev).decode()}")
        return prev

    def uses_small_batch_kernel(self, batch: int) -> bool:
        """vsmpc_small_batch_kernel_for: does a solve of `batch` instances run on the small-batch kind of the kernel?"""
        r = self.lib.vsmpc_small_batch_kernel_for(self._h, int(batch))
        if r < 0:
            raise ValueError(f"batch {batch}: {self.lib.vsmpc_strerror(r).decode()}")
        return bool(r)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self.lib.vsmpc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def kernel_name(self) -> str:
        return self.lib.vsmpc_kernel_name(self._h).decode()

    @property
    def uses_runtime_kernel(self) -> bool:
        """True when this handle solves with the runtime-sized kernel instead of a tuned per-horizon instantiation."""
        return self.kernel_name == L.RUNTIME_KERNEL_NAME

    def _records(self, a, name: str) -> np.ndarray:
        """`a` as the contiguous float64 records [batch, n_in] that the host entries take"""
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.ndim != 2 or a.shape[1] != self.n_in:
            raise ValueError(f"{name} must be [batch, {self.n_in}]")
        return a

    def _rows(self, B: int, configs, tunables):
        """the rows of per-instance tunables [B, L.TUNE_SIZE]: of `configs` (through pack_tunables) or `tunables` (packed
        already); None when neither is given"""
        if configs is None and tunables is None:
            return None
        if configs is not None and tunables is not None:
            raise ValueError("give configs or tunables, not both")
        rows = pack_tunables(self, configs) if configs is not None else np.ascontiguousarray(tunables, dtype=np.float64)
        if rows.shape != (B, L.TUNE_SIZE):
            raise ValueError(f"one configuration / one row of {L.TUNE_SIZE} tunables per instance ({B})")
        return rows

    # ---- host-buffer entry (vsmpc_solve_batch)
    def solve(self, inputs: np.ndarray, configs=None, tunables=None):
        """vsmpc_solve_batch; with `configs` (one MPCConfig per instance) or `tunables` (their packed rows, pack_tunables)
        vsmpc_solve_batch_tuned: instance i is solved under its own weights and throttle box (needs tunables=True at
        construction)."""
        inputs = self._records(inputs, "inputs")
        B = inputs.shape[0]
        x = np.empty((B, self.n_var))
        fm = np.empty((B, L.FM_SIZE))
        status = np.empty(B, dtype=np.int32)
        iters = np.empty(B, dtype=np.int32)
        rows = self._rows(B, configs, tunables)
        if rows is not None:
            _lib.check(self.lib.vsmpc_solve_batch_tuned(self._h, _ptr(inputs), _ptr(rows), B, _ptr(x), _ptr(fm), _ptr(status),
                                                        _ptr(iters), None), "vsmpc_solve_batch_tuned")
            return x, fm, status, iters
        _lib.check(self.lib.vsmpc_solve_batch(self._h, _ptr(inputs), B, _ptr(x), _ptr(fm), _ptr(status),
                                              _ptr(iters), None), "vsmpc_solve_batch")
        return x, fm, status, iters

    # ---- device-resident entry (vsmpc_solve_batch_device); arguments are torch CUDA tensors
    def solve_device(self, d_in, d_x, d_fm, d_status, d_iters, stream=None):
        _assert_f64_device(d_in)
        _lib.check(self.lib.vsmpc_solve_batch_device(
            self._h, _dptr(d_in), d_in.shape[0], _dptr(d_x), _dptr(d_fm), _dptr(d_status), _dptr(d_iters),
            _stream(d_in, stream)), "vsmpc_solve_batch_device")

    def solve_device_tuned(self, d_in, d_tun, d_x, d_fm, d_status, d_iters, stream=None):
        """vsmpc_solve_batch_tuned_device: solve_device with d_tun [batch, L.TUNE_SIZE], the rows of pack_tunables on the
        device (needs no construction flag)"""
        _assert_f64_device(d_in, d_tun)
        B = d_in.shape[0]
        assert tuple(d_tun.shape) == (B, L.TUNE_SIZE)
        _lib.check(self.lib.vsmpc_solve_batch_tuned_device(
            self._h, _dptr(d_in), _dptr(d_tun), B, _dptr(d_x), _dptr(d_fm), _dptr(d_status), _dptr(d_iters),
            _stream(d_in, stream)), "vsmpc_solve_batch_tuned_device")

    # ---- duals and KKT certificate of given primals (vsmpc_certify_batch); needs certify=True at construction
    def certify(self, records: np.ndarray, x: np.ndarray, configs=None, tunables=None, duals: bool = True):
        """vsmpc_certify_batch: (y [B, n_con], cert [B, CERT_SIZE]) of the primals `x` [B, n_var] for `records` -- the
        duals in the reference's row order and OSQP's sign, and the certificate columns CERT_* (include/vsmpc.h).  `x` is
        usually solve()'s, but any x is judged.  With `configs` (one MPCConfig per instance, through pack_tunables) or
        `tunables` (their packed rows) instance i is certified under its own weights and throttle box.  duals=False: y is
        not wanted (returned as None)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        records = self._records(records, "records")
        B = records.shape[0]
        if x.shape != (B, self.n_var):
            raise ValueError(f"x must be [{B}, {self.n_var}]")
        rows = self._rows(B, configs, tunables)
        y = np.empty((B, self.n_con)) if duals else None
        cert = np.empty((B, L.CERT_SIZE))
        _lib.check(self.lib.vsmpc_certify_batch(self._h, _ptr(records), _ptr(x), _ptr(rows), B, _ptr(y), _ptr(cert)),
                   "vsmpc_certify_batch")
        return y, cert

    def certify_device(self, d_in, d_x, d_tun, d_y, d_cert, stream=None):
        """vsmpc_certify_batch_device: torch CUDA tensors (d_tun and d_y may be None), enqueue only; needs no
        construction flag"""
        _assert_f64_device(d_in, d_x, d_tun, d_y, d_cert)
        _lib.check(self.lib.vsmpc_certify_batch_device(self._h, _dptr(d_in), _dptr(d_x), _dptr(d_tun), d_in.shape[0], _dptr(d_y),
                                                       _dptr(d_cert), _stream(d_in, stream)), "vsmpc_certify_batch_device")

    # ---- sensitivities of the solution to X0 (vsmpc_sensitivity_batch); needs sensitivity=True at construction
    def solve_sensitivity(self, inputs: np.ndarray, jacobian: bool = True) -> dict:
        """x, first_move, status, iters as solve(); dx_dx0 [B, n_var, 26] (only when `jacobian`) and dfm_dx0 [B, 24, 26]:
        d x / d X0 and d first_move / d X0; active [B, n_v]: final throttle states (L.ACTIVE_*); flags [B]: L.SENS_*."""
        inputs = self._records(inputs, "inputs")
        B, J = inputs.shape[0], L.N_STATES
        out = {"x": np.empty((B, self.n_var)), "first_move": np.empty((B, L.FM_SIZE)),
               "status": np.empty(B, dtype=np.int32), "iters": np.empty(B, dtype=np.int32),
               "dx_dx0": np.empty((B, self.n_var, J)) if jacobian else None, "dfm_dx0": np.empty((B, L.FM_SIZE, J)),
               "active": np.empty((B, self.n_v), dtype=np.int32), "flags": np.empty(B, dtype=np.int32)}
        _lib.check(self.lib.vsmpc_sensitivity_batch(
            self._h, _ptr(inputs), B, _ptr(out["x"]), _ptr(out["first_move"]), _ptr(out["status"]), _ptr(out["iters"]),
            _ptr(out["dx_dx0"]), _ptr(out["dfm_dx0"]), _ptr(out["active"]), _ptr(out["flags"]), None),
            "vsmpc_sensitivity_batch")
        if not jacobian:
            del out["dx_dx0"]
        return out

    def solve_sensitivity_device(self, d_in, d_x, d_fm, d_status, d_iters, d_dx, d_dfm, d_active, d_flags, stream=None):
        """vsmpc_sensitivity_batch_device: torch CUDA tensors (every output but d_status may be None), enqueue only"""
        _assert_f64_device(d_in)
        p = _dptr
        _lib.check(self.lib.vsmpc_sensitivity_batch_device(
            self._h, p(d_in), d_in.shape[0], p(d_x), p(d_fm), p(d_status), p(d_iters), p(d_dx), p(d_dfm), p(d_active),
            p(d_flags), _stream(d_in, stream)), "vsmpc_sensitivity_batch_device")

    # ---- adjoint of the solve (vsmpc_adjoint_batch); needs adjoint=True at construction
    def solve_adjoint(self, records: np.ndarray, xbar: np.ndarray, fmbar=None, configs=None, tunables=None) -> dict:
        """vsmpc_adjoint_batch: the solve and, for the cotangents `xbar` [B, n_var] = dL/dx and `fmbar` [B, 24] = dL/d
        first_move (or None) of a scalar loss L, its gradients.  x, first_move, status, iters as solve(); grad_x0 [B, 26]
        = dL/dX0; grad_cfg [B, L.GRAD_SIZE] = dL/d(config field) in the order L.GRAD_* (weights and throttle limits in
        percent, as an MPCConfig holds them); active [B, n_v]: final throttle states (L.ACTIVE_*); flags [B]: L.ADJ_*
        (unsolved instances have zero gradients; a degenerate one has the one-sided gradient of its final active set).
        With `configs` (one MPCConfig per instance, through pack_tunables) or `tunables` (their packed rows) instance i is
        solved and differentiated under its own weights and throttle box."""
        return self._solve_adjoint(False, records, xbar, fmbar, configs, tunables)

    def solve_adjoint_record(self, records: np.ndarray, xbar: np.ndarray, fmbar=None, configs=None, tunables=None) -> dict:
        """vsmpc_adjoint_record_batch (needs adjoint_record=True at construction): everything solve_adjoint returns, bit
        for bit, and grad_in [B, n_in] = dL/d(record entry) in the layout of the record (L.RECORD_FIELDS;
        grad_in[:, :26] is grad_x0, the hold flag and the entries nothing reads get 0) and grad_model
        [B, L.GRAD_MODEL_SIZE] = dL/d(A | Bj | Bt | c) in the layout of linearize() (L.GRAD_MODEL_*)."""
        return self._solve_adjoint(True, records, xbar, fmbar, configs, tunables)

    def _solve_adjoint(self, record: bool, records, xbar, fmbar, configs, tunables) -> dict:
        records = self._records(records, "records")
        B = records.shape[0]
        xbar = np.ascontiguousarray(xbar, dtype=np.float64)
        if xbar.shape != (B, self.n_var):
            raise ValueError(f"xbar must be [{B}, {self.n_var}]")
        if fmbar is not None:
            fmbar = np.ascontiguousarray(fmbar, dtype=np.float64)
            if fmbar.shape != (B, L.FM_SIZE):
                raise ValueError(f"fmbar must be [{B}, {L.FM_SIZE}]")
        rows = self._rows(B, configs, tunables)
        out = {"x": np.empty((B, self.n_var)), "first_move": np.empty((B, L.FM_SIZE)),
               "status": np.empty(B, dtype=np.int32), "iters": np.empty(B, dtype=np.int32),
               "grad_x0": np.empty((B, L.N_STATES)), "grad_cfg": np.empty((B, L.GRAD_SIZE)),
               "active": np.empty((B, self.n_v), dtype=np.int32), "flags": np.empty(B, dtype=np.int32)}
        args = [self._h, _ptr(records), _ptr(rows), _ptr(xbar), _ptr(fmbar), B, _ptr(out["x"]), _ptr(out["first_move"]),
                _ptr(out["status"]), _ptr(out["iters"]), _ptr(out["grad_x0"]), _ptr(out["grad_cfg"]), _ptr(out["active"]),
                _ptr(out["flags"])]
        if record:
            out["grad_in"], out["grad_model"] = np.empty((B, self.n_in)), np.empty((B, L.GRAD_MODEL_SIZE))
            _lib.check(self.lib.vsmpc_adjoint_record_batch(*args, _ptr(out["grad_in"]), _ptr(out["grad_model"]), None),
                       "vsmpc_adjoint_record_batch")
        else:
            _lib.check(self.lib.vsmpc_adjoint_batch(*args, None), "vsmpc_adjoint_batch")
        return out

    def solve_adjoint_device(self, d_in, d_tun, d_xbar, d_fmbar, d_x, d_fm, d_status, d_iters, d_grad_x0, d_grad_cfg,
                             d_active, d_flags, stream=None):
        """vsmpc_adjoint_batch_device: torch CUDA tensors (d_tun, d_fmbar and every output but d_status may be None),
        enqueue only"""
        self._adjoint_device("vsmpc_adjoint_batch_device", (d_in, d_tun, d_xbar, d_fmbar),
                             (d_x, d_fm, d_status, d_iters, d_grad_x0, d_grad_cfg, d_active, d_flags), stream)

    def solve_adjoint_record_device(self, d_in, d_tun, d_xbar, d_fmbar, d_x, d_fm, d_status, d_iters, d_grad_x0, d_grad_cfg,
                                    d_active, d_flags, d_grad_in, d_grad_model, stream=None):
        """vsmpc_adjoint_record_batch_device: solve_adjoint_device's arguments and d_grad_in [B, n_in], d_grad_model
        [B, L.GRAD_MODEL_SIZE] (each may be None), enqueue only"""
        self._adjoint_device("vsmpc_adjoint_record_batch_device", (d_in, d_tun, d_xbar, d_fmbar),
                             (d_x, d_fm, d_status, d_iters, d_grad_x0, d_grad_cfg, d_active, d_flags, d_grad_in, d_grad_model),
                             stream)

    def _adjoint_device(self, entry: str, inputs, outputs, stream):
        """inputs = (d_in, d_tun, d_xbar, d_fmbar), then the batch, `outputs` in the entry's order and the stream"""
        _assert_f64_device(*inputs)
        d_in = inputs[0]
        _lib.check(getattr(self.lib, entry)(self._h, *[_dptr(t) for t in inputs], d_in.shape[0], *[_dptr(t) for t in outputs],
                                            _stream(d_in, stream)), entry)

    def timing_begin(self, stream):
        _lib.check(self.lib.vsmpc_timing_begin(self._h, ctypes.c_void_p(stream.cuda_stream)), "vsmpc_timing_begin")

    def timing_end(self, stream, launches: int) -> float:
        ms = ctypes.c_float(0.0)
        _lib.check(self.lib.vsmpc_timing_end(self._h, ctypes.c_void_p(stream.cuda_stream), launches,
                                             ctypes.byref(ms)), "vsmpc_timing_end")
        return float(ms.value)

    # ---- parity splits
    def linearize(self, inputs: np.ndarray):
        inputs = np.ascontiguousarray(inputs, dtype=np.float64)
        B = inputs.shape[0]
        A = np.empty((B, 26, 26))
        Bj = np.empty((B, 26, 8))
        Bt = np.empty((B, 26, 4))
        c = np.empty((B, 26))
        dt = np.empty(self.cfg.n_iter)
        _lib.check(self.lib.vsmpc_linearize_batch(self._h, _ptr(inputs), B, _ptr(A), _ptr(Bj), _ptr(Bt), _ptr(c),
                                                  _ptr(dt)), "vsmpc_linearize_batch")
        return A, Bj, Bt, c, dt

    def assemble_dense(self, one_input: np.ndarray):
        one_input = np.ascontiguousarray(one_input, dtype=np.float64).reshape(-1)
        H = np.empty((self.n_var, self.n_var))
        g = np.empty(self.n_var)
        Ac = np.empty((self.n_con, self.n_var))
        lo = np.empty(self.n_con)
        hi = np.empty(self.n_con)
        _lib.check(self.lib.vsmpc_assemble_dense(self._h, _ptr(one_input), _ptr(H), _ptr(g), _ptr(Ac), _ptr(lo),
                                                 _ptr(hi)), "vsmpc_assemble_dense")
        return H, g, Ac, lo, hi

    def debug_condensed(self, one_input: np.ndarray):
        one_input = np.ascontiguousarray(one_input, dtype=np.float64).reshape(-1)
        M = np.empty((self.n_p, self.n_p))
        Lf = np.empty((self.n_p, self.n_p))
        _lib.check(self.lib.vsmpc_debug_condensed(self._h, _ptr(one_input), _ptr(M), _ptr(Lf)),
                   "vsmpc_debug_condensed")
        return M, Lf


    def kinematics(self, kin: np.ndarray, records: np.ndarray | None = None):
        """Lambda_lin,B, Lambda_ang,B, I_G from raw Robot quantities (vsmpc_kinematics_batch); optionally patches
        them into `records` in place."""
        kin = np.ascontiguousarray(kin, dtype=np.float64)
        if kin.ndim != 2 or kin.shape[1] != L.KIN_SIZE:
            raise ValueError(f"kin must be [batch, {L.KIN_SIZE}]")
        out = np.empty((kin.shape[0], L.KIN_OUT))
        if records is not None:
            assert records.flags["C_CONTIGUOUS"] and records.shape == (kin.shape[0], self.n_in)
        _lib.check(self.lib.vsmpc_kinematics_batch(self._h, _ptr(kin), kin.shape[0], _ptr(out), _ptr(records)),
                   "vsmpc_kinematics_batch")
        return out[:, 0:24].reshape(-1, 3, 8), out[:, 24:48].reshape(-1, 3, 8), out[:, 48:57].reshape(-1, 3, 3)

    def tick(self, kin: np.ndarray, records: np.ndarray):
        """vsmpc_tick: kinematics terms -> records -> solve in one submission (one synchronisation).  `records` is completed
        in place (LLIN | LANG | INERTIA).  Returns (x, first_move, status, iters) like solve()."""
        kin = np.ascontiguousarray(kin, dtype=np.float64)
        n = kin.shape[0]
        if kin.ndim != 2 or kin.shape[1] != L.KIN_SIZE:
            raise ValueError(f"kin must be [batch, {L.KIN_SIZE}]")
        assert records.dtype == np.float64 and records.flags["C_CONTIGUOUS"] and records.shape == (n, self.n_in)
        x = np.empty((n, self.n_var))
        fm = np.empty((n, L.FM_SIZE))
        st = np.zeros(n, dtype=np.int32)
        it = np.zeros(n, dtype=np.int32)
        _lib.check(self.lib.vsmpc_tick(self._h, _ptr(kin), _ptr(records), n, _ptr(x), _ptr(fm), _ptr(st), _ptr(it), None),
                   "vsmpc_tick")
        return x, fm, st, it

    def provider(self, tree: dict, states: np.ndarray, records: np.ndarray | None = None):
        """vsmpc_provider_batch: the Robot quantities of the path on the simplified tree (robot_tree.py).  Returns
        (kin[batch, KIN_SIZE], robot[batch, RO_SIZE]); `records`, when given, get the Robot-derived fields patched in
        place (including Lambda_lin / Lambda_ang / I_G through the kinematics kernel, on the device)."""
        from . import robot_tree as RT
        states = np.ascontiguousarray(states, dtype=np.float64)
        if states.ndim != 2 or states.shape[1] != RT.RS_SIZE:
            raise ValueError(f"states must be [batch, {RT.RS_SIZE}]")
        n = states.shape[0]
        kin = np.empty((n, L.KIN_SIZE))
        robot = np.empty((n, RT.RO_SIZE))
        if records is not None:
            assert records.flags["C_CONTIGUOUS"] and records.shape == (n, self.n_in)
        ctree = RT.to_c(tree)
        _lib.check(self.lib.vsmpc_provider_batch(self._h, ctypes.byref(ctree), _ptr(states), n, _ptr(kin), _ptr(robot),
                                                 _ptr(records)), "vsmpc_provider_batch")
        return kin, robot

    def tree_jacobian(self, tree: dict, q: np.ndarray, thrust: np.ndarray, terms: bool = True, jac: bool = True):
        """vsmpc_tree_jacobian_batch: what the kinematic-tree plant of a rollout hands a tick at joints q [B, 8] and thrusts
        [B, 4] (base at the origin, identity attitude) -- terms [B, 81] = A_mom,body | Lambda_lin,B | Lambda_ang,B | I_B
        (layout.TT_*) -- and their Jacobian jac [B, 81, 12] to (q | thrust).  Returns (terms, jac); either is None when not
        asked for.  Lambda_ang takes its columns through set_kinematics_options' selector."""
        from . import robot_tree as RT
        q = np.ascontiguousarray(q, dtype=np.float64)
        thrust = np.ascontiguousarray(thrust, dtype=np.float64)
        if q.ndim != 2 or q.shape[1] != RT.NJ or thrust.shape != (q.shape[0], RT.NJETS):
            raise ValueError(f"q must be [batch, {RT.NJ}] and thrust [batch, {RT.NJETS}]")
        n = q.shape[0]
        o_terms = np.empty((n, L.TT_SIZE)) if terms else None
        o_jac = np.empty((n, L.TT_SIZE, L.TT_NDIR)) if jac else None
        ctree = RT.to_c(tree)
        _lib.check(self.lib.vsmpc_tree_jacobian_batch(self._h, ctypes.byref(ctree), _ptr(q), _ptr(thrust), n, _ptr(o_terms),
                                                      _ptr(o_jac)), "vsmpc_tree_jacobian_batch")
        return o_terms, o_jac

    def tree_jacobian_device(self, tree: dict, d_q, d_thrust, d_terms=None, d_jac=None, stream=None):
        """vsmpc_tree_jacobian_batch_device on float64 CUDA tensors: d_q [B, 8], d_thrust [B, 4] -> d_terms [B, 81] and / or
        d_jac [B, 81, 12] (None: not wanted).  Only enqueues on `stream` (default: torch's current stream)."""
        from . import robot_tree as RT
        _assert_f64_device(d_q, d_thrust, d_terms, d_jac)
        n = d_q.shape[0]
        assert d_q.shape == (n, RT.NJ) and d_thrust.shape == (n, RT.NJETS)
        assert d_terms is None or d_terms.numel() == n * L.TT_SIZE
        assert d_jac is None or d_jac.numel() == n * L.TT_SIZE * L.TT_NDIR
        ctree = RT.to_c(tree)
        _lib.check(self.lib.vsmpc_tree_jacobian_batch_device(self._h, ctypes.byref(ctree), _dptr(d_q), _dptr(d_thrust), n,
                                                             _dptr(d_terms), _dptr(d_jac), _stream(d_q, stream)),
                   "vsmpc_tree_jacobian_batch_device")

    def set_kinematics_options(self, joint_selector=None, constant_lambda: bool = False):
        """vsmpc_set_kinematics_options: robot joint indices of the controlled joints (Lambda_ang columns; the
        reference selects them by name) and jointsLambdaOption 'constant'."""
        sel = None
        if joint_selector is not None:
            sel = (ctypes.c_int * 8)(*[int(v) for v in joint_selector])
        _lib.check(self.lib.vsmpc_set_kinematics_options(self._h, sel, 1 if constant_lambda else 0),
                   "vsmpc_set_kinematics_options")

    def phase_cycles(self, inputs: np.ndarray) -> np.ndarray:
        """Diagnostic build only: per-instance s_memtime stamps at the phase boundaries, [batch, 16]."""
        inputs = np.ascontiguousarray(inputs, dtype=np.float64)
        st = np.zeros((inputs.shape[0], 16), dtype=np.uint64)
        _lib.check(self.lib.vsmpc_debug_phase_cycles(self._h, _ptr(inputs), inputs.shape[0], _ptr(st)),
                   "vsmpc_debug_phase_cycles")
        return st


class VariableSamplingMPC:
    """Single-instance wrapper with the reference's method names (MPCPyBindings.cpp:22-90).

    The reference's update(QPInput) pulls the per-tick quantities out of a live iDynTree-backed Robot;
    that kinematics provider is outside the path, so `update` takes the already
    extracted input record (layout.IN_*), which is exactly what the device path consumes.  This class carries the
    joint accumulator and "consume only if Solved"; the tick-state fields of the record (hold flag, unwrapped RPY,
    reference window, alpha cursor) are the caller's here -- `reference_api.VariableSamplingMPC` is the mirror that
    takes a QPInput and runs the reference's whole tick state machine itself.
    """

    N_ROBOT_JOINTS = 23  # MPCPyBindings.cpp:43 hard-codes 23 joints
    JOINT_OFFSET = 3     # controlled joints occupy robot joints 3..10 (systemDynamicsVSMPC.cpp:348)

    def __init__(self):
        self._solver = None
        self._record = None
        self._status = 0

    def configure(self, cfg: L.MPCConfig, initial_joint_positions=None, device: int = 0) -> bool:
        self._solver = BatchedVSMPC(cfg, device=device, max_batch=1)
        self.cfg = cfg
        q0 = np.zeros(self.N_ROBOT_JOINTS) if initial_joint_positions is None else np.asarray(initial_joint_positions, float)
        self._jointsPositionReference = q0.copy()   # variableSamplingMPC.cpp:59-60
        self._thrustReference = np.zeros(4)
        self._thrustDotReference = np.zeros(4)
        self._throttleReference = np.zeros(4)       # stored as warped v (variableSamplingMPC.cpp:100)
        # what getThrottleReference returns before the first Solved tick: destandardizeThrottle_u2T of the zero-initialised
        # warped throttle, as the reference's getter computes it from its stored member (variableSamplingMPC.cpp:138-151)
        self._throttlePercent = np.array([JetModel().destandardizeThrottle_u2T(0.0)] * 4)
        self._deltaJoints = np.zeros(8)
        self._QPSolution = np.zeros(cfg.n_var)
        self._finalState = np.zeros(26)
        return True

    def update(self, record: np.ndarray) -> bool:
        rec = np.asarray(record, dtype=np.float64).reshape(-1)
        if rec.size != self.cfg.n_in:
            return False
        self._record = rec
        return True

    def solveMPC(self) -> bool:
        x, fm, status, _ = self._solver.solve(self._record[None, :])
        self._status = int(status[0])
        if self._status == L.STATUS_SOLVED:          # variableSamplingMPC.cpp:91
            self._QPSolution = x[0]
            self._deltaJoints = fm[0, L.FM_DQ:L.FM_DQ + 8]
            self._throttleReference = fm[0, L.FM_V0:L.FM_V0 + 4]
            self._throttlePercent = fm[0, L.FM_THROTTLE:L.FM_THROTTLE + 4]
            self._thrustReference = fm[0, L.FM_THRUST:L.FM_THRUST + 4]
            self._thrustDotReference = fm[0, L.FM_THRUSTDOT:L.FM_THRUSTDOT + 4]
            self._finalState = x[0, 26 * self.cfg.n_iter:26 * (self.cfg.n_iter + 1)]
            sel = slice(self.JOINT_OFFSET, self.JOINT_OFFSET + 8)
            self._jointsPositionReference[sel] += self._deltaJoints   # variableSamplingMPC.cpp:104-108
        return True                                   # the reference returns true regardless (:111)

    def getQPProblemStatus(self) -> int:
        return self._status

    def getJointsReferencePosition(self):
        return self._jointsPositionReference.copy()

    def getThrottleReference(self):
        return np.array(self._throttlePercent, copy=True)

    def getThrustReference(self):
        return np.array(self._thrustReference, copy=True)

    def getThrustDotReference(self):
        return np.array(self._thrustDotReference, copy=True)

    def getMPCSolution(self):
        return self._QPSolution[self.cfg.off_joints:].copy()

    def getFinalCoMPosition(self):
        return self._finalState[0:3].copy()

    def getFinalLinMom(self):
        return self._finalState[3:6].copy()

    def getFinalRPY(self):
        return self._finalState[6:9].copy()

    def getFinalAngMom(self):
        return self._finalState[9:12].copy()

    def getNStatesMPC(self) -> float:
        return 26.0

    def getNInputMPC(self) -> float:
        return 12.0
