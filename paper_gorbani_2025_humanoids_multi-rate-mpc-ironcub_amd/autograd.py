"""The MPC solve as a differentiable torch operation: a loss on the plan backpropagates to the measured state X0 and to the
gains (the weights and the throttle box) through vsmpc_adjoint_batch_device -- one more linear solve per instance with the
factor the solver holds, no Jacobian ("Adjoint").

    mpc = BatchedVSMPC(cfg, max_batch=B, adjoint=True)
    x, first_move, status = plan(mpc, records, x0, gains)        # records [B, n_in], x0 [B, 26], gains [B, GRAD_SIZE]
    loss(x, first_move).backward()                               # x0.grad, gains.grad

On a handle created with adjoint_record=True the record itself is differentiable too -- the reference window, the previous
throttle, the linearisation point, the posture error and the model data -- through vsmpc_adjoint_record_batch_device
("Adjoint of the record"):

    mpc = BatchedVSMPC(cfg, max_batch=B, adjoint_record=True)
    x, first_move, status = plan(mpc, records.requires_grad_(), x0, gains)
    loss(x, first_move).backward()                               # records.grad (zero in the X0 columns), x0.grad, gains.grad

A whole closed loop is differentiable too -- a loss on the flown trajectory backpropagates through every tick to the initial
plant state and to the gains, in one backward sweep over the tape of the forward run ("Adjoint of the rollout"):

    ro = ClosedLoopRollout(cfg, B, pos, vel, alpha, alpha_dt, adjoint=True)
    log, final_state = rollout(ro, state0, gains, params, ticks)  # state0 [B, 40], gains [B, GRAD_SIZE], params [B, PLANT_PARAMS]
    loss(log, final_state).backward()                            # state0.grad, gains.grad

and so are its plant parameters and its reference tracks ("Adjoint of the rollout: parameters and tracks"):

    log, final_state = rollout(ro, state0, gains, params.requires_grad_(), ticks, traj=(pos, vel, alpha))
    loss(log, final_state).backward()                            # params.grad [B, PLANT_PARAMS]; pos.grad, vel.grad, alpha.grad

and the attitude tracks of the reference ("Adjoint of the rollout: attitude tracks"):

    log, final_state = rollout(ro, state0, gains, params, ticks, att=(rpy, rpy_dot))
    loss(log, final_state).backward()                            # rpy.grad, rpy_dot.grad [n_traj, 3]

All numerics run in libvsmpc.so (HIP); there is no CPU path.
"""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

from . import layout as L
from .solver import BatchedVSMPC, pack_tunables


def gains_of(cfg: L.MPCConfig) -> np.ndarray:
    """the tunable fields of `cfg` as one row of field values in L.GRAD_* order (entry 31 is 0)"""
    row = np.zeros(L.GRAD_SIZE)
    for name, off, n in L.GRAD_FIELDS:
        row[off:off + n] = getattr(cfg, name)
    return row


def configs_of(cfg: L.MPCConfig, gains: np.ndarray) -> list:
    """one MPCConfig per row of `gains` ([B, GRAD_SIZE] field values, L.GRAD_* order): `cfg` with its tunable fields replaced"""
    out = []
    for row in np.asarray(gains, dtype=np.float64):
        kw = {name: (float(row[off]) if n == 1 else tuple(float(v) for v in row[off:off + n])) for name, off, n in L.GRAD_FIELDS}
        out.append(dataclasses.replace(cfg, **kw))
    return out


class PlanFunction(torch.autograd.Function):
    """forward(mpc, records, x0, gains, info) -> (x [B, n_var], first_move [B, 24], status [B] int32)

    Forward: `x0` [B, 26] is written into the X0 columns of a copy of `records` [B, n_in] (CUDA, float64) and the batch is
    solved with the handle's device solve entry: the tuned kernel where the handle has one, and the per-instance-tunables
    kind when `gains` [B, L.GRAD_SIZE] is given.  `gains` holds field values in L.GRAD_* order (weights and throttle limits
    in percent, as an MPCConfig holds them); packing them into the kernels' rows goes through the HOST
    (vsmpc_pack_tunables validates the values), which synchronises the stream once per forward.
    Backward: one vsmpc_adjoint_batch_device call with the incoming cotangents of x and first_move; it returns the gradients
    of x0 and of gains.  On a handle without adjoint_record every other record field is non-differentiable -- the
    linearisation depends on them, and that entry does not compute the derivative -- so `records` must not require grad.  On
    a handle with it the one call is vsmpc_adjoint_record_batch_device and `records` gets the gradient of every entry; since
    `x0` overwrites the X0 columns in the forward pass, that gradient is zero there.  Instances whose status is not Solved contribute
    zero gradient; `info` (a dict, or None) receives "flags" (L.ADJ_*) and "active" of the backward call as CUDA tensors, so
    that a caller can mask unsolved or degenerate instances.  Calls on one handle must be ordered on one stream."""

    @staticmethod
    def forward(ctx, mpc: BatchedVSMPC, records, x0, gains, info):
        if records.requires_grad and not mpc.adjoint_record:
            raise ValueError("records must not require grad: only X0 (passed as x0) and the gains are differentiable "
                             "(the other record entries: a handle created with adjoint_record=True)")
        assert records.is_cuda and records.dtype == torch.float64 and records.shape[1] == mpc.n_in
        B = records.shape[0]
        assert tuple(x0.shape) == (B, L.N_STATES) and x0.dtype == torch.float64
        d_in = records.detach().clone().contiguous()
        d_in[:, L.IN_X0:L.IN_X0 + L.N_STATES] = x0.detach()
        d_tun = None
        if gains is not None:
            assert tuple(gains.shape) == (B, L.GRAD_SIZE) and gains.dtype == torch.float64
            rows = pack_tunables(mpc, configs_of(mpc.cfg, gains.detach().cpu().numpy()))
            d_tun = torch.from_numpy(rows).to(records.device)
        x = torch.empty((B, mpc.n_var), dtype=torch.float64, device=records.device)
        fm = torch.empty((B, L.FM_SIZE), dtype=torch.float64, device=records.device)
        status = torch.empty(B, dtype=torch.int32, device=records.device)
        if d_tun is None:
            mpc.solve_device(d_in, x, fm, status, None)
        else:
            mpc.solve_device_tuned(d_in, d_tun, x, fm, status, None)
        ctx.mpc, ctx.d_in, ctx.d_tun, ctx.info = mpc, d_in, d_tun, info
        ctx.mark_non_differentiable(status)
        return x, fm, status

    @staticmethod
    def backward(ctx, gx, gfm, _gstatus):
        mpc, d_in = ctx.mpc, ctx.d_in
        B, dev = d_in.shape[0], d_in.device
        xbar = torch.zeros((B, mpc.n_var), dtype=torch.float64, device=dev) if gx is None else gx.contiguous()
        fmbar = None if gfm is None else gfm.contiguous()
        status = torch.empty(B, dtype=torch.int32, device=dev)
        g0 = torch.empty((B, L.N_STATES), dtype=torch.float64, device=dev)
        gc = torch.empty((B, L.GRAD_SIZE), dtype=torch.float64, device=dev)
        active = torch.empty((B, mpc.n_v), dtype=torch.int32, device=dev)
        flags = torch.empty(B, dtype=torch.int32, device=dev)
        gin = None
        if ctx.needs_input_grad[1]:
            gin = torch.empty((B, mpc.n_in), dtype=torch.float64, device=dev)
            mpc.solve_adjoint_record_device(d_in, ctx.d_tun, xbar, fmbar, None, None, status, None, g0, gc, active, flags, gin,
                                            None)
            gin[:, L.IN_X0:L.IN_X0 + L.N_STATES] = 0.0       # the forward pass replaced these columns by x0
        else:
            mpc.solve_adjoint_device(d_in, ctx.d_tun, xbar, fmbar, None, None, status, None, g0, gc, active, flags)
        if ctx.info is not None:
            ctx.info["flags"], ctx.info["active"] = flags, active
        return None, gin, (g0 if ctx.needs_input_grad[2] else None), (gc if ctx.needs_input_grad[3] else None), None


def plan(mpc: BatchedVSMPC, records, x0, gains=None, info: dict | None = None):
    """(x, first_move, status) of the batch, differentiable with respect to `x0` and `gains`, and on a handle created with
    adjoint_record=True with respect to `records` (PlanFunction)"""
    return PlanFunction.apply(mpc, records, x0, gains, info)


NS_LIVE = 40   # entries of the plant state the parametric plant uses (the jet-plant slots behind them carry no gradient)


class RolloutFunction(torch.autograd.Function):
    """forward(ro, state0, gains, params, ticks, info, traj_pos, traj_vel, traj_alpha, traj_rpy, traj_rpy_dot, att)
    -> (log [ticks, B, 14], final_state [B, 40])

    Forward: the rollout `ro` (a ClosedLoopRollout created with adjoint=True) is reset to `state0` [B, 40] (CUDA or CPU,
    float64; the jet-plant slots of the plant state are zero) with the plant parameters `params` [B, PLANT_PARAMS] (numpy or
    tensor) and, when `gains` [B, L.GRAD_SIZE] is given, one row of tunables per loop; then `ticks` taped ticks run.  The three
    tracks (tensors of the rollout's own shapes, or None: the rollout's tracks as they are) are written into the rollout with
    set_trajectories first; with `att` the two attitude tracks ([n_traj, 3] tensors, or None: all zero) are written with
    set_attitude_tracks(.., adjoint=True), without it the rollout's attitude tracks stay as they are.  reset, set_tunables,
    set_trajectories, set_attitude_tracks and the log go through the HOST, as ClosedLoopRollout's own methods do.
    Backward: ONE sweep with the incoming cotangents of the log columns 0..13 and of the final state:
    vsmpc_rollout_backward_device, vsmpc_rollout_backward_full_device when `params` or a track requires grad, or
    vsmpc_rollout_backward_attitude_device when an attitude track does.  `params` gets
    its row per loop (structural columns zero); a track, shared by all loops, gets the sum of the loops' rows (torch.sum over
    the batch: a reduction whose order the shape fixes).  `info` (a dict, or None) receives "flags" (OR over the ticks of
    L.ADJ_*) as a CUDA tensor."""

    @staticmethod
    def forward(ctx, ro, state0, gains, params, ticks, info, traj_pos, traj_vel, traj_alpha, traj_rpy=None, traj_rpy_dot=None,
                att=False):
        B = ro.batch
        assert tuple(state0.shape) == (B, NS_LIVE) and state0.dtype == torch.float64
        st = np.zeros((B, L.PLANT_STATE))
        st[:, :NS_LIVE] = state0.detach().cpu().numpy()
        pa = params.detach().cpu().numpy() if isinstance(params, torch.Tensor) else np.asarray(params, dtype=np.float64)
        if gains is not None:
            assert tuple(gains.shape) == (B, L.GRAD_SIZE) and gains.dtype == torch.float64
            ro.set_tunables(configs=configs_of(ro.cfg, gains.detach().cpu().numpy()))
        else:
            ro.set_tunables(None)
        tracks = [None if t is None else t.detach().cpu().numpy() for t in (traj_pos, traj_vel, traj_alpha)]
        if any(t is not None for t in tracks):
            ro.set_trajectories(*tracks)
        if att:
            ro.set_attitude_tracks(*[None if t is None else t.detach().cpu().numpy() for t in (traj_rpy, traj_rpy_dot)], adjoint=True)
        ro.reset(st, pa)
        log = ro.run(int(ticks), tape=True)
        dev = state0.device if state0.is_cuda else torch.device("cuda", ro.mpc.device)
        ctx.ro, ctx.info, ctx.dev, ctx.ticks = ro, info, dev, int(ticks)
        ctx.out_dev = state0.device
        ctx.track_devs = [None if t is None else t.device for t in (traj_pos, traj_vel, traj_alpha)]
        ctx.att_devs = [None if t is None else t.device for t in (traj_rpy, traj_rpy_dot)]
        ctx.params_dev = params.device if isinstance(params, torch.Tensor) else None
        return (torch.from_numpy(log[:, :, :14].copy()).to(state0.device),
                torch.from_numpy(ro.state()[:, :NS_LIVE].copy()).to(state0.device))

    @staticmethod
    def backward(ctx, glog, gfinal):
        ro, dev, B = ctx.ro, ctx.dev, ctx.ro.batch
        lb = sb = None
        if glog is not None:
            lb = torch.zeros((ctx.ticks, B, L.ROLLOUT_LOG), dtype=torch.float64, device=dev)
            lb[:, :, :14] = glog.to(dev)
        if gfinal is not None:
            sb = torch.zeros((B, L.PLANT_STATE), dtype=torch.float64, device=dev)
            sb[:, :NS_LIVE] = gfinal.to(dev)
        if lb is None and sb is None:
            return (None,) * 12
        g0 = torch.empty((B, L.PLANT_STATE), dtype=torch.float64, device=dev)
        gg = torch.empty((B, L.GRAD_SIZE), dtype=torch.float64, device=dev)
        flags = torch.empty(B, dtype=torch.int32, device=dev)
        want_p, want_t = ctx.needs_input_grad[3], any(ctx.needs_input_grad[6:9])
        gp = torch.empty((B, L.PLANT_PARAMS), dtype=torch.float64, device=dev) if want_p else None
        gt = torch.empty((B, ro.traj_grad_size), dtype=torch.float64, device=dev) if want_t else None
        want_a = any(ctx.needs_input_grad[9:11])
        ga = torch.empty((B, ro.att_grad_size), dtype=torch.float64, device=dev) if want_a else None
        ro.backward_device(lb, sb, g0, gg, flags, d_grad_params=gp, d_grad_traj=gt, d_grad_att=ga)
        if ctx.info is not None:
            ctx.info["flags"] = flags
        tracks = [None, None, None]
        if want_t:
            total = gt.sum(dim=0)
            for k, (off, n, shape) in enumerate(L.traj_grad_blocks(ro.n_traj, ro.n_alpha).values()):
                if ctx.needs_input_grad[6 + k]:
                    tracks[k] = total[off:off + n].reshape(shape).to(ctx.track_devs[k])
        atts = [None, None]
        if want_a:
            total = ga.sum(dim=0)
            for k, (off, n, shape) in enumerate(L.att_grad_blocks(ro.n_traj).values()):
                if ctx.needs_input_grad[9 + k]:
                    atts[k] = total[off:off + n].reshape(shape).to(ctx.att_devs[k])
        return (None, g0[:, :NS_LIVE].to(ctx.out_dev) if ctx.needs_input_grad[1] else None,
                gg.to(ctx.out_dev) if ctx.needs_input_grad[2] else None, gp.to(ctx.params_dev) if want_p else None, None, None,
                tracks[0], tracks[1], tracks[2], atts[0], atts[1], None)


def rollout(ro, state0, gains, params, ticks: int, info: dict | None = None, traj=None, att=None):
    """(log [ticks, B, 14], final_state [B, 40]) of `ticks` closed-loop ticks from `state0`, differentiable with respect to
    `state0` and `gains`, to `params` when it is a tensor that requires grad ([B, PLANT_PARAMS]), and to the tracks when
    traj = (pos [n_traj, 3], vel [n_traj, 3], alpha [n_alpha]) is given as tensors that require grad (any of the three may be
    None: that track of the rollout stays as it is) (RolloutFunction).
    Plants: the parametric plant, and the kinematic-tree plant when the rollout's tree was set with set_tree(tree, adjoint=True)
    -- `params` then gets +0.0 in the blocks that plant does not read (INERTIA_B, AMOM0, DJ); the tree's own geometry is not
    differentiated.
    att = (rpy [n_traj, 3], rpy_dot [n_traj, 3]), tensors, either may be None (that track is all zero): the attitude tracks of
    the reference, written with set_attitude_tracks(.., adjoint=True) and differentiable where they require grad.  Without
    `att` the rollout's attitude tracks stay as they are.
    The jet plant option, a tree set without adjoint=True and an RPYDot track set without adjoint=True are refused by the
    taped run."""
    pos, vel, alpha = (None, None, None) if traj is None else traj
    rpy, rpy_dot = (None, None) if att is None else att
    return RolloutFunction.apply(ro, state0, gains, params, ticks, info, pos, vel, alpha, rpy, rpy_dot, att is not None)
