"""Rank-deficient and vanishing Lambda = [Lambda_lin,B; Lambda_ang,B] (plain helper module, imported by tests).

The joint reduction p0_joint_reduction (csrc/vsmpc_kernels.hip) is the Householder QR of (Lambda W^-1/2)^T; a pivot column
whose squared norm is not above 1e-300 gets no reflector (beta = 0) and leaves a zero column in R^T.  Idle jets before
take-off (Lambda = 0) is how a flight starts.  The variants below are written on top of two tie-broken records of
tests/record_cases.py: distinct_records(cfg)[2] (free, saturating, 2 to 5 active-set iterations) and [3] (held).  They are
NOT part of record_cases.EDGE: other tests hold measured constants over that table.
"""
import numpy as np

import record_cases as rc

ROWS = slice(0, 48)       # IN_LLIN (3 x 8) followed by IN_LANG (3 x 8), as one 6 x 8 row-major matrix from IN_LLIN on


def _zero(L):
    L[:] = 0.0


def _rank3(L):
    L[3:6] = L[0:3]


def _lin_zero(L):
    L[0:3] = 0.0


def _ang_zero(L):
    L[3:6] = 0.0


def _row1_zero(L):
    L[1] = 0.0


def _first_pivot_zero(L):
    L[0] = 0.0


def _last_pivot_zero(L):
    L[5] = 0.0


def _combination(L):
    L[2] = 2.0 * L[0] - 3.0 * L[1]        # a pivot of rounding noise, not exactly zero


def _two_columns(L):
    L[:, ZERO_COLUMNS] = 0.0


def _one_joint(L):
    keep = L[:, 4].copy()
    L[:] = 0.0
    L[:, 4] = keep


def _scaled(f):
    def apply(L):
        L *= f
    return apply


ZERO_COLUMNS = [2, 5]
VARIANTS = {
    "zero": _zero, "rank3_lin_eq_ang": _rank3, "lin_zero": _lin_zero, "ang_zero": _ang_zero, "rank5_row1_zero": _row1_zero,
    "first_pivot_zero": _first_pivot_zero, "last_pivot_zero": _last_pivot_zero, "rank5_combination": _combination,
    "two_joint_columns_zero": _two_columns, "one_joint_only": _one_joint, "scaled_1e-8": _scaled(1e-8),
    "scaled_1e-140": _scaled(1e-140),     # sk about 1e-281, above the switch: reflectors with beta about 1e280
    "scaled_1e-152": _scaled(1e-152),     # below the switch
}
# joints whose optimum is the closed form U[k] = -w_reg q_err[k] / (w_dq[k] + w_reg) in every block: their column of Lambda is 0
CLOSED_FORM_JOINTS = {"zero": list(range(8)), "two_joint_columns_zero": ZERO_COLUMNS,
                      "one_joint_only": [0, 1, 2, 3, 5, 6, 7]}
# Ceilings on what the numpy route with the joint reduction (algo_model.solve_model(reduce=True), both condensing forms)
# reaches on those joints against the closed form, relative to the largest of them, over the three tabled horizons, the
# default weights and config_cases.JOINT_SPREAD (tests/test_lambda_cases.py asserts them; measured 1.5e-16, 6.1e-10 and
# 1.2e-10, profiles/lambda_cases.txt: where other joints of the block are of order 0.05, the zero-column joints of order
# 1e-5 take the block's rounding).  The device's bars are 100 times the ceilings.
CLOSED_FORM_WORST = {"zero": 2e-16, "two_joint_columns_zero": 6.5e-10, "one_joint_only": 1.3e-10}
CLOSED_FORM_BAR = {k: 100 * v for k, v in CLOSED_FORM_WORST.items()}
JOINT_BLOCK_BAR = 1e-8     # the joint block against the oracle's, relative to its own maximum: the project's parity bar


def records(cfg, layout):
    """(names, records): every variant on the free and on the held base record"""
    base = rc.distinct_records(cfg)
    names, out = [], []
    for i, kind in ((2, "free"), (3, "held")):
        assert (base[i][layout.IN_HOLD] != 0.0) == (kind == "held")
        for v, apply in VARIANTS.items():
            r = base[i].copy()
            L = r[layout.IN_LLIN:layout.IN_LLIN + 48].reshape(6, 8)       # a view
            apply(L)
            names.append(f"{v}/{kind}")
            out.append(r)
    return names, np.ascontiguousarray(np.array(out))


def closed_form_joints(rcfg, layout, rec, joints):
    """U[k] of the joints whose column of Lambda is zero: they see their own cost only"""
    w = np.asarray(rcfg.w_delta_joint, dtype=float)[joints] + rcfg.w_reg_joint_pos
    return -rcfg.w_reg_joint_pos * rec[layout.IN_QERR:layout.IN_QERR + 8][joints] / w


def joint_block_error(rcfg, x, x_ref):
    """the joint block on its own, relative to its own maximum (with Lambda = 0 the joints are 1e-5 next to states of 200)"""
    a, b = x[rcfg.off_joints:rcfg.off_throttle], x_ref[rcfg.off_joints:rcfg.off_throttle]
    return float(np.abs(a - b).max() / np.abs(b).max())
