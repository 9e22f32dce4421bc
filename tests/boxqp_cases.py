"""Records for every way into the throttle box QP of the tuned solve kernels (plain helper module, imported by tests).

box_qp (csrc/vsmpc_p4.hpp) picks its path by the size of the FIRST violated set -- how many throttles of the solve with
only the hold pin enforced leave their box (config_cases.first_violated):

  never          0        the box QP is not entered (its set-up still runs beside the throttle sweep)
  one            1        dual form, wavefront 0 forms the one column of P itself
  two            2        dual form, the columns of the first active set one per wavefront
  three_four     3..4     the same, three or four wavefronts
  five_sixteen   5..16    dual form, all columns of P up front; the register solvers up to 6 and up to 16 active bounds
  above_sixteen  > 16     primal form on the Schur complement

The entries are (workload, index, hold, size): record `index` of synth.make_batch(cfg, ., workload) with the hold flag
forced to `hold`, picked on the CPU with the oracle (test_boxqp_cases.py keeps the table honest).  DEFAULT is at the
default configuration, NARROW at config_cases.EDGE["throttle_box_45_55"] (previous throttles clipped into the box, as
config_cases.edge_records does), where most records start with more than ten violated bounds."""
import importlib

import numpy as np

import config_cases as cc

CLASSES = {"never": (0, 0), "one": (1, 1), "two": (2, 2), "three_four": (3, 4), "five_sixteen": (5, 16),
           "above_sixteen": (17, 10 ** 6)}

DEFAULT = {
    "never": [("hover", 0, 0, 0), ("montecarlo", 0, 0, 0), ("takeoff", 2, 0, 0), ("hover", 0, 1, 0), ("montecarlo", 0, 1, 0),
              ("takeoff", 2, 1, 0)],
    "one": [("hover", 29, 0, 1), ("montecarlo", 14, 0, 1), ("takeoff", 82, 0, 1), ("hover", 170, 1, 1)],
    "two": [("hover", 17, 0, 2), ("montecarlo", 24, 0, 2), ("takeoff", 33, 0, 2), ("hover", 19, 1, 2), ("montecarlo", 75, 1, 2),
            ("takeoff", 19, 1, 2)],
    "three_four": [("hover", 4, 0, 3), ("hover", 19, 0, 4), ("montecarlo", 44, 0, 3), ("hover", 222, 1, 3),
                   ("montecarlo", 35, 1, 3), ("montecarlo", 19, 1, 4)],
    "five_sixteen": [("hover", 222, 0, 5), ("montecarlo", 4, 0, 6), ("montecarlo", 66, 0, 5), ("takeoff", 0, 0, 12),
                     ("takeoff", 92, 0, 16), ("montecarlo", 4, 1, 5), ("takeoff", 0, 1, 10), ("takeoff", 1, 1, 14),
                     ("takeoff", 5, 1, 15)],
    "above_sixteen": [("takeoff", 1, 0, 17), ("takeoff", 5, 0, 18), ("takeoff", 54, 0, 23), ("takeoff", 54, 1, 19)],
}
NARROW = {
    "five_sixteen": [("hover", 4, 0, 16), ("hover", 20, 0, 14), ("hover", 8, 0, 13), ("hover", 10, 1, 14), ("hover", 4, 1, 13),
                     ("hover", 6, 1, 11)],
    "above_sixteen": [("hover", 19, 0, 24), ("hover", 17, 0, 22), ("hover", 18, 0, 19), ("hover", 19, 1, 20), ("hover", 17, 1, 17),
                      ("takeoff", 0, 1, 20)],
}
TABLES = {"default": ({}, DEFAULT), "narrow": (cc.EDGE["throttle_box_45_55"], NARROW)}


def _mod(name):
    return importlib.import_module(f"{cc.PKG}.{name}")


def entries(table):
    """the table's entries in one list, class by class: (class, workload, index, hold, size)"""
    return [(name,) + e for name, rows in TABLES[table][1].items() for e in rows]


def batch(ref, table):
    """(MPCConfig, oracle Config, records) of a table, paper horizon, one record per entry, in entries() order"""
    L, synth = _mod("layout"), _mod("synth")
    settings, _ = TABLES[table]
    cfg, rcfg = cc.configs(ref, cc.PAPER, settings)
    recs = []
    for _, workload, index, hold, _ in entries(table):
        rec = synth.make_batch(cfg, 1, workload=workload, first_index=index)[0]
        rec[L.IN_HOLD] = float(hold)
        if table == "narrow":
            rec[L.IN_UPREV:L.IN_UPREV + 4] = np.clip(rec[L.IN_UPREV:L.IN_UPREV + 4], 46.0, 54.0)
        recs.append(rec)
    return cfg, rcfg, np.ascontiguousarray(np.array(recs))
