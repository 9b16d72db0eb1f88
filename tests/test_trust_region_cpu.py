"""CPU: csrc/trust_region.h on its own — the trust-region policy and the verdict on a trial step that the four Levenberg-Marquardt
solvers share — through dvs_test_trust_region (include/dvslam_hip_test.h; no HIP call), over scripted trial records.

The independent side is written here from tests/ba_bracket.py's docstring (Ceres' schedule: initial radius 1e4; accepted:
radius <- min(1e16, radius / max(1/3, 1 - (2 rho - 1)^3)), factor <- 2; unsuccessful: radius <- radius / factor, factor doubles) and
pose_graph_ref.verdict (invalid, parameter tolerance, function tolerance, rho > 1e-3), plus what the solvers' own comments state: the LM
diagonal is kept across a rejected step only, the fifth invalid step in a row fails the solve, a radius below 1e-32 ends it.  The
hook's numbers are compared with it as bit patterns, and ba_bracket.check_schedule runs over the rows the host's rule produces."""
import ctypes as C
import math
import numpy as np
import ba_bracket
import pose_graph_ref as pgr
from dvslam_amd._lib import test_lib as _hooks

HOST, DEVICE_DECREASE, DEVICE_APPLIED = 0, 1, 2
NAN = float("nan")


class Trial(C.Structure):
    _fields_ = [("valid", C.c_int32), ("accept", C.c_int32), ("model_change", C.c_double), ("cand_cost", C.c_double),
                ("sn", C.c_double), ("xn", C.c_double)]


class Step(C.Structure):
    _fields_ = [("radius_before", C.c_double), ("cost_change", C.c_double), ("rel", C.c_double), ("radius", C.c_double),
                ("decrease_factor", C.c_double), ("kind", C.c_int32), ("reuse_diagonal", C.c_int32), ("invalid", C.c_int32),
                ("reserved", C.c_int32)]


def trial(model_change, cand_cost, valid=1, accept=0, sn=1.0, xn=1.0):
    return dict(valid=valid, accept=accept, model_change=model_change, cand_cost=cand_cost, sn=sn, xn=xn)


def run_hook(mode, trials, x_cost, ftol=0.0, ptol=0.0):
    """-> (rows, termination); a row = (radius before, kind, cost change, rho, radius, factor, reuse_diagonal, invalid count)"""
    fn = _hooks().dvs_test_trust_region
    fn.argtypes = [C.c_int32, C.POINTER(Trial), C.c_int32, C.c_double, C.c_double, C.c_double, C.POINTER(Step), C.POINTER(C.c_int32),
                   C.POINTER(C.c_int32)]
    n = len(trials)
    tin = (Trial * max(n, 1))(*[Trial(t["valid"], t["accept"], t["model_change"], t["cand_cost"], t["sn"], t["xn"]) for t in trials])
    out = (Step * max(n, 1))()
    ns, term = C.c_int32(-1), C.c_int32(-1)
    assert fn(mode, tin, n, x_cost, ftol, ptol, out, C.byref(ns), C.byref(term)) == 0
    rows = [(s.radius_before, s.kind, s.cost_change, s.rel, s.radius, s.decrease_factor, s.reuse_diagonal, s.invalid) for s in out[:ns.value]]
    return rows, term.value


def restate(mode, trials, x_cost, ftol=0.0, ptol=0.0):
    radius, factor, reuse, invalid = 1e4, 2.0, 0, 0
    rows, term, it = [], None, 0
    while term is None:
        if it >= len(trials):
            term = 1
            break
        if radius < 1e-32:
            term = 0
            break
        t = trials[it]
        it += 1
        rec = dict(finite=t["valid"], model_cost_change=t["model_change"], cand_cost=t["cand_cost"], step2=t["sn"], x2=t["xn"])
        kind, change, rho = pgr.verdict(rec, x_cost, dict(parameter_tolerance=ptol, function_tolerance=ftol))
        if mode == DEVICE_APPLIED and t["accept"]:          # already applied on the device: no host test can undo it
            kind, change = 1, x_cost - t["cand_cost"]
            rho = change / t["model_change"]
        elif mode != HOST and kind in (1, 2):               # the device's verdict in place of rho > 1e-3
            kind = 1 if t["accept"] else 2
        before = radius
        if kind == 0:
            invalid += 1
            if invalid >= 5:
                term = 2
            else:
                radius, factor, reuse = radius / factor, factor * 2.0, 0
        elif kind == 1:
            radius, factor, reuse, invalid = min(1e16, radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3)), 2.0, 0, 0
        elif kind == 2:
            radius, factor, reuse, invalid = radius / factor, factor * 2.0, 1, 0
        else:
            term = 0
        rows.append((before, kind, change, rho, radius, factor, reuse, invalid))
        if kind == 1:
            x_cost = t["cand_cost"]
    return rows, term


def bits(rows):
    return [tuple(np.float64(v).tobytes() if isinstance(v, float) else v for v in r) for r in rows]


def both(mode, trials, x_cost, ftol=0.0, ptol=0.0, schedule=None):
    """the hook's rows and termination, equal to the restatement's bit for bit"""
    got, gterm = run_hook(mode, trials, x_cost, ftol, ptol)
    want, wterm = restate(mode, trials, x_cost, ftol, ptol)
    assert gterm == wterm and len(got) == len(want)
    assert bits(got) == bits(want), [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if bits([g]) != bits([w])][:3]
    if schedule if schedule is not None else mode == HOST:
        trace = np.array([[r[0], r[1], r[2], trials[i]["model_change"], r[3], trials[i]["cand_cost"]] for i, r in enumerate(got)])
        ba_bracket.check_schedule(trace)
    return got, gterm


def step_with(x, rho):
    """a trial from cost x whose relative decrease is exactly rho: the candidate halves the cost (rho > 0) or doubles it (rho < 0)"""
    cand = x / 2 if rho > 0 else 2 * x
    change = x - cand
    model = change / rho
    assert change / model == rho and model > 0
    return trial(model, cand)


def chain(x, rhos):
    out = []
    for rho in rhos:
        out.append(step_with(x, rho))
        if rho > 1e-3:
            x = out[-1]["cand_cost"]
    return out


def test_acceptance_threshold_and_radius_update():
    above = math.nextafter(1e-3, 1.0)
    (r,), term = both(HOST, [step_with(8.0, 1e-3)], 8.0)
    assert r[1] == 2 and r[3] == 1e-3 and r[4] == 5e3 and r[5] == 4.0 and r[6] == 1 and term == 1     # rho = 1e-3 exactly: rejected
    (r,), _ = both(HOST, [trial(1.0, above, sn=1.0)], 2 * above)
    assert r[1] == 1 and r[3] == above and r[2] == above
    (r,), _ = both(HOST, [step_with(8.0, 0.5)], 8.0)
    assert r[1] == 1 and r[4] == 1e4 and r[5] == 2.0 and r[6] == 0                                     # rho = 1/2: radius unchanged
    (r,), _ = both(HOST, [step_with(8.0, 1.0)], 8.0)
    assert r[1] == 1 and abs(r[4] / 1e4 - 3.0) < 1e-15                                                 # rho = 1: radius x 3


def test_radius_cap_after_27_accepts():
    x0 = 2.0 ** 40
    rows, term = both(HOST, chain(x0, [1.0] * 27), x0)
    assert len(rows) == 27 and term == 1 and all(r[1] == 1 for r in rows)
    assert rows[-1][4] == 1e16 and rows[-2][4] == 1e16 and rows[19][4] < 1e16
    assert rows[-1][0] == 1e16                                                                         # the cap binds: tried at 1e16 again


def test_rejects_divide_by_2_4_8_16_and_keep_the_diagonal():
    rows, term = both(HOST, chain(8.0, [-1.0] * 4 + [0.5, -1.0]), 8.0)
    assert [r[1] for r in rows] == [2, 2, 2, 2, 1, 2] and term == 1
    assert [r[0] / r[4] for r in rows[:4]] == [2.0, 4.0, 8.0, 16.0]
    assert [r[6] for r in rows] == [1, 1, 1, 1, 0, 1]                                                  # kept across a rejected step only
    assert rows[4][5] == 2.0 and rows[5][0] / rows[5][4] == 2.0                                        # the accept reset the factor
    assert rows[4][2] == 4.0 and rows[5][2] == -4.0                                                    # ... and its candidate became the point


def test_invalid_steps_count_and_fail_at_five():
    bad = trial(1.0, 0.0, valid=0)
    rows, term = both(HOST, [bad] * 4 + [step_with(8.0, 0.5)] + [bad] * 2, 8.0)
    assert [r[1] for r in rows] == [0, 0, 0, 0, 1, 0, 0] and term == 1
    assert [r[7] for r in rows] == [1, 2, 3, 4, 0, 1, 2]                                               # a valid step resets the count
    assert [r[0] / r[4] for r in rows[:4]] == [2.0, 4.0, 8.0, 16.0]
    assert all(r[6] == 0 for r in rows)                                                                # an invalid step rebuilds the diagonal
    assert all(r[2] == 0.0 and r[3] == 0.0 for r in rows if r[1] == 0)
    rows, term = both(HOST, [step_with(8.0, -1.0)] + [bad] * 6, 8.0)
    assert term == 2 and [r[1] for r in rows] == [2, 0, 0, 0, 0, 0] and rows[-1][7] == 5
    assert rows[0][6] == 1 and rows[1][6] == 0                                                         # rejected keeps it, invalid does not
    assert rows[-1][4] == rows[-1][0]                                                                  # the failing step leaves the radius


def test_nan_and_zero_model_change_are_invalid():
    for m in (NAN, 0.0, -1.0):
        (r,), _ = both(HOST, [trial(m, 1.0)], 8.0, schedule=False)
        assert r[1] == 0 and r[7] == 1 and r[4] == 5e3
    for mode in (DEVICE_DECREASE, DEVICE_APPLIED):
        (r,), _ = both(mode, [trial(NAN, 1.0, accept=0)], 8.0)
        assert r[1] == 0


def test_radius_below_1e_minus_32_ends_the_solve():
    rows, term = both(HOST, chain(8.0, [-1.0] * 16), 8.0)
    assert term == 0 and all(r[1] == 2 for r in rows)
    assert rows[-1][4] < 1e-32 <= rows[-1][0] and len(rows) < 16                                       # the head stops before the script ends
    assert rows[-1][4] == 1e4 / 2.0 ** (len(rows) * (len(rows) + 1) // 2)


def test_tolerances_at_equality():
    # sqrt(0.5625) = 0.75 = 0.5 * (sqrt(1) + 0.5)
    rec = trial(1.0, 4.0, sn=0.5625, xn=1.0)
    (r,), term = both(HOST, [rec], 8.0, ptol=0.5)
    assert r[1] == 3 and term == 0 and r[2] == 4.0 and r[3] == 0.0 and r[4] == 1e4 and r[5] == 2.0
    (r,), term = both(HOST, [rec], 8.0, ptol=math.nextafter(0.5, 0.0))
    assert r[1] == 1 and term == 1
    # |4 - 3| = 0.25 * 4
    rec = trial(1.0, 3.0)
    (r,), term = both(HOST, [rec], 4.0, ftol=0.25)
    assert r[1] == 4 and term == 0 and r[2] == 1.0 and r[3] == 0.0
    (r,), term = both(HOST, [rec], 4.0, ftol=math.nextafter(0.25, 0.0))
    assert r[1] == 1 and term == 1
    # the parameter tolerance is tested first
    (r,), _ = both(HOST, [trial(1.0, 3.0, sn=0.5625)], 4.0, ftol=0.25, ptol=0.5)
    assert r[1] == 3
    # a tolerance ends the solve: the rest of the script is not run
    rows, term = both(HOST, [step_with(4.0, 0.5), trial(1.0, 1.5), step_with(2.0, 0.5)], 4.0, ftol=0.25)
    assert [r[1] for r in rows] == [1, 4] and term == 0


def test_who_decides():
    stops = trial(1.0, 4.0, sn=0.5625, xn=1.0, accept=1)          # the host's parameter-tolerance test stops here (ptol 0.5)
    broken = trial(1.0, 4.0, valid=0, accept=1)
    # the device's accept has been applied: it overrides the validity and the tolerance tests
    (r,), term = both(DEVICE_APPLIED, [broken], 8.0)
    assert r[1] == 1 and r[2] == 4.0 and r[3] == 4.0 and term == 1
    (r,), term = both(DEVICE_APPLIED, [stops], 8.0, ptol=0.5)
    assert r[1] == 1 and term == 1
    # ... without it the host's tests run
    (r,), term = both(DEVICE_APPLIED, [dict(stops, accept=0)], 8.0, ptol=0.5)
    assert r[1] == 3 and term == 0
    (r,), _ = both(DEVICE_APPLIED, [dict(broken, accept=0)], 8.0)
    assert r[1] == 0
    # the device decides the relative-decrease test only: the same records stop by tolerance / are invalid
    (r,), term = both(DEVICE_DECREASE, [stops], 8.0, ptol=0.5)
    assert r[1] == 3 and term == 0
    (r,), _ = both(DEVICE_DECREASE, [broken], 8.0)
    assert r[1] == 0
    # ... and where the host would compare rho with 1e-3, the device's word stands either way
    for mode in (DEVICE_DECREASE, DEVICE_APPLIED):
        (r,), _ = both(mode, [dict(step_with(8.0, 0.5), accept=0)], 8.0)
        assert r[1] == 2 and r[3] == 0.5 and r[6] == 1
        (r,), _ = both(mode, [dict(step_with(8.0, 1e-3), accept=1)], 8.0)
        assert r[1] == 1 and r[3] == 1e-3
    # the host ignores the flag
    (r,), _ = both(HOST, [dict(step_with(8.0, 1e-3), accept=1)], 8.0)
    assert r[1] == 2


def test_empty_script_is_the_iteration_limit():
    rows, term = both(HOST, [], 1.0, schedule=False)
    assert rows == [] and term == 1
