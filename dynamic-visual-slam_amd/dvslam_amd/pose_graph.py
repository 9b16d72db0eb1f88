import ctypes as C
import numpy as np
from ._lib import lib, test_lib, check, ptr, PgoParams, PgoSummary, PgoStepRecord


class PoseGraph:
    """Driver of the dvs_pgo_* C-ABI (include/dvslam_hip.h "Pose-graph optimisation"): nodes (R, t, fixed), edges (i, j, rvec, tvec, w_rot,
    w_trans) with x_i = R_z x_j + t_z, a Levenberg-Marquardt solve on the device, and the map correction.  hooks=True makes every call
    through lib/libdvslam_hip_test.so, which also has the operator, linear-solve and trial-step hooks (apply, pcg, trial_step)."""

    def __init__(self, device=0, hooks=False):
        self._L = test_lib() if hooks else lib()
        h = C.c_void_p()
        check(self._L.dvs_pgo_create(device, C.byref(h)))
        self._h = h
        self.N = self.E = 0

    def close(self):
        if getattr(self, "_h", None):
            self._L.dvs_pgo_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_nodes(self, R, t, fixed):
        R = np.ascontiguousarray(R, np.float64).reshape(-1, 9); t = np.ascontiguousarray(t, np.float64).reshape(-1, 3)
        fixed = np.ascontiguousarray(fixed, np.uint8)
        assert len(R) == len(t) == len(fixed)
        check(self._L.dvs_pgo_set_nodes(self._h, len(R), ptr(R), ptr(t), ptr(fixed)))
        if len(R) != self.N:
            self.E = 0
        self.N = len(R)
        return self

    def set_edges(self, i, j, rvec, tvec, w_rot, w_trans):
        i = np.ascontiguousarray(i, np.int32); j = np.ascontiguousarray(j, np.int32)
        rvec = np.ascontiguousarray(rvec, np.float64).reshape(-1, 3); tvec = np.ascontiguousarray(tvec, np.float64).reshape(-1, 3)
        w_rot = np.ascontiguousarray(w_rot, np.float64); w_trans = np.ascontiguousarray(w_trans, np.float64)
        assert len(i) == len(j) == len(rvec) == len(tvec) == len(w_rot) == len(w_trans)
        check(self._L.dvs_pgo_set_edges(self._h, len(i), ptr(i), ptr(j), ptr(rvec), ptr(tvec), ptr(w_rot), ptr(w_trans)))
        self.E = len(i)
        return self

    def evaluate(self):
        """(cost, residuals [E][6], Ji [E][6][6], Jj [E][6][6], grad [6 N]) at the current poses"""
        cost = C.c_double(); r = np.zeros((self.E, 6)); A = np.zeros((self.E, 6, 6)); B = np.zeros((self.E, 6, 6)); g = np.zeros(6 * self.N)
        check(self._L.dvs_pgo_evaluate(self._h, C.byref(cost), ptr(r), ptr(A), ptr(B), ptr(g)))
        return cost.value, r, A, B, g

    def solve(self, **params):
        """dvs_pgo_solve with the defaults of dvs_pgo_default_params overridden by keyword; returns the dvs_pgo_summary"""
        p = PgoParams()
        check(self._L.dvs_pgo_default_params(C.byref(p)))
        for k, v in params.items():
            if k not in dict(PgoParams._fields_):
                raise TypeError(f"unknown parameter {k}")
            setattr(p, k, v)
        s = PgoSummary()
        check(self._L.dvs_pgo_solve(self._h, C.byref(p), C.byref(s)))
        return s

    def nodes(self):
        R = np.zeros((self.N, 3, 3)); t = np.zeros((self.N, 3))
        check(self._L.dvs_pgo_get_nodes(self._h, ptr(R), ptr(t)))
        return R, t

    def trace(self):
        """[trial steps, 7]: radius, kind (0 invalid, 1 accepted, 2 rejected, 3 ptol, 4 ftol), cost change, model cost change, relative
        decrease, candidate cost, PCG iterations"""
        n = C.c_int32()
        check(self._L.dvs_pgo_get_trace(self._h, None, 0, C.byref(n)))
        rows = np.zeros((n.value, 7))
        check(self._L.dvs_pgo_get_trace(self._h, ptr(rows), n.value, C.byref(n)))
        return rows

    def correct_points(self, xyz, anchor, n=None):
        """the first n rows (all by default) of a float32 [.][3] array moved with their anchor keyframes; returns a new array"""
        out = np.array(xyz, np.float32, order="C").reshape(-1, 3)
        anchor = np.ascontiguousarray(anchor, np.int32)
        n = len(out) if n is None else int(n)
        assert n <= len(out) and n <= len(anchor)
        check(self._L.dvs_pgo_correct_points(self._h, n, ptr(out), ptr(anchor)))
        return out

    def correct_points_device(self, n, d_xyz, d_anchor):
        check(self._L.dvs_pgo_correct_points_device(self._h, int(n), d_xyz, d_anchor))

    def synchronize(self):
        check(self._L.dvs_pgo_synchronize(self._h))

    # the hooks of include/dvslam_hip_test_pgo.h (hooks=True)
    def apply(self, radius, p):
        p = np.ascontiguousarray(p, np.float64); y = np.zeros(6 * self.N)
        assert p.size == 6 * self.N
        check(self._L.dvs_test_pgo_apply(self._h, float(radius), ptr(p), ptr(y)))
        return y

    def pcg(self, radius, eta, max_it):
        """(x, iterations, |r|, |g|)"""
        x = np.zeros(6 * self.N); it = C.c_int32(); rn = C.c_double(); gn = C.c_double()
        check(self._L.dvs_test_pgo_pcg(self._h, float(radius), float(eta), int(max_it), ptr(x), C.byref(it), C.byref(rn), C.byref(gn)))
        return x, it.value, rn.value, gn.value

    def trial_step(self, radius, eta=0.1, max_pcg_iterations=0, reuse_diagonal=False, commit=False, x_in=None):
        """ONE trial step of the solve (dvs_test_pgo_trial_step): a dict of the point it was taken from (q, t), the step x, the LM diagonal D,
        the candidate (cand_q, cand_t) and the fields of the status record.  x_in: a step to take in place of the linear solve's."""
        N = self.N
        if x_in is not None:
            x_in = np.ascontiguousarray(x_in, np.float64)
            assert x_in.size == 6 * N
        o = dict(q=np.zeros((N, 4)), t=np.zeros((N, 3)), x=np.zeros(6 * N), D=np.zeros(6 * N), cand_q=np.zeros((N, 4)), cand_t=np.zeros((N, 3)))
        rec = PgoStepRecord()
        check(self._L.dvs_test_pgo_trial_step(self._h, float(radius), float(eta), int(max_pcg_iterations), int(bool(reuse_diagonal)), int(bool(commit)),
                                              ptr(x_in) if x_in is not None else None, ptr(o["q"]), ptr(o["t"]), ptr(o["x"]), ptr(o["D"]),
                                              ptr(o["cand_q"]), ptr(o["cand_t"]), C.byref(rec)))
        o.update({k: getattr(rec, k) for k, _ in PgoStepRecord._fields_ if k != "reserved"})
        return o
