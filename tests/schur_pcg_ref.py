"""Dense float64 numpy restatement of the linear solve of dvs_ba_solve_global (include/dvslam_hip.h, "Global BA"): Jacobi scaling
1 / (1 + sqrt(H_jj)), D = clamp(diag, 1e-6, 1e32), the reduced camera system S and its right-hand side b at a trust-region radius, the
block-Jacobi preconditioner (6 x 6 blocks, Cholesky, the diagonal's inverse if a pivot is not positive), and the PCG iteration with its
stopping rule.  Everything is formed densely: S is 6K x 6K with zero rows and columns for fixed cameras.  Inputs are the Gauss-Newton
blocks as OracleBA.normal_equations() / BAProblem.normal_equations() return them (H_pp [K,6,6], H_ll [L,3,3], W [R,6,3] in the
caller's observation order, g [6K + 3L]), or blocks_from_jacobians() of an evaluate()."""
import numpy as np


def default_cap(nc):
    """max_pcg_iterations = 0"""
    return max(100, 12 * nc)


def blocks_from_jacobians(P, r, jp, jl):
    """H_pp, H_ll, W, g from loss-corrected residuals [R,2] and Jacobians [R,2,6], [R,2,3] (tests/test_gpu_ba_window.py forms its
    reduced system from the same arrays)"""
    K, L = int(P["K"]), int(P["L"])
    cam = np.asarray(P["cam_idx"], np.int64); lm = np.asarray(P["lm_idx"], np.int64)
    hpp = np.zeros((K, 6, 6)); hll = np.zeros((L, 3, 3)); g = np.zeros(6 * K + 3 * L)
    np.add.at(hpp, cam, np.einsum("eka,ekb->eab", jp, jp))
    np.add.at(hll, lm, np.einsum("eka,ekb->eab", jl, jl))
    w = np.einsum("eka,ekb->eab", jp, jl)
    gp = np.einsum("eka,ek->ea", jp, r); gl = np.einsum("eka,ek->ea", jl, r)
    np.add.at(g[:6 * K].reshape(K, 6), cam, gp)
    np.add.at(g[6 * K:].reshape(L, 3), lm, gl)
    return hpp, hll, w, g


class SchurSystem:
    """S, b, M^-1 at one radius, and the un-cancelled magnitudes (|A| + |B| |C^-1| |B^T|) the operator's forward-error bound uses"""

    def __init__(self, P, hpp, hll, w, g, radius):
        K, L = int(P["K"]), int(P["L"])
        cam = np.asarray(P["cam_idx"], np.int64); lm = np.asarray(P["lm_idx"], np.int64)
        pf = np.asarray(P["pose_fixed"]).astype(bool); lf = np.asarray(P["lm_fixed"]).astype(bool)
        free = ~pf
        used = np.zeros(L, bool); used[lm] = True
        act = ~lf & used
        self.K, self.L, self.free, self.act, self.nc = K, L, free, act, int(free.sum())
        self.cam, self.lm = cam, lm
        sp = 1.0 / (1.0 + np.sqrt(np.einsum("caa->ca", hpp)))            # [K, 6]
        sl = 1.0 / (1.0 + np.sqrt(np.einsum("laa->la", hll)))            # [L, 3]
        U = hpp * sp[:, :, None] * sp[:, None, :]
        V = hll * sl[:, :, None] * sl[:, None, :]
        Dp = np.clip(np.einsum("caa->ca", U), 1e-6, 1e32); Dl = np.clip(np.einsum("laa->la", V), 1e-6, 1e32)
        U = U + np.einsum("ca,ab->cab", Dp / radius, np.eye(6))
        V = V + np.einsum("la,ab->lab", Dl / radius, np.eye(3))
        Vinv = np.zeros((L, 3, 3)); Vinv[act] = np.linalg.inv(V[act])
        on = free[cam] & act[lm]                                          # the observations that couple a free camera to an active landmark
        Ws = w * sp[cam][:, :, None] * sl[lm][:, None, :] * on[:, None, None]
        Wd = np.zeros((6 * K, 3 * L)); Wa = np.zeros((6 * K, 3 * L))
        for e in np.nonzero(on)[0]:
            c, l = cam[e], lm[e]
            Wd[6 * c:6 * c + 6, 3 * l:3 * l + 3] += Ws[e]; Wa[6 * c:6 * c + 6, 3 * l:3 * l + 3] += np.abs(Ws[e])
        Ud = np.zeros((6 * K, 6 * K)); Vd = np.zeros((3 * L, 3 * L))
        for c in np.nonzero(free)[0]:
            Ud[6 * c:6 * c + 6, 6 * c:6 * c + 6] = U[c]
        for l in np.nonzero(act)[0]:
            Vd[3 * l:3 * l + 3, 3 * l:3 * l + 3] = Vinv[l]
        gp = (g[:6 * K].reshape(K, 6) * sp * free[:, None]).reshape(-1)
        gl = (g[6 * K:].reshape(L, 3) * sl * act[:, None]).reshape(-1)
        self.sp, self.sl, self.Vinv, self.Ws, self.gl = sp, sl, Vinv, Ws, gl.reshape(L, 3)
        self.S = Ud - Wd @ Vd @ Wd.T
        self.b = gp - Wd @ Vd @ gl
        self.Smag = np.abs(Ud) + Wa @ np.abs(Vd) @ Wa.T
        self.bmag = np.abs(gp) + Wa @ np.abs(Vd) @ np.abs(gl)
        # preconditioner: M_c = U_c - sum_{e of c} Y_e Ws_e^T, observation by observation (a landmark seen twice in a camera is two terms)
        Y = np.einsum("eab,ebc->eac", Ws, Vinv[lm])
        M = U.copy(); Mmag = np.abs(U)
        np.subtract.at(M, cam, np.einsum("eab,ecb->eac", Y, Ws))
        np.add.at(Mmag, cam, np.einsum("eab,ecb->eac", np.abs(Y), np.abs(Ws)))
        self.M = M * free[:, None, None]; self.Mmag = Mmag * free[:, None, None]
        self.Minv = np.zeros((K, 6, 6))
        for c in np.nonzero(free)[0]:
            try:
                Lc = np.linalg.cholesky(M[c])
                Li = np.linalg.inv(Lc)
                self.Minv[c] = Li.T @ Li
            except np.linalg.LinAlgError:
                self.Minv[c] = np.diag(1.0 / np.diag(M[c]))

    def precond(self, r):
        return np.einsum("cab,cb->ca", self.Minv, r.reshape(self.K, 6)).reshape(-1)

    def back_substitute(self, x):
        """the whole step that follows from the camera rows x of S x = b, plain float64: delta_c = -x,
        delta_l = -Vinv_l (g_l + sum_e Ws_e^T delta_cam(e)), scaled back -> [6K + 3L] in parameter units"""
        dc = -np.asarray(x).reshape(self.K, 6)
        tl = self.gl.copy()
        np.add.at(tl, self.lm, np.einsum("eab,ea->eb", self.Ws, dc[self.cam]))
        dl = -np.einsum("lab,lb->la", self.Vinv, tl)
        return np.concatenate([(dc * self.sp).reshape(-1), (dl * self.sl).reshape(-1)])

    def pcg(self, eta, max_it=0):
        """-> x, iterations, |r| / |b| of the recurrence, ok (0: stopped by breakdown before the first iteration).  |b| = 0: x = 0
        solves the system, zero iterations, ok"""
        cap = max_it if max_it > 0 else default_cap(self.nc)
        b = self.b
        x = np.zeros_like(b); r = b.copy(); z = self.precond(r); p = z.copy()
        rz = r @ z; bn = np.sqrt(b @ b)
        k = 0
        if bn == 0:
            return x, 0, 0.0, 1
        while True:
            q = self.S @ p
            pq = p @ q
            if not (pq > 0) or not np.isfinite(pq):
                return x, k, (np.sqrt(r @ r) / bn if bn > 0 else 0.0), int(k > 0)
            alpha = rz / pq
            x = x + alpha * p; r = r - alpha * q
            z = self.precond(r)
            rzn = r @ z
            k += 1
            if np.sqrt(r @ r) <= eta * bn or k >= cap:
                return x, k, np.sqrt(r @ r) / bn, 1
            p = z + (rzn / rz) * p
            rz = rzn


# the four systems of the tests (include/dvslam_hip.h "Global BA"):
# (a) 95 free cameras (> 64), 162..313 observations per camera (two chunks), 13..25 per landmark (crosses k_lm_backsub's 16)
# (b) 25..45 observations per camera, 5..9 per landmark   (c) the full 20 x 200 window   (d) (c) with large noise
# They do NOT reach every branch of the kernels: at most 96 cameras (the loops that stride the cameras by 256 take one trip), every K
# a multiple of 4 (k_gba_precond's last workgroup is full), no camera with exactly 63, 64, 65, 256 or 257 observations or with three
# chunks.  Those shapes are tests/gba_step_ref.py's "259 cameras" and "chunk edges" (tests/test_gpu_ba_global_steps.py).
LARGE_NOISE = dict(pose_noise=(0.2, np.deg2rad(8)), lm_noise=0.3, outlier_frac=0.1)


def system_problem(name):
    from dvslam_amd import synth
    if name == "a":
        return synth.make_ba_banded_problem(K=96, L=1200, seed=96, half_span=12)
    if name == "b":
        return synth.make_ba_banded_problem(K=80, L=400, seed=80, half_span=4)
    if name == "c":
        return synth.make_ba_problem(K=20, L=200, seed=3)
    if name == "d":
        return synth.make_ba_problem(K=20, L=200, seed=3, **LARGE_NOISE)
    raise KeyError(name)
