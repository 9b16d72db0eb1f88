"""The assertions on ONE trial step that the step tests of the two device solvers share (tests/test_gpu_ba_steps.py:
dvs_ba_solve_device; tests/test_gpu_ba_global_steps.py: dvs_ba_solve_global), each on a probe `o` (the dict a step hook returns)
against a reference `s` (ba_step_ref.Step, built from o's scale and diag with the solver's own active set), and the loop around a
step hook that replays a solve.  The bounds are derived in tests/test_gpu_ba_steps.py's docstring.  Every check writes the distance
it measured into `dist`, in units of its bound where it has one."""
import numpy as np
import ba_step_ref as bs

EPS = bs.EPS
LD = bs.LD
FTOL, PTOL, GTOL = 1e-6, 1e-8, 1e-10


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def at(P, q, t, X):
    """the problem P at another point"""
    Q = dict(P); Q["q"], Q["t"], Q["X"] = (np.ascontiguousarray(a) for a in (q, t, X))
    return Q


def cost_of(P):
    """-> f(q, t, X): a fresh handle's evaluate() cost at that point"""
    from dvslam_amd import BAProblem

    def f(q, t, X):
        return BAProblem(at(P, q, t, X)).evaluate()[0]
    return f


def check_scale_and_diag(B, o, scale_from=None):
    hpp, hll = B[0], B[1]
    if scale_from is None:
        want = bs.jacobi_scale(hpp, hll)
        assert (np.abs(o["scale"] - want) <= 1e-11 * want).all()
    else:
        assert (bits(o["scale"]) == bits(scale_from)).all(), "the scaling is fixed at the first Jacobian"
    want = bs.lm_diagonal(hpp, hll, o["scale"])
    assert (np.abs(o["diag"] - want) <= 1e-11 * want).all()
    assert (o["diag"] >= 1e-6).all() and (o["diag"] <= 1e32).all()


def check_vinv(tag, s, o, lb, dist):
    """the per-landmark inverses by their residual; lb: s.landmark_blocks() or s.reduced()"""
    la = s.la
    assert not o["Vinv"][~la].any()
    V = lb["V"][la]
    tau, G = bs.inv3_rounding(V)
    Rm = np.abs(np.einsum("lab,lbc->lac", V, o["Vinv"][la].astype(LD)) - np.eye(3))
    lim = 16 * EPS * (np.einsum("lab,lbc->lac", np.abs(V), G) + tau[:, None, None] * np.eye(3))
    worst = int((Rm / lim).max(axis=(1, 2)).argmax())
    dist["Vinv"] = float((Rm / lim).max())
    cond = np.linalg.cond(V.astype(np.float64))
    assert (Rm <= lim).all(), f"{tag}: |V Vinv - I| = {float(Rm[worst].max()):.2e} at cond(V) = {cond[worst]:.2e}"


def check_step_residual(tag, s, o, rho, dist):
    """inactive rows exactly zero, every entry finite, the full-system residual within rho"""
    step = o["step"]
    assert not step[~s.act].any(), "rows of inactive blocks are exactly zero"
    assert np.isfinite(step).all()
    dist["step"] = s.residual(step)
    assert dist["step"] <= rho, f"{tag}: full-system residual {dist['step']:.2e} > {rho:.1e}"


def check_landmark_rows(tag, s, o, lb, dist):
    """the landmark rows alone, from the device's own camera rows and its own Vinv"""
    K, L = s.K, s.L
    dl, mag = s.landmark_part(o["step"], lb, Vinv=o["Vinv"])
    el = np.abs(dl - o["step"][6 * K:].reshape(L, 3))
    dist["landmark part"] = float((el[s.la] / mag[s.la]).max())
    assert (el <= 1e-11 * mag).all(), f"{tag}: landmark rows off by {dist['landmark part']:.2e} of their absolute terms"


def check_model_change(tag, s, o, dist):
    """against the reference formula on the device's own step -> the sum of the absolute values of the formula's terms"""
    mc, mmag = s.model_change(o["step"])
    dist["model change"] = float(abs(o["model_change"] - mc) / mmag)
    assert dist["model change"] <= 1e-11, f"{tag}: model change {o['model_change']!r}, reference formula on the device's step {float(mc)!r}"
    return mmag


def check_candidate(tag, s, o, dist):
    K, L = s.K, s.L
    la = s.la
    step = o["step"]
    dc = step[:6 * K].reshape(K, 6); dX = step[6 * K:].reshape(L, 3)
    want_q = bs.quat_plus(s.q.astype(LD), dc[:, :3].astype(LD))
    nd = np.sqrt((dc[:, :3] ** 2).sum(1))
    qlim = (8 + 2 * nd)[:, None] * EPS * bs.quat_plus_magnitude(s.q, dc[:, :3])
    eq = np.abs(o["q"] - want_q)[s.ca]
    dist["candidate q (ulp of its terms)"] = float((eq / (EPS * bs.quat_plus_magnitude(s.q, dc[:, :3])[s.ca])).max())
    assert (eq <= qlim[s.ca]).all(), f"{tag}: candidate quaternion {dist['candidate q (ulp of its terms)']:.1f} ulp off"
    assert (bits(o["t"][s.ca]) == bits(s.t[s.ca] + dc[s.ca, 3:])).all()
    assert (bits(o["X"][la]) == bits(s.X[la] + dX[la])).all()
    assert (bits(o["q"][~s.ca]) == bits(s.q[~s.ca])).all() and (bits(o["t"][~s.ca]) == bits(s.t[~s.ca])).all()
    assert (bits(o["X"][~la]) == bits(s.X[~la])).all()


def check_record(tag, s, o, B, cost_fn, dist):
    """norms, costs, gradient norm and the verdict"""
    K = s.K
    sn, xn = s.norms(o["q"], o["t"], o["X"])
    dist["sn"], dist["xn"] = float(abs(o["sn"] - sn) / sn), float(abs(o["xn"] - xn) / xn)
    assert dist["sn"] <= 1e-13 and dist["xn"] <= 1e-13
    cc = cost_fn(o["q"], o["t"], o["X"])
    dist["cand_cost"] = abs(o["cand_cost"] - cc) / cc
    assert dist["cand_cost"] <= 1e-12
    assert bits(o["x_cost"]) == bits(B[4])
    g = s.g[:6 * K].reshape(K, 6)
    glim = ((8 + 2 * np.sqrt((g[:, :3] ** 2).sum(1)))[:, None] * EPS * bs.quat_plus_magnitude(s.q, -g[:, :3]))[s.ca].max()
    dist["gmax (of its bound)"] = float(abs(o["gmax"] - s.gmax()) / glim) if glim > 0 else 0.0
    assert abs(o["gmax"] - s.gmax()) <= glim, (o["gmax"], s.gmax())
    assert o["accept"] == bs.accept_rule(o, FTOL, PTOL)


def report(tag, dist, o):
    print(f"{tag}: " + "  ".join(f"{k} {v:.2e}" for k, v in dist.items()) + f"  accept {o['accept']}")


def replay(probe, P, iters):
    """a device solver's loop around its step hook, with the trust-region schedule tests/ba_bracket.py states.
    probe(radius, refresh, commit) -> the hook's dict.  -> (trace rows, q, t, X, the probes)"""
    radius, factor, reuse = 1e4, 2.0, False
    q, t, X = P["q"], P["t"], P["X"]
    rows, probes = [], []
    invalid = 0
    for _ in range(iters):
        o = probe(radius, not reuse, True)
        probes.append(o)
        assert o["gmax"] > GTOL and radius >= 1e-32, "the replay does not model the gradient-tolerance exit"
        valid = o["ok"] and o["finite"] and o["model_change"] > 0.0
        if not valid and not o["accept"]:
            rows.append([radius, 0, 0, o["model_change"], 0, 0])
            invalid += 1
            if invalid >= 5:
                break
            radius /= factor; factor *= 2; reuse = False
            continue
        cc = o["x_cost"] - o["cand_cost"]
        if not o["accept"]:
            if np.sqrt(o["sn"]) <= PTOL * (np.sqrt(o["xn"]) + PTOL):
                rows.append([radius, 3, cc, o["model_change"], 0, o["cand_cost"]]); break
            if abs(cc) <= FTOL * o["x_cost"]:
                rows.append([radius, 4, cc, o["model_change"], 0, o["cand_cost"]]); break
        rel = cc / o["model_change"]
        rows.append([radius, 1 if o["accept"] else 2, cc, o["model_change"], rel, o["cand_cost"]])
        invalid = 0
        if o["accept"]:
            q, t, X = o["q"], o["t"], o["X"]
            radius = min(1e16, radius / max(1.0 / 3.0, 1.0 - (2.0 * rel - 1.0) ** 3))
            factor, reuse = 2.0, False
        else:
            radius /= factor; factor *= 2; reuse = True
    return np.array(rows), q, t, X, probes
