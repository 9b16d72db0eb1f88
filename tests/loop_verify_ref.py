"""Sequential float64 statement of the loop verification (include/dvslam_hip.h, "loop verification"; csrc/loop_verify.hip), one function
per stage, for tests/test_gpu_loop_verify.py, and the scenes both test files run on.  Plain numpy and Python integers, no ctypes.  Written
from the rule's DEFINITION, not from the kernels: where the kernel runs cyclic Jacobi sweeps, this file asks numpy.linalg.eigh; where
the kernel folds lane-strided partial sums, this file adds one correspondence after the other.  kabsch() is a second, independent
statement of the fit (SVD with the determinant fix): tests/test_loop_verify_cpu.py measures how far the two are apart, and that distance
— not a number chosen for the kernel — is what the GPU test's bounds are made of."""
import math
import numpy as np

from ransac_stage_ref import sample, replay_select, splitmix64, rodrigues  # noqa: F401  (the sampler and the loop are ransac.hip's)

K4 = (615.0, 615.0, 320.0, 240.0)
GAP_DEGENERATE = 1e-9          # the rule's own threshold on (lambda1 - lambda2) / |lambda1|
GAP_GATE = 1e-3                # hypotheses below it are compared for their flag only: an eigenvector's error scales with 1 / gap
BAND = 1e-9                    # no error may lie within reproj_err^2 (1 +- BAND): then counts and masks are equalities
# Measured by tests/test_loop_verify_cpu.py on the committed scenes (it re-measures and asserts they still hold; EXPERIMENTS.md "Loop
# verification"): the largest |delta (R, t)| x gap between horn() and kabsch() over the gated hypotheses of every GPU case, and the
# largest |delta (R, t)| x gap between them over every refinement set.  The GPU test gives the kernel ten times each, divided by the gap, as
# tests/test_gpu_ransac_stages.py does: the kernel's Jacobi is a third statement with its own stopping rule.
HORN_MEASURED = 3.9e-15
REFINE_MEASURED = 2.3e-15


def default_params(**kw):
    p = dict(iterations=256, min_correspondences=12, min_inliers=12, refine_rounds=2, reproj_err=4.0, confidence=0.99, seed=0, K4=K4)
    p.update(kw)
    return p


def valid(p):
    p = np.asarray(p)
    return np.isfinite(p).all(-1) & (p[..., 2] > 0)


def gather(q_xyz, n, train_row, e_xyz):
    """the correspondence list in ascending query row: (query rows, entry rows)"""
    li, lj = [], []
    for i in range(n):
        j = int(train_row[i])
        if 0 <= j < len(e_xyz) and valid(q_xyz[i]) and valid(e_xyz[j]):
            li.append(i); lj.append(j)
    return np.asarray(li, np.int64), np.asarray(lj, np.int64)


def candidate_seed(seed, entry_id):
    return splitmix64((seed ^ entry_id) & ((1 << 64) - 1))


def _sums(E, Q):
    """centroids, then the centred cross-covariance S[a][b] = sum (e_a - me_a)(q_b - mq_b), one correspondence after the other"""
    n = len(E)
    me = np.zeros(3); mq = np.zeros(3)
    for k in range(n):
        me += E[k]; mq += Q[k]
    me /= n; mq /= n
    S = np.zeros((3, 3))
    for k in range(n):
        S += np.outer(E[k] - me, Q[k] - mq)
    return me, mq, S


def horn(E, Q):
    """Horn's closed form for x_q = R x_e + t: (R, t, gap, ok); gap = (lambda1 - lambda2) / |lambda1| of the 4 x 4 matrix"""
    E = np.asarray(E, np.float64); Q = np.asarray(Q, np.float64)
    me, mq, S = _sums(E, Q)
    (Sxx, Sxy, Sxz), (Syx, Syy, Syz), (Szx, Szy, Szz) = S
    N = np.array([[Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
                  [Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz],
                  [Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy],
                  [Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz]])
    if not np.isfinite(N).all():
        return np.zeros((3, 3)), np.zeros(3), math.nan, False
    w, V = np.linalg.eigh(N)                          # ascending
    l1, l2 = w[3], w[2]
    gap = (l1 - l2) / abs(l1) if l1 != 0 else math.nan
    ok = bool(np.isfinite([l1, l2]).all() and not (l1 - l2) <= GAP_DEGENERATE * abs(l1))
    q = V[:, 3] / np.linalg.norm(V[:, 3])
    if q[0] < 0:
        q = -q
    q0, qx, qy, qz = q
    R = np.array([[q0 * q0 + qx * qx - qy * qy - qz * qz, 2 * (qx * qy - q0 * qz), 2 * (qx * qz + q0 * qy)],
                  [2 * (qx * qy + q0 * qz), q0 * q0 - qx * qx + qy * qy - qz * qz, 2 * (qy * qz - q0 * qx)],
                  [2 * (qx * qz - q0 * qy), 2 * (qy * qz + q0 * qx), q0 * q0 - qx * qx - qy * qy + qz * qz]])
    t = mq - R @ me
    ok = ok and bool(np.isfinite(R).all() and np.isfinite(t).all())
    return R, t, float(gap), ok


def kabsch(E, Q):
    """the same least-squares rotation by SVD of the cross-covariance with the determinant fix: (R, t)"""
    E = np.asarray(E, np.float64); Q = np.asarray(Q, np.float64)
    me, mq = E.mean(0), Q.mean(0)
    U, _, Vt = np.linalg.svd((E - me).T @ (Q - mq))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ D @ U.T
    return R, mq - R @ me


def errors(R, t, K, E, Q):
    """per correspondence: the larger of the two squared reprojection distances; +inf where a transformed depth is <= 0"""
    R = np.asarray(R, np.float64).reshape(3, 3); t = np.asarray(t, np.float64)
    E = np.asarray(E, np.float64); Q = np.asarray(Q, np.float64)
    fx, fy, cx, cy = K
    P = E @ R.T + t                                   # the entry's points in the query's frame
    B = (Q - t) @ R                                   # the query's points in the entry's frame
    ok = (P[:, 2] > 0) & (B[:, 2] > 0)

    def proj(X):
        z = np.where(ok, X[:, 2], 1.0)
        return np.stack([fx * X[:, 0] / z + cx, fy * X[:, 1] / z + cy], 1)
    with np.errstate(all="ignore"):
        d1 = ((proj(P) - proj(Q)) ** 2).sum(1)
        d2 = ((proj(B) - proj(E)) ** 2).sum(1)
        e = np.fmax(d1, d2)
    e = np.where(ok & np.isfinite(e), e, np.inf)
    return e


def in_band(err, thr2):
    """is any error so close to the threshold that a rounding could flip it?"""
    err = np.asarray(err)
    f = err[np.isfinite(err)]
    return bool((np.abs(f - thr2) <= BAND * thr2).any())


def hypothesis(E, Q, seed_c, h):
    """(the 3 list positions, R, t, gap, ok) of hypothesis h"""
    idx = sample(seed_c, h, len(E), 3)
    R, t, gap, ok = horn(E[idx], Q[idx])
    return idx, R, t, gap, ok


def refine_round(R, t, K, thr2, E, Q):
    """one round from the model in hand: Horn on its inliers, the new set; (Rn, tn, gap, ok, |S_new|, accepted, errors of the old model,
    errors of the new)"""
    e_old = errors(R, t, K, E, Q)
    S = e_old <= thr2
    Rn, tn, gap, ok = horn(E[S], Q[S])
    e_new = errors(Rn, tn, K, E, Q) if ok else np.full(len(E), np.inf)
    size = int((e_new <= thr2).sum()) if ok else 0
    return Rn, tn, gap, ok, size, bool(ok and size >= int(S.sum())), e_old, e_new


def verify(q_xyz, n, train_row, e_xyz, entry_id, P, n_entries=None):
    """the whole rule for one candidate, stage by stage: a dict with the record's fields and every intermediate result"""
    thr2 = P["reproj_err"] ** 2
    H = P["iterations"]
    out = dict(n_corr=0, n_inliers=0, success=0, iterations=0, R=np.zeros((3, 3)), rvec=np.zeros(3), tvec=np.zeros(3), rms_px=0.0,
               mask=np.zeros(len(q_xyz), np.uint8), list_i=np.zeros(0, np.int64), n_list=0, hyps=[], counts=[], sel=(-1, 0, 0), rounds=[])
    if n_entries is not None and not 0 <= entry_id < n_entries:
        out["n_corr"] = -1
        return out
    li, lj = gather(q_xyz, n, train_row, e_xyz)
    out["n_corr"] = len(li); out["list_i"] = li; out["list_j"] = lj
    if len(li) < P["min_correspondences"]:
        return out
    out["n_list"] = len(li)
    E = np.asarray(e_xyz, np.float64)[lj]; Q = np.asarray(q_xyz, np.float64)[li]
    out["E"], out["Q"] = E, Q
    seed_c = candidate_seed(P["seed"], entry_id)
    for h in range(H):
        idx, R, t, gap, ok = hypothesis(E, Q, seed_c, h)
        err = errors(R, t, P["K4"], E, Q) if ok else None
        out["hyps"].append(dict(idx=idx, R=R, t=t, gap=gap, ok=ok, err=err))
        out["counts"].append(int((err <= thr2).sum()) if ok else 0)
    best, it, bc, margin = replay_select(out["counts"], len(li), 3, P["confidence"], 1)
    out["sel"] = (best, it, bc); out["select_margin"] = margin
    if best < 0:
        return out
    R, t = out["hyps"][best]["R"], out["hyps"][best]["t"]
    size = bc
    out["rounds"].append(dict(R=R, t=t, size=size, accepted=True, ok=True))
    for _ in range(P["refine_rounds"]):
        Rn, tn, gap, ok, nsize, acc, e_old, e_new = refine_round(R, t, P["K4"], thr2, E, Q)
        out["rounds"].append(dict(R=Rn, t=tn, size=nsize, accepted=acc, ok=ok, gap=gap, e_old=e_old, e_new=e_new))
        if not acc:
            break
        R, t, size = Rn, tn, nsize
    err = errors(R, t, P["K4"], E, Q)
    S = err <= thr2
    out["final_err"] = err
    out["mask"][li[S]] = 1
    out.update(n_inliers=int(S.sum()), success=int(S.sum() >= P["min_inliers"]), iterations=it, R=R, rvec=rodrigues(R), tvec=t,
               rms_px=float(math.sqrt(err[S].mean())))
    return out


# ---------------------------------------------------------------- scenes ----------------------------------------------------------------
def _rot(axis, angle):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * Kx + (1 - math.cos(angle)) * Kx @ Kx


POSE_R = _rot([0.3, 1.0, -0.2], 0.2)                  # about 0.2 rad
POSE_T = np.array([0.25, -0.05, 0.15])                # about 0.3 m
# How well the planted pose can be recovered (asserted by both test files), from the scene's noise alone.  A query point's position noise is
# 0.5 px * z / f across the ray and 0.2 % of z along it; over depths 0.6 .. 6 m (rms 3.65 m) that is 3.0 mm and 7.3 mm.  The depth noise
# dominates; it turns the set about the two image axes with a lever arm of the lateral spread (about 1.2 m rms), so over N inliers the
# rotation's standard deviation is about 7.3e-3 / (1.2 sqrt(N)): 4.5e-4 rad for the 179 inliers of the smallest case.  The translation
# moves with the centroid's noise (7.3e-3 / sqrt(N) = 5.5e-4 m) and with the rotation's error times the centroid's distance (3.5 m x
# 4.5e-4 = 1.6e-3 m).  Five standard deviations: 2.5e-3 rad and 1e-2 m.
POSE_TOL_RAD, POSE_TOL_M = 2.5e-3, 1e-2
N_GOOD = 600                                          # query rows with a valid point
INVALID = [(np.nan, 0.1, 2.0), (0.3, -0.2, 0.0), (0.1, 0.1, -1.5), (np.inf, 0.0, 2.0), (0.2, -np.inf, 3.0), (0.1, 0.2, np.nan)]
N_PAD = 40                                            # rows behind the query's count


def _backproject(uv, z):
    return np.stack([(uv[:, 0] - K4[2]) * z / K4[0], (uv[:, 1] - K4[3]) * z / K4[1], z], 1)


def make_query(seed=11, pixel_noise=0.5, depth_noise=0.002):
    """One query keyframe.  Entry-frame points from pixels at depths 0.6 .. 6 m through K4; the query sees them under (POSE_R, POSE_T) with
    pixel noise and relative depth noise, stored as float32.  Rows: N_GOOD good ones with one point without depth planted after every 100th
    (NaN, z = 0, z < 0, +-inf), then N_PAD rows BEHIND the count n that hold exact transforms — perfect inliers if a kernel looked at them.
    Returns a dict: q_xyz float32 [stride][3], n, stride, good (query rows of the good points), planted (rows without depth), x_e (float64
    entry-frame point of every row), pad (the rows behind n)."""
    rng = np.random.default_rng(seed)
    total = N_GOOD + len(INVALID) + N_PAD
    uv = np.stack([rng.uniform(20, 620, total), rng.uniform(20, 460, total)], 1)
    z = rng.uniform(0.6, 6.0, total)
    x_e = _backproject(uv, z)
    x_q = x_e @ POSE_R.T + POSE_T
    uvq = np.stack([K4[0] * x_q[:, 0] / x_q[:, 2] + K4[2], K4[1] * x_q[:, 1] / x_q[:, 2] + K4[3]], 1)
    noisy = _backproject(uvq + rng.normal(0, pixel_noise, uvq.shape), x_q[:, 2] * (1 + rng.normal(0, depth_noise, total)))
    n = N_GOOD + len(INVALID)
    q = np.zeros((total, 3), np.float64)
    planted = [100 * (k + 1) + k for k in range(len(INVALID))]          # rows 100, 201, 302, ...
    good = [i for i in range(n) if i not in planted]
    q[good] = noisy[good]
    for k, i in enumerate(planted):
        q[i] = INVALID[k]
    pad = list(range(n, total))
    q[pad] = x_q[pad]
    return dict(q_xyz=q.astype(np.float32), n=n, stride=total, good=good, planted=planted, pad=pad, x_e=x_e, seed=seed)


def make_entry(query, m, seed, outliers=0.3):
    """One entry keyframe of `rows` rows and its train_idx row [stride]: m valid correspondences (query rows drawn from the good ones, entry
    rows in shuffled order; a share `outliers` of them permuted among themselves), then: every planted query row matched to a VALID entry
    point (the query side alone rules it out), len(INVALID) good query rows matched to entry points without depth (the entry side alone
    rules them out), the pad rows matched to their exact partners, two rows matched past the entry's last row and every other row
    unmatched.  Returns dict: e_xyz float32 [rows][3], train int32 [stride], m, inlier_rows (query rows of the unpermuted matches)."""
    rng = np.random.default_rng(seed)
    good = list(query["good"])
    pick = sorted(rng.choice(len(good), m, replace=False).tolist()) if m else []
    qrows = [good[k] for k in pick]
    rest = [g for g in good if g not in set(qrows)]
    side = rest[:len(INVALID)] if len(rest) >= len(INVALID) + 2 else []           # good query rows whose entry partner has no depth
    past = rest[len(INVALID):len(INVALID) + 2] if side else []
    rows = m + len(query["planted"]) + len(side) + len(query["pad"]) + 7
    order = rng.permutation(rows).tolist()
    e = np.zeros((rows, 3), np.float64)
    e[:] = (0.5, 0.5, 2.0)                                                      # fillers: valid, matched by nobody
    train = np.full(query["stride"], -1, np.int32)
    slot = iter(order)
    partner = {}
    for i in qrows + query["planted"] + query["pad"]:
        j = next(slot); partner[i] = j
        e[j] = query["x_e"][i]; train[i] = j
    for k, i in enumerate(side):
        j = next(slot)
        e[j] = INVALID[k]; train[i] = j
    for i in past:
        train[i] = rows + 3
    n_out = int(round(outliers * m)) if m >= 10 else 0
    out_rows = sorted(rng.choice(m, n_out, replace=False).tolist()) if n_out else []
    if n_out:                                                                   # a cyclic shift of the chosen matches' partners
        js = [partner[qrows[k]] for k in out_rows]
        for k, j in zip(out_rows, js[1:] + js[:1]):
            train[qrows[k]] = j
    inl = [qrows[k] for k in range(m) if k not in set(out_rows)]
    return dict(e_xyz=e.astype(np.float32), train=train, m=m, rows=rows, inlier_rows=inl, jrows=[partner[i] for i in qrows])


# the entries of the one database both test files use, in id order: (name, m, outlier share)
ENTRIES = [("m600", 600, 0.3), ("m257", 257, 0.3), ("m256", 256, 0.3), ("m255", 255, 0.3), ("m4", 4, 0.0), ("m3", 3, 0.0), ("m2", 2, 0.0),
           ("m0", 0, 0.0), ("nopoints", 300, 0.3), ("refused", 60, 0.3), ("dup", 20, 0.0)]
ENTRY_ID = {name: k for k, (name, _, _) in enumerate(ENTRIES)}
SAMPLER_SEED = 11
H_CASE = 200
# the single-candidate cases: (entry name, parameters)
CASES = [("m3", dict(iterations=16, min_correspondences=3, min_inliers=3)), ("m4", dict(iterations=16, min_correspondences=3, min_inliers=3)),
         ("m255", dict(iterations=H_CASE)), ("m256", dict(iterations=H_CASE)), ("m257", dict(iterations=H_CASE)), ("m600", dict(iterations=H_CASE)),
         ("refused", dict(iterations=64, refine_rounds=4)), ("dup", dict(iterations=64))]
RAGGED = ["m257", "m2", "m0", "m600", None, "nopoints", "m257"]     # None: an id out of range
N_DUP = 8                      # of the "dup" entry's 20 partners this many hold the SAME point: a sample with two of them is degenerate
GAP_FLAG_BAND = (0.5e-9, 2e-9)  # a gap inside it may be flagged either way; the scenes have none there (asserted on the CPU)
REFUSED_QUERY_NOISE = 2.5      # px: the "refused" entry is matched against a query of its own with this much pixel noise (see make_scene)


_scene = None


def make_scene():
    """(query, entries {name: entry}, refused_query): everything the two test files run on, built once.  The `refused` entry goes with a
    query of its own whose pixel noise is REFUSED_QUERY_NOISE: with noise of the order of the threshold a refit on the inliers of a minimal
    sample can lose some of them, which is the case the rule's "accept iff |S_r| >= |S_(r-1)|" exists for."""
    global _scene
    if _scene is None:
        query = make_query()
        rq = make_query(seed=REFUSED_SEED, pixel_noise=REFUSED_QUERY_NOISE, depth_noise=0.01)
        entries = {}
        for k, (name, m, share) in enumerate(ENTRIES):
            entries[name] = make_entry(rq if name == "refused" else query, m, 1000 + k, share)
        d = entries["dup"]
        d["e_xyz"][d["jrows"][1:N_DUP]] = d["e_xyz"][d["jrows"][0]]
        _scene = (query, entries, rq)
    return _scene


REFUSED_SEED = 14


def case_params(over):
    return default_params(seed=SAMPLER_SEED, **over)


def standard_points(entries, query, train1):
    """points for the standard scene of tests/loop_ref.py (descriptor frames `entries` and `query`): entry 1 and the query see the same
    points under the planted pose wherever the guided match (train1 = the query's train_idx row against entry 1) pairs them, everything
    else is unrelated; query row 3 has no depth.  ([float32 [rows][3] per entry], float32 [n][3])"""
    rng = np.random.default_rng(5)

    def cloud(k):
        uv = np.stack([rng.uniform(20, 620, k), rng.uniform(20, 460, k)], 1)
        return _backproject(uv, rng.uniform(0.6, 6.0, k))
    pts = [cloud(len(e)).astype(np.float32) for e in entries]
    qp = cloud(len(query))
    for i, j in enumerate(train1):
        if j >= 0:
            qp[i] = pts[1][j].astype(np.float64) @ POSE_R.T + POSE_T
    qp[3] = np.nan
    return pts, qp.astype(np.float32)
