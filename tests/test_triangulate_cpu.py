"""CPU: the numpy restatement of LandmarkInfo::triangulate (tests/triangulate_ref.py) against independent statements — numpy's SVD
null vector, ground truth on noise-free scenes — and one scene per status.  The GPU tests compare the kernel with it bit for bit."""
import numpy as np
import pytest
import triangulate_ref as tr


def _independent_null_vector(R, t, kfs, px, K=tr.K4):
    fx, fy, cx, cy = K
    Km = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    rows = []
    for k, (u, v) in zip(kfs, px.astype(np.float64)):
        P = Km @ np.hstack([R[k].reshape(3, 3), t[k].reshape(3, 1)])
        rows += [u * P[2] - P[0], v * P[2] - P[1]]
    return np.linalg.svd(np.array(rows))[2][-1]


@pytest.mark.parametrize("vmin,vmax", [(2, 2), (3, 12)])
def test_null_vector_matches_numpy_svd(vmin, vmax):
    rng = np.random.default_rng(5 + vmin)
    R, t, _ = tr.keyframes(rng, 20)
    offs, vkf, vpx, xyz, _ = tr.random_landmarks(rng, R, t, 200, vmin, vmax, noise=0.5)
    out, st, info = tr.triangulate(R, t, *tr.K4, offs, vkf, vpx, xyz, details=True)
    assert (np.abs(info["max_angle"] - tr.MIN_PARALLAX) > 1e-6).all()
    checked = 0
    for l in range(len(offs) - 1):
        if st[l] == tr.LOW_PARALLAX:
            continue
        x = info["x"][l]
        y = _independent_null_vector(R, t, vkf[offs[l]:offs[l + 1]], vpx[offs[l]:offs[l + 1]])
        a, b = x[:3] / x[3], y[:3] / y[3]
        assert np.linalg.norm(a - b) <= 1e-9 * np.linalg.norm(b), (l, a, b)
        checked += 1
    assert checked > 150


def test_noise_free_scenes_recover_ground_truth():
    rng = np.random.default_rng(17)
    R, t, _ = tr.keyframes(rng, 12)
    offs, vkf, vpx, xyz, Xt = tr.random_landmarks(rng, R, t, 300, 2, 10, noise=0.0)
    out, st, info = tr.triangulate(R, t, *tr.K4, offs, vkf, vpx, xyz, details=True)
    ok = st == tr.UPDATED
    assert ok.sum() > 250
    X = info["x"][ok, :3] / info["x"][ok, 3:4]
    err = np.linalg.norm(X - Xt[ok], axis=1) / np.linalg.norm(Xt[ok], axis=1)
    assert err.max() <= 1e-6, err.max()
    # the float positions the landmarks take are those points rounded
    assert np.abs(out[ok] - Xt[ok]).max() <= 1e-5 * np.abs(Xt[ok]).max()


def test_each_status_is_reached_by_its_scene():
    R, t, offs, vkf, vpx, xyz, expected = tr.status_scenes()
    out, st, info = tr.triangulate(R, t, *tr.K4, offs, vkf, vpx, xyz, details=True)
    assert st.tolist() == expected
    kept = st != tr.UPDATED
    assert out[kept].tobytes() == xyz[kept].tobytes()
    # landmark 6 lies behind all three cameras that see it: no view counts, so the reprojection check passes (the reference's quirk)
    Y = out[6].astype(np.float64)
    for k in vkf[offs[6]:offs[7]]:
        assert (R[k].reshape(3, 3) @ Y + t[k])[2] < 0
    assert np.abs(out[6] - np.array([0.1, 0.0, 3.0])).max() < 1e-4


def test_sweeps_stay_below_max_iter():
    rng = np.random.default_rng(23)
    R, t, _ = tr.keyframes(rng, 40)
    offs, vkf, vpx, xyz, _ = tr.random_landmarks(rng, R, t, 300, 2, 16, noise=1.0)
    o2, k2, p2, x2, _ = tr.random_landmarks(rng, R, t, 1, 300, 300, noise=1.0)
    offs = np.concatenate([offs, o2[1:] + offs[-1]]); vkf = np.concatenate([vkf, k2]); vpx = np.concatenate([vpx, p2]); xyz = np.concatenate([xyz, x2])
    _, st, info = tr.triangulate(R, t, *tr.K4, offs, vkf, vpx, xyz, details=True)
    V = np.diff(offs)
    ran = st != tr.LOW_PARALLAX
    assert ran.sum() > 250 and ran[-1]
    assert (info["sweeps"][ran] < np.maximum(2 * V[ran], 30)).all()
    assert info["sweeps"][ran].max() <= 12
