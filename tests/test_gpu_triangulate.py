"""GPU: dvs_triangulate_landmarks[_device] (csrc/triangulate.hip) against the numpy restatement tests/triangulate_ref.py, bit for bit:
positions compared as uint32, statuses equal."""
import ctypes as C
import numpy as np
import pytest
import triangulate_ref as tr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def glue(gpu):
    from dvslam_amd.glue import FrontendGlue
    return FrontendGlue()


def _same(glue, R, t, offs, vkf, vpx, xyz):
    got, gst = glue.triangulate_landmarks(R, t, *tr.K4, offs, vkf, vpx, xyz)
    want, wst = tr.triangulate(R, t, *tr.K4, offs, vkf, vpx, xyz)
    assert gst.tolist() == wst.tolist(), np.nonzero(gst != wst)[0][:10]
    bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))[0]
    assert len(bad) == 0, (bad[:10], got[bad[:3]], want[bad[:3]])
    return got, gst


def _concat(*scenes):
    offs = [np.zeros(1, np.int64)]; base = 0
    for o, *_ in scenes:
        offs.append(o[1:] + base); base += o[-1]
    return (np.concatenate(offs), np.concatenate([s[1] for s in scenes]), np.concatenate([s[2] for s in scenes]),
            np.concatenate([s[3] for s in scenes]))


def test_views_2_to_40_and_300(glue):
    rng = np.random.default_rng(101)
    R, t, _ = tr.keyframes(rng, 48)
    scenes = [tr.random_landmarks(rng, R, t, 12, v, v, noise=0.7)[:4] for v in range(2, 41)]
    scenes.append(tr.random_landmarks(rng, R, t, 1, 300, 300, noise=0.7)[:4])
    offs, vkf, vpx, xyz = _concat(*scenes)
    _, st = _same(glue, R, t, offs, vkf, vpx, xyz)
    assert (st == tr.UPDATED).mean() > 0.8 and st[-1] == tr.UPDATED


def test_skipped_views(glue):
    rng = np.random.default_rng(102)
    R, t, _ = tr.keyframes(rng, 16)
    offs, vkf, vpx, xyz, _ = tr.random_landmarks(rng, R, t, 2000, 1, 12, noise=0.5, skip=0.3)
    assert (vkf < 0).sum() > 500
    _same(glue, R, t, offs, vkf, vpx, xyz)


def test_every_status_scene(glue):
    R, t, offs, vkf, vpx, xyz, expected = tr.status_scenes()
    got, st = _same(glue, R, t, offs, vkf, vpx, xyz)
    assert st.tolist() == expected
    assert got[st != tr.UPDATED].tobytes() == xyz[st != tr.UPDATED].tobytes()


def test_100k_random_landmarks(glue):
    rng = np.random.default_rng(103)
    R, t, _ = tr.keyframes(rng, 64, span=3.0)
    offs, vkf, vpx, xyz, _ = tr.random_landmarks(rng, R, t, 100_000, 1, 14, noise=1.5, perturb=0.2, skip=0.05, depth=(1.0, 12.0))
    _, st = _same(glue, R, t, offs, vkf, vpx, xyz)
    counts = np.bincount(st, minlength=6)
    assert counts[tr.UPDATED] > 50_000 and counts[tr.FEW_VIEWS] > 0 and counts[tr.DEPTH] > 0, counts


def test_device_entry_point_and_in_place(glue, hiplib):
    from dvslam_amd._lib import DeviceBuffer, check, ptr
    rng = np.random.default_rng(104)
    R, t, _ = tr.keyframes(rng, 20)
    offs, vkf, vpx, xyz, _ = tr.random_landmarks(rng, R, t, 3000, 1, 20, noise=0.5, skip=0.1)
    want, wst = tr.triangulate(R, t, *tr.K4, offs, vkf, vpx, xyz)
    # host entry point, output aliasing the input
    xin = xyz.copy(); st = np.zeros(len(xyz), np.int32)
    check(hiplib.dvs_triangulate_landmarks(glue._h, len(R), ptr(R), ptr(t), *tr.K4, len(xyz), ptr(offs), ptr(vkf), ptr(vpx), ptr(xin), ptr(xin), ptr(st)))
    assert xin.tobytes() == want.tobytes() and st.tolist() == wst.tolist()
    # device entry point, separate output and in place
    bufs = [DeviceBuffer(a.nbytes).upload(a) for a in (R, t, offs, vkf, vpx, xyz)]
    d_out = DeviceBuffer(xyz.nbytes); d_st = DeviceBuffer(st.nbytes)
    dR, dt, do, dk, dp, dx = (b.ptr for b in bufs)
    for out in (d_out.ptr, dx):
        check(hiplib.dvs_triangulate_landmarks_device(glue._h, len(R), dR, dt, *tr.K4, len(xyz), do, dk, dp, dx, out, d_st.ptr))
        check(hiplib.dvs_matcher_synchronize(glue._h))
        got = (d_out if out == d_out.ptr else bufs[5]).download(np.float32, xyz.size).reshape(-1, 3)
        assert got.tobytes() == want.tobytes() and d_st.download(np.int32, len(xyz)).tolist() == wst.tolist()
    # the device form marks landmarks whose keyframe index is out of range, the rest are computed as usual
    bad = vkf.copy(); bad[offs[5]] = len(R)
    bufs[3].upload(bad); bufs[5].upload(xyz)
    check(hiplib.dvs_triangulate_landmarks_device(glue._h, len(R), dR, dt, *tr.K4, len(xyz), do, dk, dp, dx, d_out.ptr, d_st.ptr))
    check(hiplib.dvs_matcher_synchronize(glue._h))
    dst = d_st.download(np.int32, len(xyz)); got = d_out.download(np.float32, xyz.size).reshape(-1, 3)
    assert dst[5] == -6 and got[5].tobytes() == xyz[5].tobytes()
    keep = np.arange(len(xyz)) != 5
    assert dst[keep].tolist() == wst[keep].tolist() and got[keep].tobytes() == want[keep].tobytes()


def test_no_landmarks_and_bad_arguments(glue, hiplib):
    from dvslam_amd._lib import ptr
    h = glue._h
    R = np.eye(3).reshape(1, 9).repeat(2, 0); t = np.zeros((2, 3)); t[1, 0] = -1
    px = np.full((4, 2), 300, np.float32); xyz = np.ones((2, 3), np.float32); st = np.zeros(2, np.int32); out = np.zeros((2, 3), np.float32)
    z = np.zeros(1, np.int64)
    assert hiplib.dvs_triangulate_landmarks(h, 2, ptr(R), ptr(t), *tr.K4, 0, ptr(z), None, None, None, None, None) == 0
    assert hiplib.dvs_triangulate_landmarks_device(h, 2, None, None, *tr.K4, 0, None, None, None, None, None, None) == 0
    call = lambda offs, kf, nkf=2, nlm=2: hiplib.dvs_triangulate_landmarks(h, nkf, ptr(R), ptr(t), *tr.K4, nlm, ptr(np.array(offs, np.int64)),
                                                                          ptr(np.array(kf, np.int32)), ptr(px), ptr(xyz), ptr(out), ptr(st))
    assert call([0, 2, 4], [0, 1, 0, 1]) == 0
    assert call([0, 2, 4], [0, 2, 0, 1]) == -6                 # view_kf >= nkf
    assert call([0, 3, 2], [0, 1, 0, 1]) == -6                 # offsets decrease
    assert call([-1, 2, 4], [0, 1, 0, 1]) == -6                # negative offset
    assert call([0, 2, 4], [0, 1, 0, 1], nlm=-1) == -6         # negative counts
    assert call([0, 2, 4], [0, 1, 0, 1], nkf=-1) == -6
