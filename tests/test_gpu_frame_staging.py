"""The staging of the host forms (csrc/maptrack_internal.h, FrameStaging): dvs_maptrack_track and dvs_reloc_locate upload their five arrays
into two row groups that only grow, and call their device forms.  One MapTracker and one Relocalizer take a small frame, one past 1.25 x
the first (both groups regrow), a smaller one (nothing regrows: the groups hold more rows than the call uses) and an empty one; every
result and every per-keypoint / per-pair list must equal, byte for byte, what a fresh handle returns for the same inputs, and what the
device form returns on the same arrays uploaded by the test."""
import numpy as np
import pytest
import map_track_ref as mr
from test_gpu_map_track import ROWS, COLS, F, CX, CY, P0, _handle, _dev

pytestmark = pytest.mark.gpu

SIZES = [(32, 24), (200, 160), (8, 6), (0, 0)]        # (n_lm, n_kp)
I3, Z3 = np.eye(3), np.zeros(3)


def frame(n_lm, n_kp, seed):
    """n_lm landmarks in front of the identity pose, inside the image; keypoints at the projections of the first n_kp of them, in another
    order, with their descriptors and a few flipped bits; ascending ids that are not the row numbers"""
    rng = np.random.default_rng(seed)
    z = rng.uniform(1.0, 3.0, n_lm)
    u = rng.uniform(4, COLS - 5, n_lm); v = rng.uniform(4, ROWS - 5, n_lm)
    xyz = np.stack([(u - CX) * z / F, (v - CY) * z / F, z], 1).astype(np.float32).reshape(-1, 3)
    ldesc = mr.random_descriptors(rng, n_lm)
    perm = rng.permutation(n_lm)[:n_kp]
    kps = mr.keypoints(np.stack([u[perm], v[perm]], 1).astype(np.float32).reshape(-1, 2))
    kps["octave"] = rng.integers(0, 4, n_kp)
    kdesc = np.ascontiguousarray(ldesc[perm]).reshape(-1, 32)
    for k in range(n_kp):
        kdesc[k, rng.integers(0, 32)] ^= np.uint8(1 << int(rng.integers(0, 8)))
    return xyz, ldesc, np.arange(n_lm, dtype=np.int64) * 5 + 11, kps, kdesc


def same(a, b):
    """two result dicts, byte for byte"""
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], dict):
            same(a[k], b[k])
        else:
            assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


def same_lists(a, b):
    assert len(a) == len(b) and all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.fixture(scope="module")
def frames():
    return [frame(n_lm, n_kp, 100 + i) for i, (n_lm, n_kp) in enumerate(SIZES)]


def _uploaded(f):
    xyz, ldesc, ids, kps, kdesc = f
    return [_dev(xyz), _dev(ldesc), _dev(ids), _dev(kps), _dev(kdesc)]


def test_map_tracker_host_form_across_regrowth(gpu, frames):
    kept = _handle(P0)
    saw_matches = False
    for (n_lm, n_kp), f in zip(SIZES, frames):
        xyz, ldesc, ids, kps, kdesc = f
        res = kept.track(xyz, ldesc, ids, kps, kdesc, I3, Z3); lists = kept.matches()
        fresh = _handle(P0)
        want = fresh.track(xyz, ldesc, ids, kps, kdesc, I3, Z3); want_lists = fresh.matches()
        print((n_lm, n_kp), {k: res[k] for k in ("status", "n_visible", "n_matches", "n_inliers")})
        same(res, want); same_lists(lists, want_lists)
        assert len(lists[0]) == n_kp
        bufs = _uploaded(f)
        dev = fresh.track_device(bufs[0], bufs[1], bufs[2], n_lm, bufs[3], bufs[4], n_kp, I3, Z3); dev_lists = fresh.matches()
        same(res, dev); same_lists(lists, dev_lists)
        for b in bufs:
            b.free()
        fresh.close()
        saw_matches = saw_matches or res["n_matches"] > 0
    assert saw_matches                                   # the comparison is not one of empty results
    kept.close()


def test_relocalizer_host_form_across_regrowth(gpu, frames):
    from dvslam_amd import reloc as RL

    def make():
        return RL.Relocalizer(RL.default_params(F, F, CX, CY, min_pairs=6, min_pnp_inliers=5, min_confirmed=5), hooks=True)
    mt = _handle(P0)
    kept = make()
    saw_pairs = False
    for (n_lm, n_kp), f in zip(SIZES, frames):
        xyz, ldesc, ids, kps, kdesc = f
        res = kept.locate(mt, xyz, ldesc, ids, kps, kdesc); lists = kept.pairs()
        fresh = make()
        want = fresh.locate(mt, xyz, ldesc, ids, kps, kdesc); want_lists = fresh.pairs()
        print((n_lm, n_kp), {k: res[k] for k in ("status", "n_proposed", "n_pairs", "pnp_inliers")})
        same(res, want); same_lists(lists, want_lists)
        bufs = _uploaded(f)
        dev = fresh.locate_device(mt, bufs[0], bufs[1], bufs[2], n_lm, bufs[3], bufs[4], n_kp); dev_lists = fresh.pairs()
        same(res, dev); same_lists(lists, dev_lists)
        for b in bufs:
            b.free()
        fresh.close()
        saw_pairs = saw_pairs or res["n_pairs"] > 0
    assert saw_pairs
    kept.close(); mt.close()
