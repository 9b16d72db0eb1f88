"""The mapping backend's per-call scratch on ONE handle that lives through a whole map: after every keyframe of backend_ref.make_scene()
the sliding window, the anchors, the covisibility graph, the local window of the newest keyframe and a fusion dry run of the newest keyframe
against its predecessors, each bit for bit against the restatements (backend_ref, loop_closing_ref, covisibility_ref), then a prune in the
middle of the tables and the round once more.  The other backend files make these calls on fresh handles or on a finished map; here every
row group of the handle (csrc/backend_internal.h) is first sized by a small map and later outgrown, with the other groups' calls in between.
A group grown from the wrong count, a column left out of its group or two calls that came to share a group fail here."""
import numpy as np
import pytest

import backend_ref as br
import covisibility_ref as cr
import loop_closing_ref as lc

pytestmark = pytest.mark.gpu


def _same(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        if want[k] is None or np.isscalar(want[k]):
            assert got[k] == want[k], (what, k, got[k], want[k])
            continue
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (what, k)


def _round(mb, ref, what):
    """every call that owns scratch, on the map as it stands"""
    _same(mb.landmarks(), ref.landmark_table(), what + " landmarks")
    _same(mb.observations(), ref.observation_table(), what + " observations")
    _same(mb.keyframes(), ref.keyframe_table(), what + " keyframes")
    _same(mb.window(), ref.window_table(), what + " window")
    ids, anc = mb.anchors()
    want_ids, want_anc = lc.anchors(ref)
    assert ids.dtype == np.uint64 and anc.dtype == np.int32 and ids.tobytes() == want_ids.tobytes() and anc.tobytes() == want_anc.tobytes(), what + " anchors"
    T = cr.tables(ref)
    for theta in (1, 15):
        _same(mb.covisibility(theta), cr.graph(*T, theta), f"{what} graph at {theta}")
    frames = [int(f) for f in T[0]["frame_id"]]
    want = cr.local_window(*T, frames[-1])
    want.pop("kf_index")
    _same(mb.local_window(frames[-1]), want, what + " local window")
    if len(frames) < 2:
        return 0
    want = lc.fuse(ref, frames[-1], frames[:-1], cr.FUSED_PARAMS, apply=False)
    got = mb.fuse(frames[-1], frames[:-1], apply=False, **cr.FUSED_PARAMS)
    for k in ("n_sources", "n_targets", "n_proposals", "n_fused"):
        assert got[k] == want[k], (what, "fusion", k, got[k], want[k])
    sv, rm, err = got["pairs"]
    assert sv.tolist() == [p[0] for p in want["pairs"]] and rm.tolist() == [p[1] for p in want["pairs"]], what + " fusion pairs"
    assert err.tobytes() == np.array([p[2] for p in want["pairs"]], np.float64).tobytes(), what + " fusion errors"
    return want["n_fused"]


def test_one_handle_outgrows_every_scratch_group(gpu):
    from dvslam_amd.backend import MappingBackend
    scene = br.make_scene()
    assert len(scene) == 10
    mb = MappingBackend(br.FX, br.FY, br.CX, br.CY, filtered=("person",), initial_capacity=64)
    assert mb.intern("person") == br.PERSON and mb.intern("chair") == br.CHAIR and mb.intern("table") == br.TABLE
    ref = br.BackendRef(br.FX, br.FY, br.CX, br.CY, filtered=(br.PERSON,))
    sizes, fused = [], 0
    for k, kf in enumerate(scene):
        assert lc.add(mb, kf) == lc.add(ref, kf), k
        sizes.append((len(ref.landmark_table()["id"]), len(ref.observation_table()["id"])))
        fused += _round(mb, ref, f"keyframe {k}")
    # the fixture condition: the groups sized at the first keyframe (the largest rule is half to spare plus 64) must all be outgrown
    assert sizes[-1][0] > 1.5 * sizes[0][0] + 64 and sizes[-1][1] > 1.5 * sizes[0][1] + 64, sizes
    assert fused > 0, "the dry runs must find pairs"
    now = (scene[2]["stamp"][0] + 20, scene[2]["stamp"][1] + 1)     # landmarks last seen in keyframes 0 .. 2 are older than 20 s
    want = ref.prune(now)
    assert mb.prune(now) == want and want[0] > 20
    lid = ref.landmark_table()["id"]
    assert lid[0] < 50 and (np.diff(lid.astype(np.int64)) > 1).sum() > 5, "the prune must leave holes in the middle of the table"
    _round(mb, ref, "after prune")
    assert ref.ties == 0
    mb.close()
