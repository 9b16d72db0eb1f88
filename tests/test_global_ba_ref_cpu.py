"""CPU: the problem-assembly rule of dvs_backend_global_ba as tests/global_ba_ref.py restates it, on a hand-made map of three keyframes:
a landmark with a single observation, an observation whose landmark is gone, and a landmark nobody observes."""
import numpy as np
import global_ba_ref as gr


def test_assembly_rule_on_a_hand_made_map(hiplib):
    c, s = np.cos(0.1), np.sin(0.1)
    kfs = dict(frame_id=np.array([10, 11, 12], np.uint64),
               R=np.array([np.eye(3), [[c, 0, s], [0, 1, 0], [-s, 0, c]], np.diag([-1.0, -1.0, 1.0])]),
               t=np.array([[0.0, 0, 0], [0.5, 0, 0.1], [1.0, -0.2, 0]]))
    lms = dict(id=np.array([2, 5, 7, 9], np.uint64), xyz=np.array([[0.1, 0.2, 3.0], [1, 1, 4], [-0.5, 0.25, 2.5], [0, 0, 5]], np.float32))
    #            landmark: 2 in all three keyframes; 5 once; 7 twice; 8 is not in the table; 9 never
    obs = dict(frame_id=np.array([10, 10, 11, 11, 11, 12, 12], np.uint64), landmark_id=np.array([2, 7, 2, 5, 8, 7, 2], np.uint64),
               px=np.array([[100.5, 50], [20, 30], [101, 51], [300, 200], [7, 7], [22, 33], [99.25, 49]], np.float32))
    P, left_out, used = gr.assemble(kfs, lms, obs, 500.0, 510.0, 320.0, 240.0)
    assert (P["K"], P["L"], left_out) == (3, 4, 2)
    assert P["cam_idx"].tolist() == [0, 0, 1, 2, 2] and P["lm_idx"].tolist() == [0, 2, 0, 2, 0]
    assert P["uv"].tolist() == [[100.5, 50], [20, 30], [101, 51], [22, 33], [99.25, 49]]
    assert used.tolist() == [True, False, True, False]
    assert P["pose_fixed"].tolist() == [1, 0, 0] and not P["lm_fixed"].any()
    assert (P["X"] == lms["xyz"].astype(np.float64)).all() and P["X"].dtype == np.float64
    assert (P["fx"], P["fy"], P["cx"], P["cy"], P["sigma"], P["huber"]) == (500.0, 510.0, 320.0, 240.0, 1.0, 1.345)
    # world -> camera: q of the identity, and translation = -R^T t
    assert np.allclose(P["q"][0], [1, 0, 0, 0]) and np.allclose(P["t"][1], -kfs["R"][1].T @ kfs["t"][1], atol=1e-15)
    for k in range(3):                                   # the round trip the result takes back into the map
        R, t = gr.pose_to_rt(P["q"][k], P["t"][k])
        assert np.abs(R - kfs["R"][k]).max() < 1e-15 and np.abs(t - kfs["t"][k]).max() < 1e-15
