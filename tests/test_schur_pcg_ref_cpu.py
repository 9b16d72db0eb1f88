"""CPU: the dense restatement of the global BA solver's linear solve (tests/schur_pcg_ref.py) on the four test systems, from the
oracle's normal equations: the stopping rule delivers the residual it promises and the default iteration cap is never what stops it."""
import numpy as np
import pytest
import schur_pcg_ref as ref

_CACHE = {}


def _system(oracle, name, radius):
    key = (name, radius)
    if key not in _CACHE:
        if name not in _CACHE:
            P = ref.system_problem(name)
            _CACHE[name] = (P, oracle.OracleBA(P).normal_equations())
        P, (hpp, hll, w, g, _) = _CACHE[name]
        _CACHE[key] = ref.SchurSystem(P, hpp, hll, w, g, radius)
    return _CACHE[key]


@pytest.mark.parametrize("radius", [1e4, 1e8])
@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_restatement_reaches_the_residual_inside_the_cap(oracle, name, radius):
    s = _system(oracle, name, radius)
    bn = np.linalg.norm(s.b)
    assert bn > 0 and np.abs(s.S - s.S.T).max() <= 1e-12 * np.abs(s.S).max()
    rows = []
    for eta in (1e-1, 1e-6, 1e-10):
        x, k, rel, ok = s.pcg(eta)
        true = np.linalg.norm(s.S @ x - s.b)
        rows.append((eta, k, rel, true / bn))
        assert ok == 1 and k >= 1
        assert true <= 2 * eta * bn, f"({name}) radius {radius:g} eta {eta:g}: true residual {true / bn:.3e} |b| after {k} iterations"
    print(f"({name}) radius {radius:g} nc {s.nc} cond {np.linalg.cond(s.S[np.ix_(np.repeat(s.free, 6), np.repeat(s.free, 6))]):.2e}: "
          + ", ".join(f"eta {e:g}: {k} it, rec {r:.2e}, true {t:.2e}" for e, k, r, t in rows))
    assert rows[-1][1] < ref.default_cap(s.nc)


def test_banded_generator_is_make_ba_problem_with_a_band(oracle):
    from dvslam_amd import synth
    full = synth.make_ba_problem(K=80, L=400, seed=80)
    band = synth.make_ba_banded_problem(K=80, L=400, seed=80, half_span=4)
    keep = np.abs(full["cam_idx"].astype(np.int64) - (full["lm_idx"].astype(np.int64) * 80) // 400) <= 4
    assert (band["cam_idx"] == full["cam_idx"][keep]).all() and (band["lm_idx"] == full["lm_idx"][keep]).all()
    assert (band["uv"] == full["uv"][keep]).all() and (band["q"] == full["q"]).all() and (band["X"] == full["X"]).all()
    cc = np.bincount(band["cam_idx"], minlength=80); lc = np.bincount(band["lm_idx"], minlength=400)
    assert (cc.min(), cc.max(), lc.min(), lc.max()) == (25, 45, 5, 9)
