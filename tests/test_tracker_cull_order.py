"""The tracker's feature-culling ORDER (csrc/cull_order.h, run by k_cull on the device and by dvs_test_cull_order on the host) against the
reference's literal steps with the real std::sort on std::pair<float, int> (tests/cpp/cull_std_sort.cpp, built here with g++):
frontend.cpp:1201-1202 sorts under a comparator that looks at the response only, FAST scores are small integers with many ties, so
for more than 16 unmatched features libstdc++'s introsort decides which <= 200 a keyframe carries.  Index-for-index equality."""
import os
import subprocess
import numpy as np
import pytest
import tracker_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def std_sort(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("cull")), "cull_std_sort")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "cull_std_sort.cpp"), "-o", exe])

    def run(response, matched, max_new=200, min_response=50.0, stable=False):
        text = f"{len(response)} {max_new} {min_response!r}\n" + "".join(f"{float(r)!r} {int(m)}\n" for r, m in zip(response, matched))
        out = subprocess.run([exe] + (["stable"] if stable else []), input=text, capture_output=True, text=True, check=True)
        return np.array([int(v) for v in out.stdout.split()], np.int64)
    return run


def _cases():
    rng = np.random.default_rng(20240)
    values = np.array([7, 20, 49, 50, 51, 64, 80, 120], np.float32)
    for n in (0, 1, 16, 17, 200, 201, 1000, 2024):
        resp = rng.choice(values, n).astype(np.float32)
        yield f"n={n} random matches", resp, (rng.random(n) < 0.4).astype(np.uint8)
        yield f"n={n} none matched", resp, np.zeros(n, np.uint8)
        yield f"n={n} all matched", resp, np.ones(n, np.uint8)
        yield f"n={n} every response below 50", rng.choice(values[:3], n).astype(np.float32), np.zeros(n, np.uint8)
        yield f"n={n} two values", rng.choice(values[4:6], n).astype(np.float32), (rng.random(n) < 0.1).astype(np.uint8)
    resp = rng.choice(values[:3], 1000).astype(np.float32)
    resp[rng.choice(1000, 200, replace=False)] = rng.choice(values[3:], 200)
    yield "exactly 200 at >= 50", resp, np.zeros(1000, np.uint8)
    yield "fractional responses", (rng.integers(0, 400, 777) / 4.0).astype(np.float32), (rng.random(777) < 0.3).astype(np.uint8)


def test_stable_order_differs_from_std_sort(std_sort, hooks):
    """the case that rules out a stable sort: 300 unmatched features of two response values.  std::sort's order of the ties is not the
    index order, so the cut at 200 keeps other features; the hook follows std::sort"""
    rng = np.random.default_rng(5)
    resp = rng.choice(np.array([60, 90], np.float32), 300)
    matched = np.zeros(300, np.uint8)
    real, stable = std_sort(resp, matched), std_sort(resp, matched, stable=True)
    assert len(real) == len(stable) == 200 and (real != stable).any() and set(real.tolist()) != set(stable.tolist())
    assert (ref.cull_order(hooks, resp, matched) == real).all()


def test_cull_order_equals_std_sort_index_for_index(std_sort, hooks):
    checked = 0
    for name, resp, matched in _cases():
        want = std_sort(resp, matched)
        got = ref.cull_order(hooks, resp, matched)
        assert len(got) == len(want) and (got == want).all(), name
        assert len(got) <= 200 and (resp[got] >= 50.0).all() and not matched[got].any(), name
        checked += 1
    assert checked == 42
    # other limits
    rng = np.random.default_rng(9)
    resp = rng.choice(np.array([10, 30, 31], np.float32), 500); matched = (rng.random(500) < 0.2).astype(np.uint8)
    assert (ref.cull_order(hooks, resp, matched, 37, 30.0) == std_sort(resp, matched, 37, 30.0)).all()
    assert len(ref.cull_order(hooks, resp, matched, 0, 30.0)) == 0
