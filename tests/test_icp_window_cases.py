"""The inputs of tests/test_gpu_icp_window.py, judged by the oracle alone (no GPU): the seeded
family of tests/icp_window_cases.py has a det failure at each of the five positions the persistent
ICP's control flow distinguishes, under both OpenCV algebras, and a launch that runs every
iteration."""
import numpy as np
import pytest

import icp_window_cases as C
from test_gpu_icp_window import ALGEBRAS, SEEDS, _expect


@pytest.fixture
def cv_oracle(oracle_mod):
    yield oracle_mod
    oracle_mod.set_pose_algebra("opencv4")


@pytest.mark.parametrize("algebra", ALGEBRAS)
def test_family_covers_every_position(cv_oracle, algebra):
    exp = _expect(cv_oracle, algebra)
    classes = {C.position(n) for ok, n, _, _ in exp.values() if not ok}
    assert classes == set(range(5)), [C.CLASSES[c] for c in sorted(set(range(5)) - classes)]
    assert any(ok and n == sum(C.ITERS) for ok, n, _, _ in exp.values())
    for ok, n, _, sums in exp.values():
        assert 1 <= n <= sum(C.ITERS) and np.isfinite(sums).all()
    # every iteration index of the 3 + 3 + 3 schedule fails in some case
    assert {n - 1 for ok, n, _, _ in exp.values() if not ok} == set(range(9))
