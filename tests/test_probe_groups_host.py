"""The group-size rule of the Krylov vector passes (`mfx_probe_group`, include/mfx.h) as the library itself evaluates it: the
chosen power of two at BASELINE config 4, "all probes in one launch" -- the launches of every earlier build, and the hipGraph keys
with them -- for every other config and for the shapes of tests/test_gpu_graphs.py, and a valid partition of the probes for any shape."""

import re
import os

import pytest

from matfree_extensions import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _budget():
    src = open(os.path.join(ROOT, "experiments-lanczos-adjoints_amd", "csrc", "mfx_internal.h")).read()
    m = re.search(r"kProbeGroupBudgetBytes = \(int64_t\)(\d+) << 20;", src)
    assert m, "budget constant not found"
    return int(m.group(1)) << 20


def test_config_4_gets_a_power_of_two_that_fits_the_budget():
    n, k, p, es = 131072, 40, 64, 4
    for adjoint in (False, True):
        g = _lib.probe_group(n, k, p, es, adjoint)
        per_probe = k * n * es * (2 if adjoint else 1)
        if p * per_probe <= _budget():
            assert g == p  # grouping not enabled: the budget holds all probes
            continue
        assert 1 <= g < p and g & (g - 1) == 0
        assert g == 1 or g * per_probe <= _budget()
        assert 2 * g * per_probe > _budget()  # the LARGEST such power of two
    assert _lib.probe_group(n, k, p, es, True) <= _lib.probe_group(n, k, p, es, False)


# (n, k, p, element size): BASELINE configs 1, 2, 3, 5 and the launch-bound shapes of tests/test_gpu_graphs.py
SMALL = [(512, 20, 1, 8), (512, 20, 1, 4), (45730, 30, 8, 4), (36584, 30, 8, 4), (102400, 50, 1, 8), (2_000_000, 30, 1, 8),
         (2_000_000, 10, 1, 8), (96, 6, 1, 8), (576, 8, 1, 8), (80, 7, 1, 8), (80, 7, 3, 8), (600, 12, 32, 4)]


@pytest.mark.parametrize("n,k,p,es", SMALL)
@pytest.mark.parametrize("adjoint", [False, True])
def test_small_problems_launch_exactly_as_before(n, k, p, es, adjoint):
    assert _lib.probe_group(n, k, p, es, adjoint) == p


def test_groups_always_partition_the_probes():
    for n in (1, 1003, 131072, 4_000_000, 1 << 33):
        for k in (1, 3, 40, 500):
            for p in (1, 2, 5, 64, 65, 1000, 65535):
                for es in (4, 8):
                    for adjoint in (False, True):
                        g = _lib.probe_group(n, k, p, es, adjoint)
                        assert 1 <= g <= p, (n, k, p, es, adjoint, g)
                        groups = -(-p // g)
                        assert (groups - 1) * g < p <= groups * g
                        assert g == p or g & (g - 1) == 0
    with pytest.raises(ValueError):
        _lib.probe_group(0, 1, 1, 4, False)
