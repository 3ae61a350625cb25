"""The device leg of tests/test_problem_arrays.py: the same handful of tiny problems, rebuilt from exact-length copies of the arrays `ks_debug_problem_array` names,
uploaded and solved on the MI355X in one child process."""
import pytest

import test_problem_arrays as A


@pytest.mark.gpu
def test_exact_length_rebuilds_solve_on_the_device(request):
    A.check_rebuilds(request, "gpu")
