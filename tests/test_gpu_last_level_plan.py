"""GPU: the relpose_scnet_plan_macs contract of tests/test_last_level_plan_cpu.py under the gpu mark, so that it is executed wherever the
GPU suite runs (that file carries no mark and skips without a device): values 0 and 1 are the parent commit's, value 2 -- cached behind a
pose-outputs fill -- adds exactly the rgb head's skip halves, counted there from the network's definition."""
import pytest

import test_last_level_plan_cpu as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def net():
    return P.make_net()


@pytest.mark.parametrize("n", P.SIZES)
def test_plan_macs_values_and_the_rgb_skip_halves(net, n):
    P.check_parent_values(net, n)
    P.check_order(net, n)
    P.check_value_2_counts_the_rgb_skip_halves(net, n)
