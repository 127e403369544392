"""CPU: tests/pt_layer_oracle.py — the float64 oracle of csrc/pt_layer.hip's six entries and the driver that tests/test_gpu_pt_layer_oracle.py runs on the
device — run against the host-emulated kernels (the builds of tests/test_pt_layer_host.py and tests/test_pt_layer_wide_host.py): the narrow edge scenes and one
scene past a grid cap, two wide edge scenes, the argument checks; and the flip-free construction alone on EVERY scene of the device file, so that its two limits
(rounds, touched share) are known to hold before a GPU is asked."""
import pytest

from tests import pt_layer_oracle as O
from tests.attention_oracle import HostBackend
from tests.test_pt_layer_host import host as narrow_library            # noqa: F401  (fixtures: the two host builds)
from tests.test_pt_layer_wide_host import host as wide_library         # noqa: F401


@pytest.fixture(scope="module")
def narrow(narrow_library):
    return O.LayerEntries(narrow_library, HostBackend())


@pytest.fixture(scope="module")
def wide(wide_library):
    return O.LayerEntries(wide_library, HostBackend())


@pytest.mark.parametrize("n,K,C", O.NARROW_EDGE + [(2100, 16, 64)])
def test_narrow_entries_on_the_host(narrow, n, K, C):
    """training forward (all outputs and buffers) and backward (17 gradients) without and with an order, and the evaluation-mode forward"""
    idx, t, _, _ = O.case(n, K, C)
    tag = "host (%d, %d, %d)" % (n, K, C)
    O.check_narrow(narrow, idx, t, O.reference_layer(idx, t), tag, idx.size)
    ref = O.reference_layer(idx, t, training=False)
    for name, table in O.tables(idx, idx.size).items():
        got, _ = narrow.forward(idx, t, table[0], "eval")
        O.check_eval(got, ref, t, "narrow eval %s %s:" % (tag, name))


@pytest.mark.parametrize("n,K,C", [(37, 5, 128), (23, 16, 256)])
def test_wide_entries_on_the_host(wide, n, K, C):
    idx, t, _, _ = O.case(n, K, C)
    O.check_wide(wide, idx, t, O.reference_layer(idx, t), "host (%d, %d, %d)" % (n, K, C), idx.size)


def test_refused_calls_on_the_host(narrow, wide):
    O.check_arguments(narrow, wide=False)
    O.check_arguments(wide, wide=True)


@pytest.mark.parametrize("n,K,C", O.NARROW_EDGE + O.NARROW_CAPS + O.wide_scenes())
def test_flip_free_construction_within_its_limits(n, K, C):
    """make_flip_free asserts its own three conditions (nothing within 1e-5 of zero at the end, at most 12 rounds, at most 3 % of the points touched); here
    they are held on every scene the device file compares gradients on, and the result is looked at once more from outside"""
    idx, t, touched, rounds = O.case(n, K, C)
    assert rounds <= 12 and touched <= 0.03 * n
    assert O.near_zero(idx, t)[3] >= 1e-5
