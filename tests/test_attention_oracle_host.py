"""CPU: tests/attention_oracle.py — the float64 oracle of csrc/attention.hip and the driver that tests/test_gpu_attention.py runs on the device — run once
against the host-emulated library (tests/host_emul/full_library.py), one small scene per width with every check of the device file (training and evaluation
forward, both aggregations, the scatter and the gather backward entries with and without an `order`; C = 32 / 64 also with unaligned rows), so that a slip in
the oracle or in a call shows up without a GPU; and the flip-free construction alone on the two largest device scenes that have gradients."""
import numpy as np
import pytest

from tests import attention_oracle as O
from tests.host_emul import full_library


@pytest.fixture(scope="module")
def entries():
    return O.Entries(full_library.load(), O.HostBackend())


@pytest.mark.parametrize("n,K,C", [(40, 8, 32), (33, 17, 64), (37, 5, 128), (23, 16, 256), (17, 33, 512)])
def test_oracle_against_the_host_emulated_entries(entries, n, K, C):
    idx, a, _, _ = O.case(n, K, C)
    O.check_all(entries, idx, a, "host (%d, %d, %d)" % (n, K, C), unaligned=C <= 64)


def test_neighbour_tables_hold_their_special_rows():
    for n, K in ((41, 8), (50, 1), (9, 64), (2600, 8)):
        idx = O.neighbours(n, K, n + K)
        count = np.bincount(idx.reshape(-1), minlength=n)
        assert idx.dtype == np.int32 and count[n - 1] == 0 and (idx[n // 3] == O.REPEATED).all()
        assert all(idx[i, 0] == i for i in range(n - 1) if i != n // 3)
        assert K == 1 or (count[O.HUB] > 3 * K and count[O.HUB] % 4 != 0)
        for order in (None, np.random.default_rng(n).permutation(n).astype(np.int32)):
            inv_start, inv_src = O.transposed(idx, order)
            for r in (0, n // 3, n - 1):
                j = r if order is None else order[r]
                assert sorted(inv_src[inv_start[r]:inv_start[r + 1]]) == list(np.flatnonzero(idx.reshape(-1) == j))


@pytest.mark.parametrize("n,K,C", [(16500, 17, 32), (4200, 16, 64)])
def test_flip_free_construction_within_its_limits(n, K, C):
    """the two limits are conditions of the construction: at most 8 rounds (asserted by make_flip_free itself), at most 0.1 % of the pairs touched.  On the two
    device scenes with gradients that have the most pairs (280500 and 67200).  A pair is touched when ANY of its C channels is within 1e-5 of zero, which happens
    with probability C * 2e-5 * (the density of z at 0, about 0.4): 0.03 % of the pairs at C = 32, 0.05 % at 64 — and 0.1 / 0.2 / 0.4 % at C = 128 / 256 / 512,
    whatever the seed, so the share is a condition only at the narrow widths and a printed figure at the wide ones (O.case)."""
    seed = n + K + C
    idx, a = O.neighbours(n, K, seed), O.scene(n, K, C, seed + 1)
    before = a["p1"].copy()
    touched = O.make_flip_free(idx, a, seed=seed + 2)
    print("(%d, %d, %d): %d of %d pairs touched in %d rounds" % (n, K, C, touched, n * K, O.make_flip_free.rounds))
    assert O.make_flip_free.rounds <= 8 and touched <= 1e-3 * n * K
    moved = (a["p1"] != before).any(-1)
    assert int(moved.sum()) == touched and float(np.abs(a["p1"] - before).max()) <= 8 * 2e-3 + 1e-6
    assert float(O.min_abs_z(idx, a).min()) >= 1e-5
