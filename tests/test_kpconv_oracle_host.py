"""CPU: tests/kpconv_oracle.py — the float64 oracle of KPConv, its scene generator and the driver that tests/test_gpu_kpconv_oracle.py runs on the device —
on the host-emulated kernels (the build of local_aggregation.hip + kpconv_backward.hip that tests/test_local_aggregation_host.py makes, unchanged): every EDGE
scene in all four (influence, mode) combinations through both forward entries, the scatter entry and the gather entry over the numpy-built tables, so that a
slip in the oracle, in a scene or in a call shows up without a GPU.  The oracle itself is held once against the older restatement
(oracle/local_aggregation_oracle.py), so the two cannot drift; and the scene conditions are asserted for the device file's large shapes as well."""
import numpy as np
import pytest

from oracle import local_aggregation_oracle as LA
from tests import kpconv_oracle as O
from tests.test_local_aggregation_host import host  # noqa: F401  (the fixture that builds and loads the host library)


@pytest.fixture(scope="module")
def entries(host):  # noqa: F811
    return O.Entries(host, O.HostBackend())


def run_all(E, sc, shift=0):
    for influence in O.INFLUENCES:
        for mode in O.MODES:
            ref = O.reference(sc, influence, mode)
            O.check_forward(E, sc, influence, mode, ref, shift)
            if shift:
                rc, _, _ = E.gather(sc, influence, mode, O.tables(sc.idx, sc.n0, sc.seed)["index order"], shift=shift)
                assert rc == O.ERR_UNSUPPORTED, rc
                continue
            O.check_scatter(E, sc, influence, mode, ref)
            for form, table in O.tables(sc.idx, sc.n0, sc.seed).items():
                O.check_gather(E, sc, influence, mode, ref, table, form)


@pytest.mark.parametrize("n,n0,K,C,KP", O.EDGE)
def test_oracle_against_the_host_emulated_entries(entries, n, n0, K, C, KP):
    run_all(entries, O.case(n, n0, K, C, KP)[0])


def test_unaligned_rows_and_the_scene_at_the_origin(entries):
    run_all(entries, O.case(*O.UNALIGNED)[0], shift=1)
    run_all(entries, O.case(*O.AT_THE_ORIGIN, translated=False)[0])


@pytest.mark.parametrize("influence", O.INFLUENCES)
@pytest.mark.parametrize("mode", O.MODES)
def test_oracle_against_the_older_restatement(influence, mode):
    """the fp32 forward restatement within 1e-5 of the largest entry (its own rounding: sums of K KP <= 240 products), its float64 gradients (returned as
    fp32) within 1e-6.  Feature row 0 is inf in the scene and listed by nobody: neither restatement touches it."""
    sc = O.case(50, 80, 16, 64, 15)[0]
    out, gf, gkw = O.reference(sc, influence, mode)
    old = LA.kpconv(sc.q, sc.s, sc.idx, sc.f, sc.kpts, sc.kw, sc.extent, influence, mode)
    assert np.abs(old - out).max() <= 1e-5 * np.abs(out).max()
    ogf, ogkw = LA.kpconv_grads(sc.q, sc.s, sc.idx, sc.f, sc.kpts, sc.kw, sc.extent, sc.go, influence, mode)
    assert np.abs(ogf - gf).max() <= 1e-6 * np.abs(gf).max() and np.abs(ogkw - gkw).max() <= 1e-6 * np.abs(gkw).max()


def test_transposed_tables_hold_their_special_rows():
    sc = O.case(50, 80, 17, 64, 15)[0]
    flat = sc.idx.reshape(-1)
    for order, inv_start, inv_src in O.tables(sc.idx, sc.n0, 1).values():
        assert inv_start.dtype == inv_src.dtype == np.int32 and inv_start[-1] == inv_src.size == int((flat < sc.n0).sum())
        for r in range(sc.n0):
            j = r if order is None else order[r]
            assert list(inv_src[inv_start[r]:inv_start[r + 1]]) == list(np.flatnonzero(flat == j))
        at = {int(j if order is None else np.flatnonzero(order == j)[0]): j for j in (O.POISON, O.HUB, sc.n0 - 1)}
        deg = {j: int(inv_start[r + 1] - inv_start[r]) for r, j in at.items()}
        assert deg == {O.POISON: 0, O.HUB: O.HUB_PAIRS, sc.n0 - 1: 0}


def test_scene_conditions_at_the_device_shapes():
    """the generator asserts its conditions itself (flip-free, both sides of the clamp, the special rows): run it for the shapes only the device file uses.
    The four CAPS scenes differ in K and KP, so each has a geometry of its own."""
    for n, n0, K, C, KP, _, _ in O.CAPS:
        sc = O.case(n, n0, K, C, KP)[0]
        assert sc.hub and sc.rounds <= 8 and sc.moved <= 0.05 * n0
