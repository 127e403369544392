"""CPU: tests/pospool_oracle.py — the float64 oracle of PosPool, its scene generator and the driver that tests/test_gpu_pospool_oracle.py runs on the device —
on the host-emulated kernels (the build of pospool.hip that tests/test_local_aggregation_host.py makes, unchanged): every EDGE scene in the three reductions
through the forward, the scatter and the gather entry over the numpy-built tables, the unaligned scene, the twins without padding, the empty support set and the
refusals, so that a slip in the oracle, in a scene or in a call shows up without a GPU.  The emulation evaluates v_sin_f32 with the library sine: what the
instruction itself adds is measured on the device alone (profiles/pospool_oracle_device.md).  The oracle is held against the older fp32 restatement
(oracle/local_aggregation_oracle.py), its written-out gradient against finite differences of its own forward, and the scene conditions are asserted for the
device file's large shapes as well."""
import copy

import numpy as np
import pytest

from oracle import local_aggregation_oracle as LA
from tests import pospool_oracle as O
from tests.test_local_aggregation_host import host  # noqa: F401  (the fixture that builds and loads the host library)


@pytest.fixture(scope="module")
def entries(host):  # noqa: F811
    return O.Entries(host, O.HostBackend())


def run_all(E, sc, reductions=O.REDUCTIONS):
    for reduction in reductions:
        O.check_forward(E, sc, reduction)
        O.check_scatter(E, sc, reduction)
        first = None
        for form, table in O.tables(sc.idx, sc.n0, sc.seed).items():
            r = O.check_gather(E, sc, reduction, table, form, same_bits=first)
            first = r[1] if r else None


@pytest.mark.parametrize("n,n0,K,C,pe", O.EDGE)
def test_oracle_against_the_host_emulated_entries(entries, n, n0, K, C, pe):
    run_all(entries, O.case(n, n0, K, C, pe))


def test_the_scene_at_the_origin_and_the_twins_without_padding(entries):
    run_all(entries, O.case(*O.AT_THE_ORIGIN, translated=False))
    for shape in O.NO_PADDING:
        sc = O.case(*shape, padded=False, reductions=("mean",))
        run_all(entries, sc, ("mean",))
        big = np.abs(sc.ref["mean"][0]).max(1)
        assert big[sc.shadow_row] > 1e4 * np.median(big), "the row made of padding_num alone is not divided by 1e-5"


def test_unaligned_rows(entries):
    """the forward through the scalar kernel; the gather refuses shifted gradients (asserted by O.check_gather at every scene, here at this one)"""
    sc = O.case(*O.UNALIGNED)
    for reduction in O.REDUCTIONS:
        O.check_forward(entries, sc, reduction, shift=1)
    rc, _ = entries.gather(sc, sc.pe, "mean", O.tables(sc.idx, sc.n0, sc.seed)["index order"], shift=1)
    assert rc == O.ERR_BAD_ARG, rc


def test_refusals_max_ties_and_the_empty_support_set(entries):
    O.check_refusals(entries)
    O.check_empty_support(entries)
    for shape in ((40, 60, 17, 72, "sin_cos"), (39, 58, 20, 64, "exp_-d"), (120, 48, 3, 12, "xyz")):
        O.check_max_ties(entries, O.case(*shape))


@pytest.mark.parametrize("n,n0,K,C,pe", [s for s in O.EDGE if s[3] <= 144])
@pytest.mark.parametrize("reduction", O.REDUCTIONS)
def test_oracle_against_the_older_restatement(n, n0, K, C, pe, reduction):
    """the fp32 forward restatement at the tolerance the suite holds the kernels to against it (rtol 1e-4, atol 1e-4 max|ref|), its float64-accumulated
    gradient likewise.  The inf feature rows are listed by nobody, but the older restatement gathers by multiplication-free indexing too: neither touches them.
    Its 'max' gradient decides ties on fp32 products: the scenes are flip-free, so both share alike."""
    sc = O.case(n, n0, K, C, pe)
    out, gf = sc.ref[reduction]
    old, _, _ = LA.pospool(sc.q, sc.s, sc.idx, sc.f, sc.radius, pe, reduction)
    np.testing.assert_allclose(old, out, rtol=1e-4, atol=1e-4 * np.abs(out).max())
    f = sc.f.copy()
    f[[O.POISON, sc.n0 - 1]] = 0.0                                    # the older gradient multiplies a zero selection with every gathered value
    ogf = LA.pospool_grad_features(sc.q, sc.s, sc.idx, f, sc.radius, sc.go, pe, reduction)
    np.testing.assert_allclose(ogf, gf, rtol=1e-4, atol=1e-4 * np.abs(gf).max())


@pytest.mark.parametrize("reduction", O.REDUCTIONS)
@pytest.mark.parametrize("n,n0,K,C,pe", [(40, 60, 17, 72, "sin_cos"), (45, 52, 9, 18, "direction_exp_-d"), (37, 50, 26, 9, "three_order")])
def test_gradient_against_finite_differences(n, n0, K, C, pe, reduction):
    """sum(grad_features * D) against the central difference of L(f) = sum(out * go) along a random direction D, in float64.  The forward is linear in f for
    'sum' / 'mean' and piecewise linear for 'max': away from a tie the difference is exact up to rounding; at a tie (the planted zeros, the repeated row) L has
    no derivative, so grad_out is zeroed on the tied (p, c) — the shares there are asserted by O.check_max_ties."""
    base = O.case(n, n0, K, C, pe)
    sc = copy.copy(base)
    rng = np.random.default_rng(7)
    sc.f = base.f.astype(np.float64)
    sc.f[[O.POISON, n0 - 1]] = 0.0
    if reduction == "max":
        tied = O.max_figures(base, pe)[1]
        sc.go = np.where(tied, np.float32(0), base.go)
    D = rng.normal(size=sc.f.shape)
    _, gf = O.reference(sc, pe, reduction)
    h = 1e-6

    def loss(f):
        moved = copy.copy(sc)
        moved.f = f
        return float((O.reference(moved, pe, reduction)[0] * sc.go.astype(np.float64)).sum())

    fd = (loss(sc.f + h * D) - loss(sc.f - h * D)) / (2 * h)
    want = float((gf * D).sum())
    assert abs(fd - want) <= 1e-7 * np.abs(gf * D).sum(), (fd, want)


@pytest.mark.parametrize("n,n0,K,C,pe,reduction", [c for c in O.CAPS if c[0] < 100000])
def test_past_the_grid_caps_on_the_host(entries, n, n0, K, C, pe, reduction):
    """the emulation launches the capped grids as they are, so the second trips run here too (all but the 1048583-point scene, which takes it most of a minute)"""
    run_all(entries, O.case(n, n0, K, C, pe, reductions=(reduction,)), (reduction,))


def test_scene_conditions_at_the_device_shapes():
    """the generator asserts its conditions itself (the special rows, flip-free, the rounded-input share): run it for the shapes only the device file uses.
    The host-emulated kernels run every grid in full, second trips included, so the smallest of them go through the driver here as well."""
    for n, n0, K, C, pe, reduction in O.CAPS:
        sc = O.case(n, n0, K, C, pe, reductions=(reduction,))
        assert sc.redrawn < 0.01 and max(sc.share[reduction]) <= O.ROUNDING_SHARE
