"""GPU: the round-5 regression inputs of the contrast kernels and a bounded, seeded share of the randomized campaign (tests/host_emul/fuzz_cases.py), presented to
the DEVICE library (contrastboundary_amd/lib/libcbl_amd.so, through its C ABI) and compared with the oracles (oracle/cbl_oracle.py, oracle/_build/liboracle.so) —
the same case generators and assertions the host-emulated suites run, with one difference: every numpy argument travels to HBM for the call and back after it.

Reference behaviour these hold: /root/reference/tensorflow/models/heads/head.py:749-760 (max-shifted exponentials, the margin's separate negatives' sum),
/root/reference/pytorch/model/heads.py:145-246 (pair mining), lib/pointops/src/knnquery/knnquery_cuda_kernel.cu:65-111 (tie order), sampling_cuda_kernel.cu:14-129,
tensorflow/ops/cpp_wrappers/cpp_neighbors/neighbors/neighbors.cpp:213-336, cpp_subsampling/grid_subsampling/grid_subsampling.cpp."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


class Arg:
    """a numpy argument of a C-ABI call: uploaded before the call, downloaded after it"""
    __slots__ = ("a",)

    def __init__(self, a):
        self.a = a


def wrap(a):
    return None if a is None else Arg(a)


class DeviceLib:
    """libcbl_amd.so with numpy in place of device pointers: `lib.cbl_x(n, P(xyz), ...)` copies every P(...) array to the device (one buffer per distinct array, so
    aliased arguments stay aliased), calls the entry on the null stream, waits, and copies every buffer back into its array (outputs and untouched inputs alike)"""

    def __init__(self):
        import torch
        from contrastboundary_amd import _lib
        self._torch, self._lib = torch, _lib.lib()

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name.endswith("_bytes"):
            return fn
        torch = self._torch

        def call(*args):
            bufs, out = {}, []
            for x in args:
                if isinstance(x, Arg):
                    key = (x.a.__array_interface__["data"][0], x.a.nbytes)
                    if key not in bufs:
                        host = np.ascontiguousarray(x.a).reshape(-1).view(np.uint8)
                        bufs[key] = (x.a, torch.from_numpy(host.copy()).cuda() if host.size else torch.empty(16, dtype=torch.uint8, device="cuda"))
                    out.append(ctypes.c_void_p(bufs[key][1].data_ptr()))
                else:
                    out.append(x)
            rc = fn(*out)
            torch.cuda.synchronize()
            for a, t in bufs.values():
                if a.size:
                    assert a.flags["C_CONTIGUOUS"] and a.flags["WRITEABLE"]
                    a.reshape(-1).view(np.uint8)[:] = t.cpu().numpy()
            return rc
        return call


@pytest.fixture(scope="module")
def dev():
    return DeviceLib()


@pytest.fixture()
def cbl_cases(monkeypatch):
    import tests.test_cbl_host as T
    monkeypatch.setattr(T, "P", wrap)
    return T


# ---- the two defects the round-5 campaign found (fixed in commit 301ff19): both inputs on the device, against the oracle ------------------------------------------
def test_gradient_stays_finite_when_every_valid_neighbour_is_far_behind_a_masked_one(dev, cbl_cases):
    cbl_cases.test_gradient_stays_finite_when_every_valid_neighbour_is_far_behind_a_masked_one(dev)


def test_negatives_far_below_the_positives_keep_their_sum(dev, cbl_cases):
    cbl_cases.test_negatives_far_below_the_positives_keep_their_sum(dev)


@pytest.mark.parametrize("nsample,d,nce", [(8, 16, 0), (17, 32, 0), (33, 4, 0), (36, 32, 0), (40, 64, 0), (65, 8, 0), (17, 32, 1)])
def test_point_contrast_every_row_width(dev, cbl_cases, nsample, d, nce):
    cbl_cases.test_point_contrast(dev, nsample, d, nce)


# ---- a seeded share of the campaign ----------------------------------------------------------------------------------------------------------------------------
FAMILIES = [("knn", 205, 6), ("knn", 305, 6), ("knn", 405, 6), ("radius", 102, 25), ("radius", 202, 25), ("grid", 103, 60), ("subsample", 110, 60), ("fps", 104, 4), ("fps", 204, 4),
            ("transpose", 105, 20), ("transpose", 205, 20), ("cbl", 106, 80), ("cbl", 206, 80), ("cbl", 306, 80), ("cbl", 406, 80), ("cbl", 506, 80), ("cbl", 606, 80),
            ("gather", 107, 60), ("gather", 207, 60), ("gather", 307, 60), ("aggregation", 108, 30), ("aggregation", 208, 30), ("aggregation", 308, 30)]


@pytest.mark.parametrize("which,seed,cases", FAMILIES)
def test_random_cases_equal_the_oracles_on_the_device(dev, monkeypatch, which, seed, cases):
    from tests.host_emul import fuzz_cases as Z
    import tests.test_local_aggregation_host as A
    import tests.test_pointops_gather_host as G
    for mod in (Z, G, A):
        monkeypatch.setattr(mod, "P", wrap)
    monkeypatch.setattr(Z, "lib", lambda: dev)
    assert Z.run(which, seed, cases) == 0
