"""CPU: the builder of the host-emulation libraries (tests/host_emul/host_build.py) — the dependencies it derives hold the headers the hand-written lists of
the test files used to miss, its stale check, and the size_t results of a loaded library."""
import ctypes
import glob
import os
import subprocess

from tests.host_emul import host_build as B
from tests.test_index_pool_host import host  # noqa: F401  (the fixture: the smallest library with workspace entries)


def test_dependencies_are_derived_from_the_tree():
    rel = lambda files: {os.path.relpath(d, B.ROOT) for d in B.dependencies(files)}
    kp = rel(["kpconv_backward"])
    assert {"contrastboundary_amd/csrc/kpconv_backward.hip", "contrastboundary_amd/csrc/wave_ops.h", "contrastboundary_amd/csrc/cbl_common.h", "include/cbl_amd.h",
            "tests/host_emul/host_tu.py", "tests/host_emul/host_build.py"} <= kp
    knn = rel(["knn_grid"])
    assert {"contrastboundary_amd/csrc/knn_wave.h", "tests/host_emul/wave/knn_wave.h"} <= knn
    assert any(d.startswith("tests/host_emul/wave/rocprim/") for d in knn)
    assert "contrastboundary_amd/csrc/kpconv_backward.hip" not in knn
    assert all(os.path.isfile(os.path.join(B.ROOT, d)) for d in kp | knn)


def test_stale(tmp_path):
    target, old, new = [str(tmp_path / n) for n in ("target", "old", "new")]
    for path, t in ((old, 1000), (new, 3000)):
        open(path, "w").close()
        os.utime(path, (t, t))
    assert B.stale(target, [old])                                        # missing
    open(target, "w").close()
    os.utime(target, (2000, 2000))
    assert B.stale(target, [old, new])                                   # older than one of them
    assert not B.stale(target, [old])
    os.utime(target, (3000, 3000))
    assert not B.stale(target, [old, new])                               # as new as the newest: the comparison the test files always made


def test_size_t_results_of_a_loaded_library(host):
    so = host._name
    assert so == os.path.join(B.BUILD, "libindex_pool.so")
    symbols = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout.split()
    exported = [n for n in symbols if n.endswith("_bytes")]
    assert {"cbl_ind_max_pool_backward_workspace_bytes", "cbl_neighbor_transpose_workspace_bytes", "cbl_adaptive_weight_backward_csr_workspace_bytes"} <= set(exported)
    assert all(getattr(host, n).restype is ctypes.c_size_t for n in exported)
    assert host.cbl_ind_max_pool.restype is ctypes.c_int                 # nothing else is touched
    assert not glob.glob(so + "*.tmp")
