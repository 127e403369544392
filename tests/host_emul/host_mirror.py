"""TEST INFRASTRUCTURE: the package's Python mirrors (autograd functions and modules) run on CPU tensors over the WHOLE library compiled for the host
(tests/host_emul/full_library.py), so that a composition of entries — convnet_blocks.LocalAggregation, the ResNet blocks, the backbone — is driven on a machine
without the device exactly as the device test drives it.  Inside `mirror()`:
  - contrastboundary_amd._lib.lib() returns the host library, _lib.stream_of() the null stream (a host launch is synchronous);
  - the argument checks of unary.py and local_aggregation.py accept CPU tensors (everything else they check stays);
  - pointops.spatial_order() gives no order (the rows as they are: same values), pointops.neighbor_transpose() the transposed table restated in numpy
    (host_build.transposed_table, no order array: the entries take NULL).
Nothing of this is product code and nothing outside tests/ imports it.  `pyramid()` is cbl_pyramid on the host, cut as tf_ops.segmentation_inputs_radius cuts."""
import contextlib
import ctypes

import numpy as np
import torch

from tests.host_emul import full_library
from tests.host_emul.host_build import size_t_results, transposed_table


def library():
    return size_t_results(full_library.load())


def _ptrs(arrs, count):
    a = (ctypes.c_void_p * count)()
    for i, x in enumerate(arrs):
        a[i] = x.ctypes.data
    return a


def pyramid(points, dl0, density, layers, limits):
    """-> dict(points, neighbors, pools) of numpy arrays: one cloud through cbl_pyramid (tf_ops._segmentation_inputs_radius_native's call and cuts)"""
    L = library()
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    xyz = np.ascontiguousarray(points, np.float32)
    n, b = xyz.shape[0], 1
    lens = np.array([n], np.int32)
    lims = np.int32([int(limits[l]) for l in range(layers)])
    gbytes = L.cbl_radius_neighbors_workspace_bytes(b, n)
    grids = [np.zeros(gbytes + 64, np.uint8) for _ in range(layers)]
    nb = [np.full((n, int(lims[l])), -5, np.int32) for l in range(layers)]
    pp = [np.full((n, 3), np.nan, np.float32) for _ in range(layers - 1)]
    pl = [np.full(b, -1, np.int32) for _ in range(layers - 1)]
    po = [np.full((n, int(lims[l])), -5, np.int32) for l in range(layers - 1)]
    up = [np.full((n, int(lims[l])), -5, np.int32) for l in range(layers - 1)]
    mx, sizes = np.full(3 * layers, -1, np.int32), np.full(layers, -1, np.int32)
    nbytes = L.cbl_pyramid_layer_workspace_bytes(b, n)
    ws = np.zeros(nbytes + 64, np.uint8)
    rc = L.cbl_pyramid(b, n, P(xyz), P(lens), ctypes.c_float(dl0 * density / 2.0), ctypes.c_float(dl0), layers, P(lims), _ptrs(grids, layers), ctypes.c_size_t(gbytes),
                       _ptrs(nb, layers), _ptrs(pp, layers), _ptrs(pl, layers), _ptrs(po, layers), _ptrs(up, layers), P(mx), P(sizes), P(ws), ctypes.c_size_t(nbytes), None)
    assert rc == 0, rc
    cut = lambda t, rows, w: np.ascontiguousarray(t[:rows, :min(int(w), t.shape[1])])
    return dict(points=[xyz] + [np.ascontiguousarray(pp[l][:sizes[l + 1]]) for l in range(layers - 1)],
                neighbors=[cut(nb[l], sizes[l], mx[3 * l]) for l in range(layers)],
                pools=[cut(po[l], sizes[l + 1], mx[3 * l + 1]) for l in range(layers - 1)] + [np.zeros((0, 1), np.int32)])


def _chk_unary(t, name):
    if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.is_contiguous()):
        raise TypeError(f"{name}: expected a contiguous tensor of torch.float32")
    return t


def _chk_la(t, dtype, name):
    if not (isinstance(t, torch.Tensor) and t.dtype == dtype and t.is_contiguous()):
        raise TypeError(f"{name}: expected a contiguous tensor of {dtype}")
    return t


def _neighbor_transpose(idx, n0, build=True, **_):
    inv_start, inv_src = transposed_table(idx.numpy(), int(n0))
    return None, torch.from_numpy(inv_start), torch.from_numpy(inv_src)


@contextlib.contextmanager
def mirror():
    from contrastboundary_amd import _lib, local_aggregation, pointops, unary
    saved = [(_lib, "_lib", _lib._lib), (_lib, "stream_of", _lib.stream_of), (unary, "_chk", unary._chk), (local_aggregation, "_chk", local_aggregation._chk),
             (pointops, "spatial_order", pointops.spatial_order), (pointops, "neighbor_transpose", pointops.neighbor_transpose)]
    try:
        _lib._lib = library()
        _lib.stream_of = lambda t: ctypes.c_void_p(0)
        unary._chk, local_aggregation._chk = _chk_unary, _chk_la
        pointops.spatial_order = lambda points: None
        pointops.neighbor_transpose = _neighbor_transpose
        yield
    finally:
        for obj, name, value in saved:
            setattr(obj, name, value)
