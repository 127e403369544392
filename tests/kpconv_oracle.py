"""TEST ORACLE: KPConv (PseudoGrid, the reference's tensorflow/models/local_aggregation_operators.py:681-728) restated in float64 numpy from the float32
inputs — the output and, for a given grad_out, d / d features and d / d kernel_weights — the scenes it is tested on, and the one driver that calls the four C
entries (cbl_kpconv_forward, cbl_kpconv_forward_ordered, cbl_kpconv_backward, cbl_kpconv_backward_csr) through ctypes on the buffers of a backend (host arrays
in tests/test_kpconv_oracle_host.py, device tensors in tests/test_gpu_kpconv_oracle.py), so both run the same calls against the same oracle.
    out[i, c] = sum_kp kw[kp, c] * sum_k w[i, kp, k] * f[idx[i, k], c]          w = 1 ('constant') or max(1 - |s[idx] - q - kpts| / extent, 0) ('linear'),
    in 'closest' mode kept only at the nearest kernel point of the neighbour (first minimum, :705-708); the shadow index n0 is a point at 1e6 with a zero row.

A scene (`case`) is one blob a few extents wide, translated far from the origin, in which every support is a plausible neighbour of every query, so the
neighbour table is drawn, not searched.  Its conditions are asserted here on the float64 quantities alone:
    * flip-free: for every real pair the squared distances to the nearest and the second-nearest kernel point differ by at least 1e-4 extent^2 (offsets are at
      most ~3 extents, a squared distance at most ~9 extent^2, a few fp32 ulp of it ~3e-6 extent^2: the margin is over 30 times that); supports that offend
      are moved.  ONE pair is exempt on purpose: its neighbour lies on the mirror plane of the last two kernel points, which are mirror images, at coordinates
      where the two distances are EQUAL in fp32 and in float64, and no other kernel point is as near — the first-minimum rule decides it.
    * weights on both sides of the clamp: in 'linear' mode at least half of the real pairs have a non-zero weight at some kernel point, at least 5 % at none.
    * translation by OFFSET (one scene is also built without it).
    * trailing shadow indices on a fifth of the rows, one row all shadow, one row that lists one support K times, a support nobody lists (n0 - 1), a hub listed
      by HUB_PAIRS = 131 pairs (three 64-pair chunks of the gather; left out where the table has under 2 * 131 free pairs), and feature row 0 = inf, listed by
      nobody: the kernels' clamped loads of shadow neighbours read it, and a 0 * inf leak is a NaN in an output that must be finite.
`close` holds EVERY entry of an array to 1e-4 of the largest reference entry (README: floats within 1e-4) and excludes nothing."""
import ctypes
import functools

import numpy as np

from tests.attention_oracle import HostBackend  # noqa: F401  (the host buffers of the driver; the device file brings its own backend)
from tests.host_emul.host_build import size_t_results

EXTENT = 0.09375                                                       # 3 / 32: the same number in fp32 and float64
OFFSET = (37.5, -12.25, 81.0)
POISON, TIE, HUB, REPEATED = 0, 1, 2, 3                                # support rows with a part to play; random draws start at FIRST_FREE
FIRST_FREE = 4
HUB_PAIRS = 131
MARGIN = 1e-4                                                          # of extent^2
FAR_SHARE = 0.12
OK, ERR_BAD_ARG, ERR_UNSUPPORTED = 0, -1, -3                           # include/cbl_amd.h
INFLUENCES, MODES = ("constant", "linear"), ("sum", "closest")
CHUNK = 2048                                                           # query points per float64 block: (CHUNK, K, C) stays under 100 MB at the largest scene

_i, _f, _z = ctypes.c_int, ctypes.c_float, ctypes.c_size_t

# The shapes (n, n0, K, C, KP), and per shape the kernels they take.  Forward (csrc/local_aggregation.hip): kpconv_fwd_c64_kernel<CLOSEST, LINEAR, ONE> where
# C % 4 == 0, C <= 64 and features / out / kernel_weights are 16-byte aligned (ONE: K <= 16) — eight instances, all four (influence, mode) combinations of every
# such shape; kpconv_fwd_kernel<true> where C % 4 == 0 and C > 64; kpconv_fwd_kernel<false> where C % 4 != 0 or the rows are not aligned.  Backward: the scatter
# kernel kpconv_bwd_kernel at K <= 64 (BAD_ARG above), the gather kpconv_bwd_csr_kernel<GF, GKW, CLOSEST> (csrc/kpconv_backward.hip) at C % 4 == 0 and aligned
# rows (UNSUPPORTED otherwise) — six instances: the two modes times the three gradient selections of check_gather.
EDGE = [(41, 57, 1, 4, 1),        # c64 ONE: K = 1, one channel quad, one kernel point (no argmin partner, no tie pair)
        (50, 80, 16, 64, 15),     # c64 ONE at its boundary K = 16: the bench configuration, with shadows
        (50, 80, 17, 64, 15),     # c64 !ONE: one neighbour in the second 16-chunk
        (33, 60, 64, 32, 16),     # c64 !ONE: K = 64 (the scatter entry's largest), KP = 16: no masked accumulator row
        (29, 90, 65, 48, 13),     # c64 !ONE: the second 64-neighbour chunk (ids and coordinates reloaded); scatter refuses, gather at K > 64
        (27, 200, 130, 72, 7),    # generic float4 kernel (C > 64): three 64-chunks, two channel chunks; scatter refuses
        (31, 70, 26, 68, 15),     # generic float4 kernel: the second channel chunk has one live lane quad
        (23, 64, 31, 144, 15),    # generic float4 kernel at the ConvNet's width: three channel chunks
        (37, 50, 9, 6, 15),       # C % 4 != 0: scalar forward kernel, scatter backward; the gather entry refuses
        (25, 40, 20, 67, 5)]      # C % 4 != 0 over two channel chunks
UNALIGNED = (40, 60, 16, 64, 15)  # features / out one float past a 16-byte boundary: leaves the c64 kernel for the scalar one; forward only, the gather refuses
AT_THE_ORIGIN = (50, 80, 17, 64, 15)                                   # the one EDGE scene that is also run untranslated
# CAPS: past the hard caps in the sources, whatever occupancy the runtime reports.  Forward grid <= 2048 workgroups x 4 points = 8192 points per trip: the
# three-deep pipeline of the c64 kernel needs four trips, n = 24611 > 3 x 8192 (no multiple of 32: the XCD dealing leaves holes).  Gather grid <= KB_MAX_GRID =
# 2048 workgroups x 4 targets: the two-ahead prefetch needs three trips, n0 = 16501 > 2 x 8192.  (n, n0, K, C, KP, influence, mode):
CAPS = [(24611, 16501, 9, 32, 15, "constant", "closest"),             # c64 <true, false, true>; gather CLOSEST
        (24611, 16501, 20, 64, 13, "linear", "sum"),                  # c64 <false, true, false>
        (24611, 16501, 26, 72, 15, "linear", "sum"),                  # generic float4 kernel
        (24611, 16501, 16, 64, 15, "linear", "closest")]              # c64 <true, true, true>; gather CLOSEST at the bench width


# ---------------------------------------------------------------------------------------------------------------- float64
def _weights(q, s, idx, kpts, rows):
    """float64, for the query rows `rows` (a slice): real (m, K) bool, sq (m, K, KP) squared distances neighbour - centre - kernel point (shadow: from 1e6)"""
    n0 = s.shape[0]
    ids = idx[rows]
    real = (ids >= 0) & (ids < n0)
    nb = np.where(real[..., None], s[np.where(real, ids, 0)].astype(np.float64), 1e6) - q[rows].astype(np.float64)[:, None, :]
    diff = nb[:, :, None, :] - kpts.astype(np.float64)[None, None]
    return real, (diff * diff).sum(-1)


def _influence(sq, extent, influence, mode):
    """(m, K, KP) float64 weights"""
    w = np.ones_like(sq) if influence == "constant" else np.maximum(1.0 - np.sqrt(sq) / float(extent), 0.0)
    if mode == "closest":
        w = w * np.eye(sq.shape[-1])[sq.argmin(-1)]                    # np.argmin: the first minimum
    return w


def reference(sc, influence, mode):
    """-> out (n, C), grad_features (n0, C), grad_kernel_weights (KP, C) in float64, the gradients under the loss sum(out * sc.go)"""
    assert influence in INFLUENCES and mode in MODES
    n, n0, C = sc.n, sc.n0, sc.C
    f, kw, go = sc.f.astype(np.float64), sc.kw.astype(np.float64), sc.go.astype(np.float64)
    out, gf, gkw = np.zeros((n, C)), np.zeros((n0, C)), np.zeros_like(kw)
    for a in range(0, n, CHUNK):
        rows = slice(a, min(a + CHUNK, n))
        real, sq = _weights(sc.q, sc.s, sc.idx, sc.kpts, rows)
        w = _influence(sq, sc.extent, influence, mode)                # (m, K, KP)
        ids = np.where(real, sc.idx[rows], 0)
        nf = np.where(real[..., None], f[ids], 0.0)                   # the shadow row is zeros (:713); a select, never a product with what row 0 holds
        wf = np.matmul(w.transpose(0, 2, 1), nf)                      # (m, KP, C)  :716
        out[rows] = (kw[None] * wf).sum(1)                            # :723-727
        gkw += np.einsum("mc,mpc->pc", go[rows], wf)
        g_nf = np.matmul(w, kw) * go[rows][:, None, :]                # (m, K, C)
        t = ids[real]
        o = np.argsort(t, kind="stable")
        ts = t[o]
        first = np.flatnonzero(np.r_[True, ts[1:] != ts[:-1]])
        if ts.size:
            gf[ts[first]] += np.add.reduceat(g_nf[real][o], first, axis=0)
    return out, gf, gkw


def pair_figures(sc):
    """float64, per pair (n, K): real; gap = second smallest - smallest squared distance to a kernel point (inf at KP = 1); touched = some 'linear' weight
    is non-zero"""
    real, gap, touched = [], [], []
    for a in range(0, sc.n, CHUNK):
        r, sq = _weights(sc.q, sc.s, sc.idx, sc.kpts, slice(a, min(a + CHUNK, sc.n)))
        two = np.sort(sq, -1)[..., :2]
        real.append(r)
        gap.append(two[..., 1] - two[..., 0] if sq.shape[-1] > 1 else np.full(r.shape, np.inf))
        touched.append(np.sqrt(two[..., 0]) < float(sc.extent))
    return np.concatenate(real), np.concatenate(gap), np.concatenate(touched)


# ---------------------------------------------------------------------------------------------------------------- scenes
class Scene:
    """float32 / int32 inputs of one shape: q (n, 3), s (n0, 3), idx (n, K), f (n0, C), kpts (KP, 3), kw (KP, C), go (n, C), extent; and what the generator
    placed: rep_row, shadow_row, tie (row, column) or None, hub (bool), moved (supports the flip-free pass moved), rounds"""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self.tag = "(%d, %d, %d, %d, %d)%s" % (self.n, self.n0, self.K, self.C, self.KP, "" if self.translated else " at the origin")


def _unit(rng, m):
    v = rng.normal(size=(m, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _kernel_points(rng, KP, E):
    """kpts[0] = 0; the others at 0.5 .. 1 extents from it; from KP = 3 the last two are mirror images in x, and no other kernel point is within half an
    extent of the point (0, E/2, -E/4) on their mirror plane, which is E/4 from both"""
    k = np.zeros((KP, 3))
    tie_at = np.array([0.0, E / 2, -E / 4])
    for j in range(1, KP):
        while True:
            k[j] = _unit(rng, 1)[0] * rng.uniform(0.5 * E, E)
            if KP < 3 or np.linalg.norm(k[j] - tie_at) > 0.5 * E:
                break
    if KP >= 3:
        k[KP - 2] = (E / 4, E / 2, -E / 4)
        k[KP - 1] = (-E / 4, E / 2, -E / 4)
    return k.astype(np.float32), tie_at


def transposed(idx, n0, order=None):
    """the transposed table in numpy (independent of neighbor_transpose.hip): segment r of inv_src lists, ascending, the flat pairs p = i * K + k with
    idx[p] == (order[r] if an order is given else r); shadow neighbours (== n0) are in no list.  -> inv_start (n0 + 1), inv_src, int32"""
    flat = idx.reshape(-1)
    keep = np.flatnonzero((flat >= 0) & (flat < n0))
    by_target = keep[np.argsort(flat[keep], kind="stable")].astype(np.int32)
    deg = np.bincount(flat[keep], minlength=n0)
    first = np.concatenate([[0], np.cumsum(deg)])
    if order is None:
        return first.astype(np.int32), by_target
    inv_start = np.concatenate([[0], np.cumsum(deg[order])]).astype(np.int32)
    inv_src = np.concatenate([by_target[first[j]:first[j + 1]] for j in order]).astype(np.int32)
    return inv_start, inv_src


def tables(idx, n0, seed):
    """the gather entry's tables built in numpy: targets in index order (no order_dst), and in a random processing order; (order, inv_start, inv_src)"""
    order = np.random.default_rng(seed).permutation(n0).astype(np.int32)
    return {"index order": (None,) + transposed(idx, n0), "ordered": (order,) + transposed(idx, n0, order)}


@functools.lru_cache(maxsize=None)
def geometry(n, n0, K, C, KP, seed, translated=True):
    """the scene of a shape (the same for the four (influence, mode) combinations), every condition of the module's docstring asserted"""
    assert n >= 20 and n0 >= 16 and K >= 1 and 1 <= KP <= 16
    rng = np.random.default_rng(seed)
    E = EXTENT
    kpts, tie_at = _kernel_points(rng, KP, E)
    # queries within 0.35 extents of the blob's centre; near supports N(0, (0.45 E)^2) per axis, at most 1.9 extents out; far supports 2.4 .. 2.6 extents
    # out: at least 2.05 extents from every query, so beyond the extent of every kernel point (those are at most one extent from the query)
    ql = rng.normal(size=(n, 3)) * 0.1 * E
    ql *= np.minimum(1.0, 0.35 * E / np.linalg.norm(ql, axis=1))[:, None]
    sl = rng.normal(size=(n0, 3)) * 0.45 * E
    sl *= np.minimum(1.0, 1.9 * E / np.linalg.norm(sl, axis=1))[:, None]
    free_rows = np.arange(FIRST_FREE, n0 - 1)
    far = rng.choice(free_rows, max(1, int(round(FAR_SHARE * free_rows.size))), replace=False)
    sl[far] = _unit(rng, far.size) * rng.uniform(2.4 * E, 2.6 * E, (far.size, 1))
    near = np.setdiff1d(free_rows, far)
    sl[HUB], sl[REPEATED] = (0.3 * E, -0.2 * E, 0.25 * E), (-0.25 * E, 0.3 * E, 0.2 * E)      # both well inside the centre kernel point's extent
    shift = np.array(OFFSET if translated else (0.0, 0.0, 0.0))
    q, s = (ql + shift).astype(np.float32), (sl + shift).astype(np.float32)

    idx = near[rng.integers(0, near.size, (n, K))].astype(np.int32)
    padded = rng.choice(n, n // 5, replace=False)                     # trailing shadow neighbours, as the radius search pads
    for i, npad in zip(padded, rng.integers(1, max(1, K // 3) + 1, padded.size)):
        idx[i, K - npad:] = n0
    rep_row, shadow_row, tie = n // 3, n // 3 + 1, ((n // 2, 0) if KP >= 3 else None)
    idx[rep_row] = REPEATED
    idx[shadow_row] = n0
    if tie:
        idx[tie] = TIE
        s[TIE] = q[tie[0]] + tie_at.astype(np.float32)                # x: the query's own, bit for bit
    pos = np.arange(n * K)
    flat = idx.reshape(-1)
    free = pos[(flat < n0) & (pos // K != rep_row) & ((pos != tie[0] * K + tie[1]) if tie else True)]
    hub = free.size >= 2 * HUB_PAIRS
    if hub:
        at = rng.choice(free, HUB_PAIRS, replace=False)
        flat[at] = HUB
        free = np.setdiff1d(free, at)
    at = rng.choice(free, int(np.ceil(FAR_SHARE * free.size)), replace=False)
    flat[at] = far[rng.integers(0, far.size, at.size)]

    f = rng.normal(size=(n0, C)).astype(np.float32)
    f[POISON] = np.inf
    sc = Scene(n=n, n0=n0, K=K, C=C, KP=KP, seed=seed, translated=translated, extent=E, q=q, s=s, idx=np.ascontiguousarray(idx), f=f, kpts=kpts,
               kw=rng.normal(size=(KP, C)).astype(np.float32), go=rng.normal(size=(n, C)).astype(np.float32), rep_row=rep_row, shadow_row=shadow_row,
               tie=tie, hub=hub)

    # flip-free: move every support that a pair within the margin lists (the exempt pair's support is listed by that pair alone and stays)
    exempt = np.zeros((n, K), bool)
    if tie:
        exempt[tie] = True
    moved = np.zeros(n0, bool)
    for rounds in range(9):
        real, gap, touched = pair_figures(sc)
        bad = real & ~exempt & (gap < MARGIN * E * E)
        if not bad.any():
            break
        assert rounds < 8, "%s: still %d pairs within the margin after 8 rounds" % (sc.tag, int(bad.sum()))
        rows = np.unique(idx[bad])
        s[rows] += (rng.normal(size=(rows.size, 3)) * 0.01 * E).astype(np.float32)
        moved[rows] = True
    sc.moved, sc.rounds = int(moved.sum()), rounds

    # the conditions, on the float64 figures of the final scene
    count = np.bincount(idx.reshape(-1), minlength=n0 + 1)
    assert real.sum() == count[:n0].sum() and not real[shadow_row].any() and (idx[rep_row] == REPEATED).all()
    assert count[POISON] == 0 and count[n0 - 1] == 0 and count[TIE] == (1 if tie else 0) and not moved[TIE]
    assert (count[HUB] == HUB_PAIRS) if hub else (n * K < 4 * HUB_PAIRS), (sc.tag, int(count[HUB]))
    assert (np.diff((idx == n0).astype(int), axis=1) >= 0).all(), "shadow indices are not trailing"
    assert int((idx == n0).any(1).sum()) >= n // 5 - 2
    assert float(gap[real & ~exempt].min()) >= MARGIN * E * E
    if tie:
        _, sq = _weights(sc.q, sc.s, sc.idx, sc.kpts, slice(tie[0], tie[0] + 1))
        sq = sq[0, tie[1]]
        assert sq[KP - 2] == sq[KP - 1] and (np.delete(sq, [KP - 2, KP - 1]) >= sq[KP - 1] + MARGIN * E * E).all(), "the exact tie is not one in float64"
        d = sc.s[TIE] - sc.q[tie[0]] - sc.kpts[[KP - 2, KP - 1]]       # fp32, the kernels' own association
        sq32 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        assert d.dtype == np.float32 and sq32[0] == sq32[1], "the exact tie is not one in fp32"
    share_on, share_off = float(touched[real].mean()), float((~touched[real]).mean())
    assert share_on >= 0.5 and share_off >= 0.05, (sc.tag, share_on, share_off)
    print("scene %s: %d real pairs, %.0f %% with a non-zero linear weight, %d supports moved in %d rounds, hub %s" %
          (sc.tag, int(real.sum()), 100 * share_on, sc.moved, sc.rounds, hub))
    return sc


def case(n, n0, K, C, KP, influence="linear", mode="sum", seed=None, translated=True):
    """-> (scene, influence, mode): the inputs a shape is tested on (seed: n + n0 + K + C + KP unless given).  The geometry does not depend on the influence
    or the mode — every scene is flip-free, so it serves all four — and is built once per process."""
    assert influence in INFLUENCES and mode in MODES
    return geometry(n, n0, K, C, KP, n + n0 + K + C + KP if seed is None else seed, translated), influence, mode


# ---------------------------------------------------------------------------------------------------------------- the contract
def close(got, ref, tag):
    """the project's contract (README: floats within 1e-4): |got - ref| <= 1e-4 max|ref| for EVERY entry; prints and returns the worst
    |got - ref| / max|ref|"""
    ref, got = np.asarray(ref, np.float64), np.asarray(got, np.float64)
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    assert np.isfinite(ref).all(), tag
    scale = max(float(np.abs(ref).max()), 1e-30)
    ratio = float(np.abs(got - ref).max()) / scale if np.isfinite(got).all() else float("inf")
    print("%s: worst |got - ref| / max|ref| %.3e" % (tag, ratio))
    assert ratio <= 1e-4, "%s: an entry is off by %.3e of the largest reference entry (bound 1e-4)" % (tag, ratio)
    return ratio


# ---------------------------------------------------------------------------------------------------------------- the entries
class Entries:
    """the four KPConv entries on one backend.  Outputs are pre-filled with NaN (zeros for the scatter entry, which accumulates); the gather entry's workspace
    has exactly cbl_kpconv_backward_csr_workspace_bytes bytes.  Every call returns (status, numpy arrays...); an array is None where the entry was not given
    one.  `shift`: features and out (forward) / features (gather) start that many floats past an aligned address."""

    def __init__(self, lib, backend):
        self.L, self.B = lib, backend
        size_t_results(lib)

    def _inputs(self, sc, keys, shift=0):
        return {k: self.B.put(getattr(sc, k), shift if k == "f" else 0) for k in keys}

    @staticmethod
    def _cfg(sc, influence, mode):
        return _f(sc.extent), _i(INFLUENCES.index(influence)), _i(MODES.index(mode))

    def forward(self, sc, influence, mode, order=None, shift=0):
        """cbl_kpconv_forward, or cbl_kpconv_forward_ordered where an `order` (a permutation of the query points, int32) is given"""
        B, P = self.B, self.B.ptr
        d = self._inputs(sc, ("q", "s", "idx", "f", "kpts", "kw"), shift)
        out = B.put(np.full((sc.n, sc.C), np.nan, np.float32), shift)
        head = [_i(sc.n), _i(sc.n0), _i(sc.K), _i(sc.C), _i(sc.KP)] + [P(d[k]) for k in ("q", "s", "idx", "f", "kpts", "kw")] + list(self._cfg(sc, influence, mode))
        if order is None:
            rc = self.L.cbl_kpconv_forward(*head, P(out), B.stream)
        else:
            dorder = B.put(np.ascontiguousarray(order, np.int32))
            rc = self.L.cbl_kpconv_forward_ordered(*head, P(dorder), P(out), B.stream)
        return rc, B.get(out)

    def scatter(self, sc, influence, mode):
        """cbl_kpconv_backward -> status, grad_features, grad_kernel_weights"""
        B, P = self.B, self.B.ptr
        d = self._inputs(sc, ("q", "s", "idx", "f", "kpts", "kw", "go"))
        gf, gkw = B.fill((sc.n0, sc.C), 0.0), B.fill((sc.KP, sc.C), 0.0)
        rc = self.L.cbl_kpconv_backward(_i(sc.n), _i(sc.n0), _i(sc.K), _i(sc.C), _i(sc.KP), *[P(d[k]) for k in ("q", "s", "idx", "f", "kpts", "kw")],
                                        *self._cfg(sc, influence, mode), P(d["go"]), P(gf), P(gkw), B.stream)
        return rc, B.get(gf), B.get(gkw)

    def gather(self, sc, influence, mode, table, want_f=True, want_w=True, shift=0):
        """cbl_kpconv_backward_csr over `table` = (order_dst or None, inv_start, inv_src): numpy arrays, or buffers that are already the backend's"""
        B, P = self.B, self.B.ptr
        d = self._inputs(sc, ("q", "s", "f", "kpts", "kw", "go"), shift)
        tab = [B.put(t) if isinstance(t, np.ndarray) else t for t in table]
        nbytes = self.L.cbl_kpconv_backward_csr_workspace_bytes(_i(sc.n0), _i(sc.C), _i(sc.KP))
        ws = B.fill((nbytes,), 0, np.uint8)
        gf = B.fill((sc.n0, sc.C), np.nan) if want_f else None
        gkw = B.fill((sc.KP, sc.C), np.nan) if want_w else None
        rc = self.L.cbl_kpconv_backward_csr(_i(sc.n), _i(sc.n0), _i(sc.K), _i(sc.C), _i(sc.KP), *[P(d[k]) for k in ("q", "s", "f", "kpts", "kw")],
                                            *self._cfg(sc, influence, mode), P(d["go"]), *[P(t) for t in tab], P(gf), P(gkw), P(ws), _z(nbytes), B.stream)
        return rc, (B.get(gf) if want_f else None), (B.get(gkw) if want_w else None)


# ---------------------------------------------------------------------------------------------------------------- the checks
def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_forward(E, sc, influence, mode, ref, shift=0):
    """both forward entries against the oracle; a random processing order gives the unordered result bit for bit"""
    tag = "%s %s %s%s" % (sc.tag, influence, mode, ", rows shifted by one float" if shift else "")
    rc, out = E.forward(sc, influence, mode, shift=shift)
    assert rc == OK, (tag, rc)
    ratio = close(out, ref[0], tag + " forward")
    order = np.random.default_rng(sc.seed + 5).permutation(sc.n).astype(np.int32)
    rc, ordered = E.forward(sc, influence, mode, order=order, shift=shift)
    assert rc == OK, (tag, rc)
    close(ordered, ref[0], tag + " forward_ordered")
    assert np.array_equal(bits(ordered), bits(out)), tag + ": the ordered entry's bits differ from the unordered entry's"
    return ratio


def check_scatter(E, sc, influence, mode, ref):
    tag = "%s %s %s scatter" % (sc.tag, influence, mode)
    rc, gf, gkw = E.scatter(sc, influence, mode)
    if sc.K > 64:
        assert rc == ERR_BAD_ARG, (tag, rc)
        return None
    assert rc == OK, (tag, rc)
    return close(gf, ref[1], tag + " grad features"), close(gkw, ref[2], tag + " grad kernel_weights")


SELECTIONS = ((True, True), (True, False), (False, True))             # both gradients, the features' alone, the kernel weights' alone


def check_gather(E, sc, influence, mode, ref, table, form):
    """the three gradient selections over one table: values, exact zeros for the targets nobody lists, the same bits on a second run.  Where C % 4 != 0 the
    entry must refuse.  -> the ratios of the run with both gradients"""
    tag = "%s %s %s gather, %s" % (sc.tag, influence, mode, form)
    if sc.C % 4:
        rc, _, _ = E.gather(sc, influence, mode, table)
        assert rc == ERR_UNSUPPORTED, (tag, rc)
        return None
    first = ratios = None
    for want_f, want_w in SELECTIONS + (SELECTIONS[0],):
        rc, gf, gkw = E.gather(sc, influence, mode, table, want_f, want_w)
        assert rc == OK, (tag, rc)
        if first is not None and want_f and want_w:                  # the second run of the first selection
            assert np.array_equal(bits(gf), bits(first[0])) and np.array_equal(bits(gkw), bits(first[1])), tag + ": a second run gives other bits"
            break
        # every selection is a kernel instance of its own, with a grid of its own (the workgroups resident at once), so grad_kernel_weights is summed in
        # another order: each is held to the oracle, none to another's bits
        sel = "" if want_f and want_w else ", features alone" if want_f else ", kernel_weights alone"
        r = (close(gf, ref[1], tag + sel + " grad features") if want_f else None, close(gkw, ref[2], tag + sel + " grad kernel_weights") if want_w else None)
        if want_f:
            assert (gf[POISON] == 0.0).all() and (gf[sc.n0 - 1] == 0.0).all(), tag + sel + ": the row of a target nobody lists is not exactly 0"
        if first is None:
            first, ratios = (gf, gkw), r
    return ratios
