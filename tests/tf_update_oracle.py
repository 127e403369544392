"""TEST ORACLE: the three fragments of the reference's TF-side parameter update restated in float64 numpy, from the TensorFlow semantics they rest on —

  weight loss   wd * tf.nn.l2_loss(var) = wd * sum(var^2) / 2 for every variable created with wd > 0, added up (tensorflow/models/basic_operators.py:100-130,
                :371-378; build_models.py:140-145)
  clip          tf.clip_by_norm(g, c) = g * c / max(||g||_2, c) on every variable by itself, per tower, before the towers are averaged
                (tensorflow/utils/average_gradients.py:21-30, :41-51)
  step          tf.train.MomentumOptimizer: accum = momentum * accum + g; var -= lr * accum (tensorflow/utils/tf_graph_builder.py:99-100)

TensorFlow is absent here, so this is a restatement of documented semantics, not a recording: parity is unpinned by execution.  It uses nothing of the kernels
(csrc/tf_update.hip): no chunks, no partial sums.  Beside the oracle: the cases and the checks tests/test_tf_update_host.py (host emulation) and
tests/test_gpu_tf_update.py (device) share, written against a `Driver` that hides where the buffers live.

Tolerances.  eps = 2^-23, u = eps / 2 the unit roundoff of fp32.  The scalars (lr, clip_norm, momentum, grad_scale, seg_wd) reach the kernels
as fp32 and the oracle takes those fp32 values, so they add nothing.
  norms, loss     sums of squares accumulated in fp64 over fp32 inputs, one rounding to fp32 at the end (and, under fold_decay, the two roundings of
                  h = g + wd w): a few u.  Held to 1e-6 relative.
  g'              fl(wd w), fl(g + .), fl(h clip), fl(. / den), den within 6 u:  |err| <= 10 u |g'| + 4 u wd |w|
  accum'          fl(m a), fl(s g'), fl(+):                                      |err| <= 2 u |a| + 12 u |g'| + 4 u wd |w|
  w'              fl(lr a'), fl(w - .):                                          |err| <= u (5 |w| + 4 lr |a| + 14 lr |g'|)     (lr wd <= 1)
  every one is within  BOUND = 8 eps  times  (|g'| + wd |w|),  (|a| + |g'| + wd |w|),  (|w| + lr |a| + lr |g'|)  respectively — two orders below the project's
  1e-4 of the segment's scale.  The checks report the largest observed ratio to the bound."""
import ctypes

import numpy as np

EPS = 2.0 ** -23
BOUND = 8 * EPS
REL = 1e-6
CHUNK = 2048                                                         # TU_CHUNK (csrc/tf_update.hip)
CAP_CHUNKS = 1024 * 4                                                # TU_MAX_BLOCKS workgroups of TU_WAVES waves, one chunk per wave and trip
CLIP, STEP = 1, 2
EDGE_SIZES = [1, 3, 4, 63, 64, 65, 255, CHUNK, CHUNK + 1, 2 * CHUNK + 5]
EDGE_WD = [0.05, 0.0, 0.5, 0.001, 0.0, 0.0, 0.0, 0.0, 0.01, 0.1]     # mixed; 0 on the segments whose gradient norm the case pins (4: zero, 5, 6, 7)
CLIP_NORM, MOMENTUM, LR = 2.0, 0.98, 0.01
ratios = {}                                                          # what -> the largest observed error / bound of this process (profiles/tf_update_device.md)


# ---------------------------------------------------------------------------------------------- the oracle
def f64(a):
    return np.asarray(a, np.float64)


def segments(begin):
    return [(int(begin[s]), int(begin[s + 1])) for s in range(len(begin) - 1)]


def weight_loss(params, begin, wd):
    """-> (loss, per-segment terms); a segment with wd = 0 contributes 0 whatever it holds"""
    terms = np.array([float(c) * 0.5 * np.sum(f64(params[a:b]) ** 2) if c != 0 else 0.0 for (a, b), c in zip(segments(begin), wd)])
    return terms.sum(), terms


def weight_loss_grad(params, begin, wd, grad_loss):
    out = np.zeros(len(params))
    for (a, b), c in zip(segments(begin), wd):
        if c != 0:
            out[a:b] = float(grad_loss) * float(c) * f64(params[a:b])
    return out


def clip_by_norm(g, clip_norm):
    """tf.clip_by_norm: -> (g * clip_norm / max(norm, clip_norm), norm); clip_norm <= 0: no clip (use_clip, average_gradients.py:21)"""
    norm = np.sqrt(np.sum(g * g))
    return (g * clip_norm / max(norm, clip_norm) if clip_norm > 0 else g), norm


def clip(params, grads, begin, wd, clip_norm, fold):
    """-> (g' (float64), norms): per segment h = g + (fold ? wd w : 0), clipped by its own norm"""
    out, norms = f64(grads).copy(), np.zeros(len(begin) - 1)
    for s, (a, b) in enumerate(segments(begin)):
        h = f64(grads[a:b]) + (float(wd[s]) * f64(params[a:b]) if fold else 0.0)
        out[a:b], norms[s] = clip_by_norm(h, clip_norm)
    return out, norms


def average_towers(tower_grads):
    """average_gradients.py:41-51: the mean over the tower dimension"""
    return np.mean(np.stack([f64(g) for g in tower_grads]), axis=0)


def momentum_step(params, accum, g, lr, momentum):
    a = momentum * f64(accum) + f64(g)
    return f64(params) - lr * a, a


# ---------------------------------------------------------------------------------------------- cases
def f32(x):
    return float(np.float32(x))


def make_case(sizes, seed, shift=1, wd=None, pinned=False):
    """flat fp32 buffers of EXACTLY shift + sum(sizes) elements, the first segment beginning at `shift` (odd begins against an aligned base).  pinned (the ten
    EDGE_SIZES): segment 4's gradient is all zero, 5's norm is just below CLIP_NORM, 6's just above, 7's a thousand times above"""
    rng = np.random.default_rng(seed)
    begin = np.concatenate([[shift], shift + np.cumsum(sizes)]).astype(np.int64)
    total = int(begin[-1])
    case = dict(total=total, begin=begin, S=len(sizes),
                wd=np.asarray(wd if wd is not None else [0.05 if s % 2 == 0 else 0.0 for s in range(len(sizes))], np.float32),
                params=rng.normal(size=total).astype(np.float32), grads=rng.normal(size=total).astype(np.float32),
                accum=rng.normal(0, 0.5, size=total).astype(np.float32))
    if pinned:
        for s, factor in ((4, 0.0), (5, 1 - 1e-5), (6, 1 + 1e-5), (7, 1e3)):
            a, b = segments(begin)[s]
            g = f64(case["grads"][a:b])
            case["grads"][a:b] = (g * (factor * CLIP_NORM / np.sqrt(np.sum(g * g)))).astype(np.float32)
    return case


def edge_case():
    return make_case(EDGE_SIZES, 7, wd=EDGE_WD, pinned=True)


# ---------------------------------------------------------------------------------------------- a driver over one build of the library
class Driver:
    """the entries of one build of the library (host emulation, or the device's) over numpy arrays: put(array, off) -> a buffer of exactly that many elements
    where the kernels run (off: elements its base lies behind a 16-byte boundary), get(buffer) -> numpy, ptr(buffer) -> c_void_p.  Nothing a caller passes in
    is modified; outputs that are written are pre-filled with NaN"""

    def __init__(self, L, put, get, ptr):
        self.L, self.put, self.get, self.ptr = L, put, get, ptr

    def plan(self, total, begin, plan_bytes=None):
        """-> (code, plan (int32 array), n_chunks); host code in every build"""
        S = len(begin) - 1
        n = self.L.cbl_tf_update_plan_bytes(ctypes.c_longlong(total), ctypes.c_longlong(S))
        plan = np.full(max(1, n // 4), -7, np.int32)
        nc = ctypes.c_longlong(-1)
        b = np.ascontiguousarray(begin, np.int64)
        rc = self.L.cbl_tf_update_plan(ctypes.c_longlong(total), ctypes.c_longlong(S), b.ctypes.data_as(ctypes.c_void_p), plan.ctypes.data_as(ctypes.c_void_p),
                                       ctypes.c_size_t(n if plan_bytes is None else plan_bytes), ctypes.byref(nc))
        return rc, plan, nc.value

    def layout(self, case):
        rc, plan, nc = self.plan(case["total"], case["begin"])
        assert rc == 0, rc
        S = case["S"]
        starts = plan[:S + 1]
        assert starts[0] == 0 and starts[S] == nc and nc == sum(-(-(b - a) // CHUNK) for a, b in segments(case["begin"]))
        assert all((plan[S + 1 + starts[s]:S + 1 + starts[s + 1]] == s).all() for s in range(S))
        ws = self.L.cbl_tf_update_workspace_bytes(ctypes.c_longlong(case["total"]), ctypes.c_longlong(S))
        return dict(total=ctypes.c_longlong(case["total"]), S=ctypes.c_longlong(S), begin=self.put(case["begin"]), plan=self.put(plan), nc=ctypes.c_longlong(nc),
                    ws=self.put(np.zeros(ws, np.uint8)), ws_bytes=ctypes.c_size_t(ws))

    def weight_loss(self, case, lay, params=None, wd=None, want_terms=True):
        p = self.put(case["params"] if params is None else params)
        loss, terms = self.put(np.full(1, np.nan, np.float32)), self.put(np.full(case["S"], np.nan, np.float32))
        wd = self.put(case["wd"] if wd is None else wd)              # (every buffer stays referenced until the results are fetched: the launches are asynchronous)
        rc = self.L.cbl_tf_weight_loss_forward(lay["total"], lay["S"], self.ptr(p), self.ptr(lay["begin"]), self.ptr(wd),
                                               self.ptr(lay["plan"]), lay["nc"], self.ptr(loss), self.ptr(terms) if want_terms else None, self.ptr(lay["ws"]),
                                               lay["ws_bytes"], None)
        assert rc == 0, rc
        out = self.get(loss)[0], self.get(terms)
        del wd, p
        return out

    def weight_loss_grad(self, case, lay, grad_loss, params=None, off=0):
        p, g = self.put(case["params"] if params is None else params), self.put(case["grads"], off)
        wd, up = self.put(case["wd"]), self.put(np.full(1, grad_loss, np.float32))
        rc = self.L.cbl_tf_weight_loss_backward(lay["total"], lay["S"], self.ptr(p), self.ptr(lay["begin"]), self.ptr(wd), self.ptr(lay["plan"]),
                                                lay["nc"], self.ptr(up), self.ptr(g), None)
        assert rc == 0, rc
        out = self.get(g)
        del wd, up, p
        return out

    def clip_update(self, case, lay, mode, fold, clip_norm=CLIP_NORM, grad_scale=1.0, lr=LR, momentum=MOMENTUM, grads=None, active=None, off=(0, 0, 0)):
        """-> (params, grads, accum, norms) after the call"""
        p, g, a = self.put(case["params"], off[0]), self.put(case["grads"] if grads is None else grads, off[1]), self.put(case["accum"], off[2])
        norms = self.put(np.full(case["S"], np.nan, np.float32))
        wd, rate = self.put(case["wd"]), self.put(np.full(1, lr, np.float32))
        act = None if active is None else self.put(np.asarray(active, np.int32))
        rc = self.L.cbl_tf_clip_update(lay["total"], lay["S"], ctypes.c_int(mode), ctypes.c_int(fold), self.ptr(p), self.ptr(g), self.ptr(a),
                                       self.ptr(lay["begin"]), self.ptr(wd), None if act is None else self.ptr(act),
                                       self.ptr(lay["plan"]), lay["nc"], ctypes.c_float(clip_norm), ctypes.c_float(momentum), ctypes.c_float(grad_scale),
                                       self.ptr(rate), self.ptr(norms), self.ptr(lay["ws"]), lay["ws_bytes"], None)
        assert rc == 0, rc
        out = self.get(p), self.get(g), self.get(a), self.get(norms)
        del wd, rate, act
        return out


# ---------------------------------------------------------------------------------------------- checks
def within(got, want, scale, what):
    """|got - want| <= BOUND * scale elementwise (and exactly equal where the scale is 0); records the largest ratio"""
    got, want, scale = f64(got), f64(want), f64(scale)
    assert np.isfinite(got).all(), what + ": not finite"
    err = np.abs(got - want)
    ratio = float(np.max(np.where(scale > 0, err / np.where(scale > 0, BOUND * scale, 1.0), np.where(err == 0, 0.0, np.inf)))) if got.size else 0.0
    ratios[what] = max(ratios.get(what, 0.0), ratio)
    assert ratio <= 1.0, "%s: error / bound = %.3g" % (what, ratio)


def relative(got, want, what):
    got, want = f64(got), f64(want)
    assert np.isfinite(got).all(), what + ": not finite"
    err = np.abs(got - want)
    ratio = float(np.max(np.where(want != 0, err / np.where(want != 0, REL * np.abs(want), 1.0), np.where(err == 0, 0.0, np.inf))))
    ratios[what] = max(ratios.get(what, 0.0), ratio)
    assert ratio <= 1.0, "%s: relative error / 1e-6 = %.3g" % (what, ratio)


def per_element(case, per_segment):
    out = np.zeros(case["total"])
    for (a, b), v in zip(segments(case["begin"]), per_segment):
        out[a:b] = v
    return out


def inside(case):
    m = np.zeros(case["total"], bool)
    m[int(case["begin"][0]):int(case["begin"][-1])] = True
    return m


def expected_update(case, mode, fold, clip_norm, grad_scale, lr, momentum, grads=None):
    """the oracle's (params, grads, accum, norms) and the three error scales, with the scalars as the fp32 values the kernels receive"""
    grads = case["grads"] if grads is None else grads
    clip_norm, grad_scale, lr, momentum = f32(clip_norm), f32(grad_scale), f32(lr), f32(momentum)
    fold = bool(fold) and bool(mode & CLIP)
    wdw = np.abs(per_element(case, f64(case["wd"])) * f64(case["params"])) if fold else np.zeros(case["total"])
    gp, norms = clip(case["params"], grads, case["begin"], case["wd"], clip_norm, fold) if mode & CLIP else (f64(grads), None)
    m = inside(case)
    gp = np.where(m, gp, f64(grads))
    if mode & STEP:
        w, a = momentum_step(case["params"], case["accum"], grad_scale * gp, lr, momentum)
        w, a = np.where(m, w, f64(case["params"])), np.where(m, a, f64(case["accum"]))
    else:
        w, a = f64(case["params"]), f64(case["accum"])
    scales = dict(g=np.abs(gp) + wdw, a=np.abs(f64(case["accum"])) + np.abs(gp) + wdw, w=np.abs(f64(case["params"])) + lr * (np.abs(f64(case["accum"])) + np.abs(gp)))
    return w, gp, a, norms, scales


def check_update(drv, case, lay, mode, fold, clip_norm=CLIP_NORM, grad_scale=1.0, lr=LR, grads=None, off=(0, 0, 0), what=""):
    """one cbl_tf_clip_update call against the oracle; the mode bits' promises: CLIP alone leaves params / accum bit-unchanged, STEP alone leaves grads
    bit-unchanged; nothing outside the segments changes.  -> the call's outputs"""
    grads = case["grads"] if grads is None else grads
    w, g, a, norms = drv.clip_update(case, lay, mode, fold, clip_norm, grad_scale, lr, grads=grads, off=off)
    ew, eg, ea, enorms, sc = expected_update(case, mode, fold, clip_norm, grad_scale, lr, MOMENTUM, grads)
    tag = "%s mode %d fold %d" % (what, mode, fold)
    out = ~inside(case)
    assert np.array_equal(w[out], case["params"][out]) and np.array_equal(g[out], grads[out]) and np.array_equal(a[out], case["accum"][out]), tag + ": wrote outside"
    if mode & CLIP:
        relative(norms, enorms, "norms")
        within(g, eg, sc["g"], "clipped gradient")
    else:
        assert np.array_equal(g.view(np.int32), grads.view(np.int32)), tag + ": STEP alone changed grads"
        assert np.isnan(norms).all(), tag + ": STEP alone wrote norms"
    if mode & STEP:
        within(a, ea, sc["a"], "momentum")
        within(w, ew, sc["w"], "updated parameter")
    else:
        assert np.array_equal(w.view(np.int32), case["params"].view(np.int32)) and np.array_equal(a.view(np.int32), case["accum"].view(np.int32)), \
            tag + ": CLIP alone changed params / accum"
    return w, g, a, norms


def check_all_modes(drv, case, what=""):
    """every mode, fold_decay on and off, clip_norm = 0, and CLIP then STEP(1/2) against the oracle's average of two identical towers"""
    lay = drv.layout(case)
    for fold in (0, 1):
        check_update(drv, case, lay, CLIP | STEP, fold, what=what)
        _, g1, _, norms = check_update(drv, case, lay, CLIP, fold, what=what)
        check_update(drv, case, lay, CLIP | STEP, fold, clip_norm=0.0, what=what + " no clip")
        # two towers with the same gradients: clip each (the same g'), average, step.  Ours: CLIP, (all-reduce: a sum, 2 g'), STEP with grad_scale = 1/2
        tower, _ = clip(case["params"], case["grads"], case["begin"], case["wd"], f32(CLIP_NORM), bool(fold))
        mean = average_towers([tower, tower])
        ew, ea = momentum_step(case["params"], case["accum"], mean, f32(LR), f32(MOMENTUM))
        summed = (2 * g1).astype(np.float32)                          # exact: a doubling
        w, g, a, _ = drv.clip_update(case, lay, STEP, 0, grad_scale=0.5, grads=summed)
        m = inside(case)
        _, _, _, _, sc = expected_update(case, CLIP | STEP, fold, CLIP_NORM, 1.0, LR, MOMENTUM)
        within(a[m], ea[m], sc["a"][m], "momentum")
        within(w[m], ew[m], sc["w"][m], "updated parameter")
        assert np.array_equal(g, summed)
    check_update(drv, case, lay, STEP, 0, what=what)
    check_update(drv, case, lay, STEP, 1, grad_scale=0.25, what=what)       # fold_decay is CLIP's: STEP alone ignores it
    return lay


def check_weight_loss(drv, case, lay):
    loss, terms = drv.weight_loss(case, lay)
    eloss, eterms = weight_loss(case["params"], case["begin"], case["wd"])
    relative(loss, eloss, "weight loss")
    relative(terms, eterms, "weight loss terms")
    loss2, _ = drv.weight_loss(case, lay, want_terms=False)
    assert loss2 == loss
    # a segment with wd = 0 is not read: NaN there must not reach the loss, nor its term
    poisoned = case["params"].copy()
    for (a, b), c in zip(segments(case["begin"]), case["wd"]):
        if c == 0:
            poisoned[a:b] = np.nan
    poisoned[~inside(case)] = np.nan
    loss3, terms3 = drv.weight_loss(case, lay, params=poisoned)
    assert loss3 == loss and np.array_equal(terms3, terms)
    # the gradient ACCUMULATES: grads + grad_loss * wd * w; undecayed segments are neither read nor written
    for off in (0, 1):
        g = drv.weight_loss_grad(case, lay, 0.75, params=poisoned, off=off)
        add = weight_loss_grad(case["params"], case["begin"], case["wd"], f32(0.75))
        decayed = per_element(case, f64(case["wd"])) != 0
        within(g[decayed], (f64(case["grads"]) + add)[decayed], (np.abs(f64(case["grads"])) + np.abs(add))[decayed], "weight loss gradient")
        assert np.array_equal(g[~decayed], case["grads"][~decayed])


def check_pinned_norms(drv, case, lay):
    """the gradient cases of the edge buffer: a zero gradient has norm 0 and stays zero (no NaN), the segments just below / above / far above the clip norm"""
    _, g, _, norms = drv.clip_update(case, lay, CLIP, 0)
    segs = segments(case["begin"])
    assert norms[4] == 0.0 and not g[segs[4][0]:segs[4][1]].any()
    assert norms[5] < CLIP_NORM < norms[6] and abs(norms[7] / CLIP_NORM - 1e3) < 1
    after = [np.sqrt(np.sum(f64(g[a:b]) ** 2)) for a, b in segs]
    assert abs(after[5] - norms[5]) < 1e-5 and abs(after[6] - CLIP_NORM) < 1e-5 and abs(after[7] - CLIP_NORM) < 1e-5
    _, g0, _, norms0 = drv.clip_update(case, lay, CLIP, 0, clip_norm=0.0)
    assert np.array_equal(g0, case["grads"]) and np.array_equal(norms0, norms)      # no clip: the gradients as they were, the norms still reported


def check_inactive(drv, case, lay, idle):
    """segments with seg_active = 0 keep value, momentum and gradient bit for bit; the others are updated as without the mask"""
    active = [0 if s in idle else 1 for s in range(case["S"])]
    w, g, a, norms = drv.clip_update(case, lay, CLIP | STEP, 1, active=active)
    w1, g1, a1, norms1 = drv.clip_update(case, lay, CLIP | STEP, 1)
    assert np.array_equal(norms, norms1)
    for s, (b, e) in enumerate(segments(case["begin"])):
        for got, full, before in ((w, w1, case["params"]), (g, g1, case["grads"]), (a, a1, case["accum"])):
            assert np.array_equal(got[b:e], before[b:e] if s in idle else full[b:e])


def check_deterministic(drv, case, lay):
    one, two = drv.clip_update(case, lay, CLIP | STEP, 1), drv.clip_update(case, lay, CLIP | STEP, 1)
    assert all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(one, two))
    assert drv.weight_loss(case, lay)[0] == drv.weight_loss(case, lay)[0]


def check_arguments(L, device_pointer=None):
    """the documented code of every bad argument (cbl_amd.h): validation happens before any launch, so `L` may be the device build on a machine without a GPU.
    device_pointer: any non-null address standing in for device memory (never dereferenced: every call here fails)"""
    BAD, WS, UNSUPPORTED = -1, -2, -3
    ll, sz, null = ctypes.c_longlong, ctypes.c_size_t, None
    drv = Driver(L, None, None, None)
    begin = np.array([1, 4, 9], np.int64)
    assert drv.plan(9, begin)[0] == 0 and drv.plan(9, begin)[2] == 2
    assert drv.plan(8, begin)[0] == BAD                              # the last segment ends behind total
    assert drv.plan(9, np.array([-1, 4, 9]))[0] == BAD
    assert drv.plan(9, np.array([1, 9, 4]))[0] == BAD                # descending
    assert drv.plan(9, np.array([1, 4, 4]))[0] == BAD                # an empty segment
    assert drv.plan(9, begin, plan_bytes=4)[0] == WS
    assert drv.plan(0, np.array([0]))[:3:2] == (0, 0)                # S = 0
    nc = ctypes.c_longlong(0)
    assert L.cbl_tf_update_plan(ll(9), ll(2), null, null, sz(64), ctypes.byref(nc)) == BAD
    assert L.cbl_tf_update_plan(ll(9), ll(2), begin.ctypes.data_as(ctypes.c_void_p), null, sz(64), ctypes.byref(nc)) == BAD
    assert L.cbl_tf_update_plan(ll(-1), ll(2), null, null, sz(64), ctypes.byref(nc)) == BAD
    assert L.cbl_tf_update_plan(ll(1 << 45), ll(1), np.array([0, 1 << 45], np.int64).ctypes.data_as(ctypes.c_void_p), null, sz(0), ctypes.byref(nc)) == BAD
    scratch = np.zeros(64, np.int64)
    assert L.cbl_tf_update_plan(ll(1 << 45), ll(1), np.array([0, 1 << 45], np.int64).ctypes.data_as(ctypes.c_void_p), scratch.ctypes.data_as(ctypes.c_void_p),
                                sz(0), ctypes.byref(nc)) == UNSUPPORTED                 # 2^34 chunks
    x = ctypes.c_void_p(device_pointer if device_pointer is not None else scratch.ctypes.data)
    ws = L.cbl_tf_update_workspace_bytes(ll(9), ll(2))
    assert ws >= 8 * 2 + 12 * 2
    f = ctypes.c_float
    upd = lambda total=9, S=2, mode=3, fold=1, p=x, g=x, a=x, b=x, wd=x, plan=x, n=2, lr=x, norms=x, w=x, wb=ws: L.cbl_tf_clip_update(
        ll(total), ll(S), ctypes.c_int(mode), ctypes.c_int(fold), p, g, a, b, wd, null, plan, ll(n), f(1.0), f(0.9), f(1.0), lr, norms, w, sz(wb), null)
    assert upd(S=0) == 0 and upd(S=0, p=null, g=null, a=null, b=null, plan=null) == 0
    for bad in (dict(total=-1), dict(S=-1), dict(mode=0), dict(mode=4), dict(g=null), dict(b=null), dict(plan=null), dict(n=1), dict(n=3), dict(p=null),
                dict(a=null), dict(lr=null), dict(norms=null), dict(w=null), dict(wd=null), dict(mode=1, fold=1, p=null), dict(mode=2, a=null)):
        assert upd(**bad) == BAD, bad
    assert upd(wb=ws - 1) == WS and upd(mode=1, wb=0) == WS
    fwd = lambda total=9, S=2, p=x, b=x, wd=x, plan=x, n=2, loss=x, w=x, wb=ws: L.cbl_tf_weight_loss_forward(ll(total), ll(S), p, b, wd, plan, ll(n), loss, null, w,
                                                                                                            sz(wb), null)
    assert fwd(S=0) == 0
    for bad in (dict(total=-1), dict(S=-1), dict(p=null), dict(b=null), dict(wd=null), dict(plan=null), dict(n=0), dict(loss=null), dict(w=null)):
        assert fwd(**bad) == BAD, bad
    assert fwd(wb=ws - 1) == WS
    bwd = lambda total=9, S=2, p=x, b=x, wd=x, plan=x, n=2, gl=x, g=x: L.cbl_tf_weight_loss_backward(ll(total), ll(S), p, b, wd, plan, ll(n), gl, g, null)
    assert bwd(S=0) == 0
    for bad in (dict(total=-1), dict(p=null), dict(b=null), dict(wd=null), dict(plan=null), dict(n=5), dict(gl=null), dict(g=null)):
        assert bwd(**bad) == BAD, bad
