"""CPU: what conv1d_1x1, pool_bn and up_conv (contrastboundary_amd/unary.py) answer to their arguments, before any kernel runs — the exception TYPE of
every bad combination, and of the mixed ones that pin the ORDER of the checks (the first exception raised is the one that counts) — then the good paths
(bn=False, training, evaluation) and zero rows, forward and backward.  The ops run on CPU tensors over the whole library compiled for the host
(tests/host_emul/host_mirror.py), at rows 8 and widths 4 and 5."""
import pytest
import torch

from tests.host_emul import host_mirror

ROWS, C_IN, C_OUT, N1, K = 8, 4, 5, 3, 2


class _Table(torch.Tensor):
    """up_conv tests its table's device itself, not through the hook the mirror replaces: a CPU table that answers as the device's would"""
    is_cuda = property(lambda self: True)


def table(rows=ROWS, k=K, n1=N1, dtype=torch.int32):
    t = (torch.arange(rows * k).reshape(rows, k) % (n1 + 1)).to(dtype)   # (the id n1 is a shadow id: the zero row)
    return t.as_subclass(_Table)


def rnd(*shape, seed=0, dtype=torch.float32):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed + sum(shape)), dtype=torch.float64).to(dtype)


def bn_vectors(c=C_OUT):
    return dict(gamma=rnd(c, seed=1) + 2.0, beta=rnd(c, seed=2), moving_mean=rnd(c, seed=3), moving_variance=rnd(c, seed=4).abs() + 0.5)


def conv_args(rows=ROWS, c_in=C_IN, c_out=C_OUT):
    return dict(features=rnd(rows, c_in), weights=rnd(c_in, c_out, seed=5), biases=rnd(c_out, seed=6), shortcut=rnd(rows, c_out, seed=7), **bn_vectors(c_out))


def pool_args(rows=ROWS, c=C_OUT):
    return dict(x=rnd(rows, c), **bn_vectors(c))


def up_args(n2=ROWS, n1=N1, c_up=C_IN, c_skip=C_OUT, c_out=C_OUT):
    return dict(coarse=rnd(n1, c_up), upsample_inds=table(n2, K, n1), skip=rnd(n2, c_skip, seed=8), weights=rnd(c_up + c_skip, c_out, seed=5),
                biases=rnd(c_out, seed=6), **bn_vectors(c_out))


GOOD = {"conv1d_1x1": conv_args, "pool_bn": pool_args, "up_conv": up_args}
NO_BN = dict(gamma=None, beta=None, moving_mean=None, moving_variance=None)
f64 = lambda n: torch.zeros(n, dtype=torch.float64)

# (op, what is wrong, the arguments replaced in the good call, the exception)
BAD = [
    # ---- conv1d_1x1
    ("conv1d_1x1", "features of float64", dict(features=rnd(ROWS, C_IN, dtype=torch.float64)), TypeError),
    ("conv1d_1x1", "weights of float64", dict(weights=rnd(C_IN, C_OUT, dtype=torch.float64)), TypeError),
    ("conv1d_1x1", "gamma of float64", dict(gamma=f64(C_OUT)), TypeError),
    ("conv1d_1x1", "shortcut of float64", dict(shortcut=rnd(ROWS, C_OUT, dtype=torch.float64)), TypeError),
    ("conv1d_1x1", "features not contiguous", dict(features=rnd(C_IN, ROWS).t()), TypeError),
    ("conv1d_1x1", "moving_mean not contiguous", dict(moving_mean=rnd(2 * C_OUT)[::2]), TypeError),
    ("conv1d_1x1", "features not a tensor", dict(features=[[0.0] * C_IN] * ROWS), TypeError),
    ("conv1d_1x1", "features of rank 3", dict(features=rnd(2, ROWS, C_IN)), ValueError),
    ("conv1d_1x1", "weights of rank 1", dict(weights=rnd(C_IN)), ValueError),
    ("conv1d_1x1", "features and weights that do not fit", dict(features=rnd(ROWS, C_IN + 1)), ValueError),
    ("conv1d_1x1", "gamma without beta", dict(beta=None), ValueError),
    ("conv1d_1x1", "beta without gamma", dict(gamma=None), ValueError),
    ("conv1d_1x1", "moving statistics without a batch norm", dict(gamma=None, beta=None), ValueError),
    ("conv1d_1x1", "moving_mean alone", dict(moving_variance=None), ValueError),
    ("conv1d_1x1", "moving_variance alone", dict(moving_mean=None), ValueError),
    ("conv1d_1x1", "evaluation without moving statistics", dict(moving_mean=None, moving_variance=None, is_training=False), ValueError),
    ("conv1d_1x1", "gamma of the wrong length", dict(gamma=rnd(C_OUT + 1)), ValueError),
    ("conv1d_1x1", "biases of the wrong length", dict(biases=rnd(C_OUT - 1)), ValueError),
    ("conv1d_1x1", "moving_variance of the wrong length", dict(moving_variance=rnd(1)), ValueError),
    ("conv1d_1x1", "beta of rank 2", dict(beta=rnd(1, C_OUT)), ValueError),
    ("conv1d_1x1", "shortcut of the wrong shape", dict(shortcut=rnd(ROWS, C_OUT + 1)), ValueError),
    ("conv1d_1x1", "shortcut of the wrong rows", dict(shortcut=rnd(ROWS + 1, C_OUT)), ValueError),
    ("conv1d_1x1", "c_out 4097", dict(weights=rnd(C_IN, 4097), biases=None, shortcut=None, **NO_BN), NotImplementedError),
    ("conv1d_1x1", "c_in 4097", dict(features=rnd(ROWS, 4097), weights=rnd(4097, C_OUT)), NotImplementedError),
    # the order: types before everything, the two shapes before the limit, the limit before the batch norm's consistency, that before the lengths
    ("conv1d_1x1", "gamma of float64 beside a missing beta", dict(gamma=f64(C_OUT), beta=None), TypeError),
    ("conv1d_1x1", "moving_variance of float64 without a batch norm", dict(gamma=None, beta=None, moving_variance=f64(C_OUT)), TypeError),
    ("conv1d_1x1", "shortcut of float64 beside c_out 4097", dict(weights=rnd(C_IN, 4097), shortcut=rnd(ROWS, C_OUT, dtype=torch.float64)), TypeError),
    ("conv1d_1x1", "c_out 4097 beside features that do not fit", dict(features=rnd(ROWS, C_IN + 1), weights=rnd(C_IN, 4097)), ValueError),
    ("conv1d_1x1", "c_out 4097 beside gamma without beta", dict(weights=rnd(C_IN, 4097), beta=None), NotImplementedError),
    ("conv1d_1x1", "c_out 4097 beside vectors of the wrong length", dict(weights=rnd(C_IN, 4097)), NotImplementedError),
    ("conv1d_1x1", "gamma of the wrong length beside moving_mean alone", dict(gamma=rnd(C_OUT + 1), moving_variance=None), ValueError),
    # ---- pool_bn
    ("pool_bn", "x of float64", dict(x=rnd(ROWS, C_OUT, dtype=torch.float64)), TypeError),
    ("pool_bn", "beta of float64", dict(beta=f64(C_OUT)), TypeError),
    ("pool_bn", "x not contiguous", dict(x=rnd(C_OUT, ROWS).t()), TypeError),
    ("pool_bn", "x of rank 1", dict(x=rnd(C_OUT)), ValueError),
    ("pool_bn", "x of rank 3", dict(x=rnd(2, ROWS, C_OUT)), ValueError),
    ("pool_bn", "gamma without beta", dict(beta=None), ValueError),
    ("pool_bn", "moving statistics without a batch norm", dict(gamma=None, beta=None), ValueError),
    ("pool_bn", "moving_mean alone", dict(moving_variance=None), ValueError),
    ("pool_bn", "evaluation without moving statistics", dict(moving_mean=None, moving_variance=None, is_training=False), ValueError),
    ("pool_bn", "gamma of the wrong length", dict(gamma=rnd(C_OUT + 1)), ValueError),
    ("pool_bn", "moving_mean of the wrong length", dict(moving_mean=rnd(C_OUT - 1)), ValueError),
    ("pool_bn", "width 4097", dict(x=rnd(ROWS, 4097), **NO_BN), NotImplementedError),
    ("pool_bn", "beta of float64 beside a missing gamma", dict(gamma=None, beta=f64(C_OUT)), TypeError),
    ("pool_bn", "gamma of float64 beside x of rank 3", dict(x=rnd(2, ROWS, C_OUT), gamma=f64(C_OUT)), TypeError),
    ("pool_bn", "width 4097 beside gamma without beta", dict(x=rnd(ROWS, 4097), beta=None), NotImplementedError),
    ("pool_bn", "width 4097 beside vectors of the wrong length", dict(x=rnd(ROWS, 4097)), NotImplementedError),
    # ---- up_conv
    ("up_conv", "coarse of float64", dict(coarse=rnd(N1, C_IN, dtype=torch.float64)), TypeError),
    ("up_conv", "skip not contiguous", dict(skip=rnd(C_OUT, ROWS).t()), TypeError),
    ("up_conv", "a table of int64", dict(upsample_inds=table(dtype=torch.int64)), TypeError),
    ("up_conv", "a table not contiguous", dict(upsample_inds=table(k=2 * K)[:, ::2]), TypeError),
    ("up_conv", "biases of float64", dict(biases=f64(C_OUT)), TypeError),
    ("up_conv", "coarse of rank 3", dict(coarse=rnd(1, N1, C_IN)), ValueError),
    ("up_conv", "a table of rank 1", dict(upsample_inds=table(k=1).reshape(-1)), ValueError),
    ("up_conv", "a table without a column", dict(upsample_inds=table(k=0)), ValueError),
    ("up_conv", "a table of other rows than skip", dict(upsample_inds=table(rows=ROWS + 1)), ValueError),
    ("up_conv", "c_up + c_skip != weights.shape[0]", dict(weights=rnd(C_IN + C_OUT + 1, C_OUT)), ValueError),
    ("up_conv", "n1 == 0", dict(coarse=rnd(0, C_IN)), ValueError),
    ("up_conv", "gamma without beta", dict(beta=None), ValueError),
    ("up_conv", "moving statistics without a batch norm", dict(gamma=None, beta=None), ValueError),
    ("up_conv", "moving_variance alone", dict(moving_mean=None), ValueError),
    ("up_conv", "evaluation without moving statistics", dict(moving_mean=None, moving_variance=None, is_training=False), ValueError),
    ("up_conv", "beta of the wrong length", dict(beta=rnd(C_OUT + 2)), ValueError),
    ("up_conv", "biases of the wrong length", dict(biases=rnd(1)), ValueError),
    ("up_conv", "c_out 4097", dict(weights=rnd(C_IN + C_OUT, 4097), biases=None, **NO_BN), NotImplementedError),
    ("up_conv", "c_up + c_skip 4097", dict(coarse=rnd(N1, 4092), weights=rnd(4097, C_OUT)), NotImplementedError),
    ("up_conv", "gamma of float64 beside a table of other rows", dict(gamma=f64(C_OUT), upsample_inds=table(rows=ROWS + 1)), TypeError),
    ("up_conv", "moving_mean of float64 beside a missing moving_variance", dict(moving_mean=f64(C_OUT), moving_variance=None), TypeError),
    ("up_conv", "c_out 4097 beside a table of other rows", dict(weights=rnd(C_IN + C_OUT, 4097), upsample_inds=table(rows=ROWS + 1)), ValueError),
    ("up_conv", "c_out 4097 beside n1 == 0", dict(weights=rnd(C_IN + C_OUT, 4097), coarse=rnd(0, C_IN)), ValueError),
    ("up_conv", "c_out 4097 beside gamma without beta", dict(weights=rnd(C_IN + C_OUT, 4097), beta=None), NotImplementedError),
    ("up_conv", "c_out 4097 beside vectors of the wrong length", dict(weights=rnd(C_IN + C_OUT, 4097)), NotImplementedError),
]


def call(op, args):
    from contrastboundary_amd import unary
    args = dict(args)
    first = [args.pop(name) for name in {"conv1d_1x1": ("features", "weights"), "pool_bn": ("x",), "up_conv": ("coarse", "upsample_inds", "skip", "weights")}[op]]
    return getattr(unary, op)(*first, **args)


@pytest.mark.parametrize("op,what,replaced,exception", BAD, ids=["%s: %s" % (c[0], c[1]) for c in BAD])
def test_the_first_exception_of_every_bad_combination(op, what, replaced, exception):
    with host_mirror.mirror():
        with pytest.raises(Exception) as info:
            call(op, dict(GOOD[op](), **replaced))
    assert type(info.value) is exception, "%s: %r" % (what, info.value)


def test_a_cpu_tensor_is_refused_outside_the_mirror():
    """there is no fallback: the hook the mirror replaces is what refuses a CPU tensor"""
    for op in sorted(GOOD):
        with pytest.raises(TypeError):
            call(op, GOOD[op]())


MODES = {"bn=False": dict(NO_BN), "training": dict(is_training=True), "evaluation": dict(is_training=False)}


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("op", sorted(GOOD))
def test_the_good_paths_run(op, mode):
    """finite output of the right shape; training moves the moving statistics, evaluation and bn=False leave them alone"""
    args = dict(GOOD[op](), **MODES[mode])
    before = None if args["moving_mean"] is None else (args["moving_mean"].clone(), args["moving_variance"].clone())
    with host_mirror.mirror():
        out = call(op, args)
    assert tuple(out.shape) == (ROWS, C_OUT) and out.dtype == torch.float32 and bool(torch.isfinite(out).all())
    if before is not None:
        moved = not torch.equal(before[0], args["moving_mean"]) and not torch.equal(before[1], args["moving_variance"])
        assert moved == (mode == "training")


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("op", sorted(GOOD))
def test_zero_rows_forward_and_backward(op, mode):
    """no row: an empty output, empty gradients of the rows, and ZEROS in every gradient that is a sum over the rows"""
    args = dict(GOOD[op](0), **MODES[mode])
    diff = [name for name, t in args.items() if isinstance(t, torch.Tensor) and t.is_floating_point() and not name.startswith("moving")]
    for name in diff:
        args[name] = args[name].clone().requires_grad_(True)
    before = None if args["moving_mean"] is None else (args["moving_mean"].clone(), args["moving_variance"].clone())
    with host_mirror.mirror():
        out = call(op, args)
        assert tuple(out.shape) == (0, C_OUT)
        out.backward(torch.zeros_like(out))
    for name in diff:
        t, g = args[name], args[name].grad
        assert g is not None and g.shape == t.shape, name
        if name in ("features", "x", "skip", "shortcut"):
            assert g.numel() == 0, name
        else:
            assert g.numel() > 0 and bool((g == 0).all()), name    # coarse, weights, biases, gamma, beta
    if before is not None:                                           # nothing was launched
        assert torch.equal(before[0], args["moving_mean"]) and torch.equal(before[1], args["moving_variance"])
