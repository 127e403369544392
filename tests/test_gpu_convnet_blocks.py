"""GPU: LocalAggregation, simple_block / bottleneck / strided_bottleneck and ResnetBackbone (contrastboundary_amd/convnet_blocks.py) on a real pyramid of
tf_ops.segmentation_inputs_radius, against the float64 restatement of the graph code (tests/convnet_blocks_oracle.py; parity unpinned by execution — TF
absent).  The modules are compared through their tf_scopes(): the oracle looks every variable up by its TF name.
The driver (cases, seed rule, oracle, bound) is shared with tests/test_convnet_blocks_host.py, which runs it on the host-emulated library (source='host').
Tolerance: the oracle is the reference.  The error of a run is ONE figure: the worst, over every tensor (outputs, the features' gradient, every
parameter's gradient, every updated buffer) and every entry, of |got - ref| over the largest |ref| of that tensor (convnet_blocks_oracle.error_figure).  The
bound is 4 x that figure of the SAME oracle evaluated in float32 on the CPU (an independent fp32 evaluation; the factor covers another summation order).
No entry is excluded.  (One figure per case, not one per tensor: a buffer of eight floats is reproduced by one fp32 evaluation to a fifth of a unit in the
last place by luck, and four times that is less than the half unit any float32 result may be off.)  Seeds: the first of 0, 1, ... for which the float64 oracle finds no
pre-activation within 1e-5 of zero and no two candidates of a maximum within 5e-5 (a CPU search over the oracle, repeated and asserted by every case)."""
import functools

import numpy as np
import pytest
import torch

from tests import convnet_blocks_oracle as O

pytestmark = pytest.mark.gpu

WIDTH, RATIO = 24, 2                                                  # base width and bottleneck ratio: mid widths 12 and 24
DL0, DENSITY = 0.05, 5.0                                              # first_subsampling_dl, density_parameter: r0 = 0.125
KERNEL_POINTS = 15


def cloud(n, seed):
    return np.random.default_rng(seed).uniform(0.0, 1.0, (n, 3)).astype(np.float32) * np.array([1.0, 1.0, 0.4], np.float32)


def clustered_cloud(n, seed, spread):
    """n points in n / 8 tight groups of 8 (a scene of small objects) in the unit cube: the first subsampling keeps about one point a group, so the
    deeper layers are small — the backbone's pre-activations, each of which a seed has to keep out of the guard band, stay countable"""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(0.0, 1.0, (n // 8, 3))
    return (np.repeat(centres, 8, axis=0) + rng.uniform(-spread, spread, (n, 3))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def pyramid(n, layers, dl0, seed=0, limit=20, clustered=False, source="device"):
    """-> (the pyramid as tensors, as numpy arrays): points, neighbors, pools of tf_ops.segmentation_inputs_radius; source 'host': the same entry
    (cbl_pyramid) of the host-emulated library, CPU tensors (tests/test_convnet_blocks_host.py)"""
    xyz = clustered_cloud(n, seed, 0.2 * dl0) if clustered else cloud(n, seed)
    if source == "host":
        from tests.host_emul import host_mirror
        host = host_mirror.pyramid(xyz, dl0, DENSITY, layers, [limit] * (layers + 1))
        return {k: [torch.from_numpy(a) for a in v] for k, v in host.items()}, host
    from contrastboundary_amd import tf_ops
    pts = torch.from_numpy(xyz).cuda()
    pyr = tf_ops.segmentation_inputs_radius(pts, torch.tensor([n], dtype=torch.int32, device="cuda"), dl0, DENSITY, layers, [limit] * (layers + 1))
    host = {k: [t.cpu().numpy() for t in pyr[k]] for k in ("points", "neighbors", "pools")}
    return pyr, host


def kernel_points(radius=1.0, seed=5):
    """a fixed kernel-point set (their generator is not part of the library): the centre and 14 points inside the sphere of `radius`"""
    rng = np.random.default_rng(seed)
    p = rng.normal(size=(KERNEL_POINTS, 3))
    p = p / np.linalg.norm(p, axis=1, keepdims=True) * rng.uniform(0.3, 1.0, (KERNEL_POINTS, 1)) ** (1 / 3)
    p[0] = 0.0
    return (p * radius).astype(np.float32)


R0 = DL0 * DENSITY / 2
LA = {"adaptive_weight": dict(kind="adaptive_weight"),               # the shipped options: 'dp', shared_channels 1, no softmax, mean
      "pospool": dict(kind="pospool", position_embedding="xyz", reduction="mean"),
      "pointwisemlp": dict(kind="pointwisemlp", local_input_feature="dp_fj", reduction="max"),
      "pseudo_grid": dict(kind="pseudo_grid", KP_extent=1.0, density_parameter=DENSITY, KP_influence="linear", convolution_mode="sum"),
      "identity": dict(kind="identity")}


def la_of(kind, radius):
    la = dict(LA[kind])
    if kind == "pseudo_grid":
        la["kernel_points"] = kernel_points(1.5 * la["KP_extent"] * radius / la["density_parameter"])
    return la


def module_la(la):
    return {k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in la.items()}


# name -> (kind of block, aggregation, in width, out width)
CASES = {"simple adaptive_weight": ("simple", "adaptive_weight", WIDTH, WIDTH),
         "simple pospool": ("simple", "pospool", WIDTH, WIDTH),
         "simple pointwisemlp": ("simple", "pointwisemlp", WIDTH, WIDTH),
         "simple pseudo_grid": ("simple", "pseudo_grid", WIDTH, WIDTH),
         "simple identity": ("simple", "identity", WIDTH, WIDTH),
         "simple identity widening": ("simple", "identity", WIDTH, 2 * WIDTH),        # output_conv in the place of pool_bn (:297-302)
         "simple pospool widening": ("simple", "pospool", WIDTH, 2 * WIDTH),          # pool_bn AND output_conv
         "bottleneck": ("bottleneck", "adaptive_weight", WIDTH, WIDTH),               # no shortcut conv
         "bottleneck widening": ("bottleneck", "adaptive_weight", WIDTH, 2 * WIDTH),  # shortcut conv
         "strided": ("strided", "adaptive_weight", WIDTH, 2 * WIDTH),
         "strided same width": ("strided", "pospool", WIDTH, WIDTH)}


def build_module(name):
    from contrastboundary_amd import convnet_blocks as B
    block, kind, c_in, c_out = CASES[name]
    la = module_la(la_of(kind, R0))
    if block == "simple":
        return B.SimpleBlock(0, c_in, c_out, R0, la, scope="blk")
    if block == "bottleneck":
        return B.Bottleneck(0, c_in, c_out, RATIO, R0, la, scope="blk")
    return B.StridedBottleneck(0, c_in, c_out, RATIO, R0, la, scope="blk")


def oracle_build(name, inputs):
    block, kind, c_in, c_out = CASES[name]
    la = la_of(kind, R0)
    if block == "simple":
        return lambda g, f: O.simple_block(g, 0, la, inputs, f, "blk", R0, c_out)
    return lambda g, f: O.bottleneck(g, 0, la, inputs, f, "blk", R0, c_out, RATIO, strided=block == "strided")


def data(rows_in, c_in, rows_out, c_out, seed):
    rng = np.random.default_rng(1000 + seed)
    return rng.normal(size=(rows_in, c_in)).astype(np.float32), rng.normal(size=(rows_out, c_out)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def prepared(name, training, source="device"):
    """-> (seed, module on the CPU with that seed's variables, its TF-named variables, features, cotangent): the first seed the float64 oracle guards in
    that mode"""
    _, host = pyramid(300, 2, DL0, source=source)
    block = CASES[name][0]
    n_in, n_out = host["points"][0].shape[0], host["points"][1 if block == "strided" else 0].shape[0]
    for seed in range(32):
        torch.manual_seed(seed)
        m = build_module(name)
        O.randomize_(m, seed)
        variables = O.tf_variables(m)
        f, go = data(n_in, CASES[name][2], n_out, CASES[name][3], seed)
        if O.evaluate(oracle_build(name, host), variables, host, f, go, training=training, backward=False)["guarded"]:
            return seed, m, variables, f, go
    raise AssertionError("no flip-free seed among 32")


def compare(got, ref64, ref32, what):
    """the device's error figure within 4 x the fp32 oracle's; prints both; -> device figure / bound"""
    ref = O.flat(ref64)
    own, own_at = O.error_figure(O.flat(ref32), ref)
    err, err_at = O.error_figure(got, ref)
    print("%s: fp32 oracle error %.3e (%s), device error %.3e (%s)" % (what, own, own_at, err, err_at))
    assert err <= 4.0 * own, "%s: device error %.3e at %s, bound %.3e = 4 x the fp32 oracle's %.3e" % (what, err, err_at, 4.0 * own, own)
    return err / (4.0 * own)


def run_module(m, pyr, f, gos, training, device="cuda"):
    """forward + backward on the device, in the library's deterministic mode (neighbor_state.deterministic(): the aggregators' gradients are gathered in a
    fixed order; the default mode sums some of them with float atomics, whose error varies from run to run — against a bound that is four times the error
    of torch's pairwise fp32 sums that would be a test that passes on some runs only)  -> the flattened results under the oracle's keys"""
    from contrastboundary_amd import neighbor_state
    with neighbor_state.deterministic():
        return _run_module(m, pyr, f, gos, training, device)


def _run_module(m, pyr, f, gos, training, device="cuda"):
    m = m.to(device)
    m.train(training)
    scopes = m.tf_scopes()
    tf_name = lambda key: scopes[key] + "/" + key.rsplit(".", 1)[-1]
    buffers = {k: v for k, v in m.named_buffers() if k in scopes}      # (the variables: PseudoGrid's kernel points are a constant of the graph)
    before = {k: v.clone() for k, v in buffers.items()}
    x = torch.from_numpy(f).to(device).requires_grad_(True)
    out = m(pyr, x)
    outs = list(out) if isinstance(out, (list, tuple)) else [out]
    torch.autograd.backward(outs, [torch.from_numpy(g).to(device) for g in gos])
    got = {"out%d" % i: o.detach().cpu().numpy() for i, o in enumerate(outs)}
    got["grad_features"] = x.grad.cpu().numpy()
    for key, p in m.named_parameters():
        assert p.grad is not None, key
        got["grad " + tf_name(key)] = p.grad.cpu().numpy()
    for key, b in buffers.items():
        if training:
            got["update " + tf_name(key)] = b.cpu().numpy()
        else:
            assert torch.equal(b, before[key]), "inference mode wrote " + key
    return got


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("name", sorted(CASES))
def test_blocks(name, training):
    check_block(name, training)


def check_block(name, training, source="device"):
    import copy
    pyr, host = pyramid(300, 2, DL0, source=source)
    n0, n1 = host["points"][0].shape[0], host["points"][1].shape[0]
    assert 250 <= n0 and 8 <= n1 < n0
    assert (host["neighbors"][0] == n0).any() and (host["pools"][0] == n0).any()      # real shadow entries in both tables
    seed, m, variables, f, go = prepared(name, training, source)
    ref64 = O.evaluate(oracle_build(name, host), variables, host, f, go, torch.float64, training)
    ref32 = O.evaluate(oracle_build(name, host), variables, host, f, go, torch.float32, training)
    assert ref64["guarded"], "bad seed %d: |z| %.2e, gap %.2e" % (seed, ref64["min_abs_z"], ref64["min_gap"])
    assert ref64["used"] == set(variables), sorted(ref64["used"] ^ set(variables))    # every variable of the module is one of the graph's, by name
    got = run_module(copy.deepcopy(m), pyr, f, [go], training, "cuda" if source == "device" else "cpu")
    worst = compare(got, ref64, ref32, name)
    print("%s, %s, seed %d: device error / (4 x fp32 oracle error) %.3f" % (name, "training" if training else "inference", seed, worst))


def test_local_aggregation_options_and_refusals():
    from contrastboundary_amd import convnet_blocks as B
    with pytest.raises(NotImplementedError):
        B.LocalAggregation(24, 24, "attention_point")
    with pytest.raises(NotImplementedError):
        B.LocalAggregation(24, 24, "other")
    with pytest.raises(TypeError):
        B.LocalAggregation(24, 24, "pospool", no_such_option=1)
    with pytest.raises(NotImplementedError):
        B.LocalAggregation(24, 24, "pospool", position_embedding="other")
    with pytest.raises(ValueError):
        B.LocalAggregation(24, 24, "pseudo_grid")                    # no kernel points
    assert B.LocalAggregation(24, 24, "adaptive_weight").output_conv is None
    assert B.LocalAggregation(24, 24, "adaptive_weight", output_conv=True).output_conv is not None
    assert B.LocalAggregation(24, 24, "identity").pool_bn is not None and B.LocalAggregation(24, 48, "identity").pool_bn is None
    la = B.LocalAggregation(24, 24, "pseudo_grid", kernel_points=torch.from_numpy(kernel_points()))
    assert la.tf_scopes()["aggregator.weights"] == "local_aggregation" and la.tf_scopes()["pool_bn.gamma"] == "local_aggregation/bn"
    assert "aggregator.kernel_points" not in la.state_dict()
    pyr, _ = pyramid(300, 2, DL0)
    with pytest.raises(TypeError):                                   # CPU features: the first operator that meets them raises (its _chk)
        B.LocalAggregation(24, 24, "adaptive_weight").cuda()(pyr["points"][0], pyr["points"][0], pyr["neighbors"][0], torch.zeros(pyr["points"][0].shape[0], 24), R0)


# ---------------------------------------------------------------------------------------------------------------- the backbone
BB = dict(n=2000, dl0=0.04, in_fdim=4, base_fdim=8, ratio=2, depth=1, layers=5)


def backbone_scopes():
    """the reference's tf.variable_scope nesting for depth 1, five layers, adaptive_weight (shipped options: fc_num 1 -> 'fc_1'), read off resnet.py:340-420,
    :127-183, :235-296, local_aggregation_operators.py:316-500 and basic_operators.py:223-235 BY HAND: TF variable name -> shape"""
    names = {}

    def conv(scope, cin, cout):
        names[scope + "/weights"] = (cin, cout)
        for v in ("gamma", "beta", "moving_mean", "moving_variance"):
            names[scope + "/bn/" + v] = (cout,)

    def aggregation(scope, c):
        names[scope + "/fc_1/weights"] = (3, c)
        names[scope + "/fc_1/biases"] = (c,)
        for v in ("gamma", "beta", "moving_mean", "moving_variance"):
            names[scope + "/pool_bn/" + v] = (c,)

    def block(scope, cin, cout):
        conv(scope + "/conv1/conv1d_1x1", cin, cout // 2)
        aggregation(scope + "/conv2/local_aggregation", cout // 2)
        conv(scope + "/conv3/conv1d_1x1", cout // 2, cout)
        if cin != cout:
            conv(scope + "/shortcut/conv1d_1x1", cin, cout)

    conv("resnet_backbone/res1_input_conv", 4, 8)
    aggregation("resnet_backbone/res1_simple_block/local_aggreagtion", 8)
    block("resnet_backbone/res1_bottleneck0", 8, 16)
    block("resnet_backbone/res2_strided_bottleneck", 16, 32)
    block("resnet_backbone/res2_bottleneck0", 32, 32)
    block("resnet_backbone/res3_strided_bottleneck", 32, 64)
    block("resnet_backbone/res3_bottleneck0", 64, 64)
    block("resnet_backbone/res4_strided_bottleneck", 64, 128)
    block("resnet_backbone/res4_bottleneck0", 128, 128)
    block("resnet_backbone/res5_strided_bottleneck", 128, 256)
    block("resnet_backbone/res5_bottleneck0", 256, 256)
    return names


def build_backbone(seed):
    from contrastboundary_amd import convnet_blocks as B
    torch.manual_seed(seed)
    m = B.ResnetBackbone(BB["in_fdim"], BB["dl0"] * DENSITY / 2, BB["base_fdim"], BB["ratio"], BB["depth"], dict(kind="adaptive_weight"), num_layers=BB["layers"])
    O.randomize_(m, seed)
    return m


def backbone_oracle(host):
    return lambda g, f: O.resnet_backbone(g, dict(kind="adaptive_weight"), host, f, BB["dl0"] * DENSITY / 2, BB["base_fdim"], BB["ratio"], BB["depth"], BB["layers"])


# the first two seeds the float64 oracle guards on this pyramid (python -m tests.test_gpu_convnet_blocks on a machine with the device: the pyramid is built
# there; the search itself runs on the CPU).  About one seed in fifty passes: the backbone has some 250 000 pre-activations and 10 000 maxima.  Every
# backbone test asserts the guard again
BACKBONE_SEEDS = (42, 44)


def backbone_case(seed, host, training=True):
    """inference: the moving statistics are the batch statistics of these features (one float64 training pass of the oracle with momentum 0, stored as
    float32) — a network that has been trained; with arbitrary moving statistics the activations of a five-stage network drift to scales at which an
    absolute guard band holds for no seed (none of 3000 tried)"""
    sizes = [p.shape[0] for p in host["points"]]
    widths = [2 ** (l + 1) * BB["base_fdim"] for l in range(BB["layers"])]
    m = build_backbone(seed)
    rng = np.random.default_rng(2000 + seed)
    f = rng.normal(size=(sizes[0], BB["in_fdim"])).astype(np.float32)
    gos = [rng.normal(size=(n, w)).astype(np.float32) for n, w in zip(sizes, widths)]
    if not training:
        batch = O.evaluate(backbone_oracle(host), O.tf_variables(m), host, f, gos, training=True, backward=False, bn_momentum=0.0)["updates"]
        scopes = m.tf_scopes()
        state = m.state_dict()
        with torch.no_grad():
            for key in state:
                name = scopes[key] + "/" + key.rsplit(".", 1)[-1]
                if name in batch:
                    state[key].copy_(torch.from_numpy(batch[name]))
    return m, O.tf_variables(m), f, gos


def find_backbone_seeds(count=2, seeds=range(4000), source="device"):
    _, host = pyramid(BB["n"], BB["layers"], BB["dl0"], clustered=True, source=source)
    found = []
    for seed in seeds:
        m, variables, f, gos = backbone_case(seed, host)
        if O.evaluate(backbone_oracle(host), variables, host, f, gos, training=True, backward=False)["guarded"]:
            found.append(seed)
            if len(found) == count:
                return tuple(found)
    raise AssertionError("no flip-free seed")


@functools.lru_cache(maxsize=None)
def backbone_prepared(training=True, source="device"):
    _, host = pyramid(BB["n"], BB["layers"], BB["dl0"], clustered=True, source=source)
    for seed in BACKBONE_SEEDS:                                      # (found in training mode; inference sees the same activations up to float32 statistics)
        case = backbone_case(seed, host, training)
        if O.evaluate(backbone_oracle(host), case[1], host, case[2], case[3], training=training, backward=False)["guarded"]:
            return (seed,) + case
    raise AssertionError("bad seeds: none of %s is flip-free on this pyramid" % (BACKBONE_SEEDS,))


def test_backbone_names_every_variable_once_under_the_references_scopes():
    m = build_backbone(0)
    scopes = m.tf_scopes()
    state = m.state_dict()
    assert set(scopes) == set(state) and len(state) == len(list(m.named_parameters())) + len(list(m.named_buffers()))
    named = {scopes[k] + "/" + k.rsplit(".", 1)[-1]: tuple(v.shape) for k, v in state.items()}
    assert len(named) == len(state)                                  # no two variables share a TF name
    assert named == backbone_scopes()
    from contrastboundary_amd import convnet_blocks as B
    deep = B.ResnetBackbone(4, 0.1, 8, 2, 1, dict(kind="adaptive_weight"), num_layers=7)
    assert [deep.res6_strided_bottleneck.radius, deep.res6_bottleneck0.radius, deep.res7_strided_bottleneck.radius, deep.res7_bottleneck0.radius] == \
        pytest.approx([16 * 0.1, 25 * 0.1, 25 * 0.1, 36 * 0.1])      # (layer_idx - 1)^2 and layer_idx^2 times the base radius (resnet.py:429, :436)
    assert deep.res7_bottleneck0.conv3.weights.shape[1] == 2 ** 7 * 8
    with pytest.raises(NotImplementedError):
        B.ResnetBackbone(4, 0.1, 8, 2, 1, dict(kind="adaptive_weight"), num_layers=4)


@pytest.mark.parametrize("training", [True, False])
def test_backbone(training):
    check_backbone(training)


def check_backbone(training, source="device"):
    import copy
    pyr, host = pyramid(BB["n"], BB["layers"], BB["dl0"], clustered=True, source=source)
    sizes = [p.shape[0] for p in host["points"]]
    print("backbone layer sizes", sizes)
    assert len(sizes) == 5 and min(sizes) >= 8, sizes
    seed, m, variables, f, gos = backbone_prepared(training, source)
    ref64 = O.evaluate(backbone_oracle(host), variables, host, f, gos, torch.float64, training)
    ref32 = O.evaluate(backbone_oracle(host), variables, host, f, gos, torch.float32, training)
    assert ref64["guarded"] and ref64["used"] == set(variables)
    assert [o.shape for o in ref64["out"]] == [(n, 2 ** (l + 1) * 8) for l, n in enumerate(sizes)]
    got = run_module(copy.deepcopy(m), pyr, f, gos, training, "cuda" if source == "device" else "cpu")
    worst = compare(got, ref64, ref32, "backbone")
    print("backbone, %s, seed %d: device error / (4 x fp32 oracle error) %.3f" % ("training" if training else "inference", seed, worst))


def test_two_training_steps_from_one_state_give_the_same_bits():
    import copy
    from contrastboundary_amd import neighbor_state
    pyr, host = pyramid(BB["n"], BB["layers"], BB["dl0"], clustered=True)
    seed, m, variables, f, gos = backbone_prepared()
    with neighbor_state.deterministic():
        a = _run_module(copy.deepcopy(m), pyr, f, gos, True)
        b = _run_module(copy.deepcopy(m), pyr, f, gos, True)
    for key in a:
        np.testing.assert_array_equal(a[key].view(np.uint32), b[key].view(np.uint32), err_msg=key)


if __name__ == "__main__":                                           # BACKBONE_SEEDS
    print("BACKBONE_SEEDS", find_backbone_seeds())
