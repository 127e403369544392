"""CPU: the q / k / v projections of the WIDE attention stages (C = 128 | 256 | 512: cbl_triple_linear_forward / _backward, the tiled MFMA kernels of
contrastboundary_amd/csrc/skinny_linear.hip) compiled for the HOST and run with wave semantics (tests/host_emul/wave: v_mfma_f32_16x16x4_f32 as a rendezvous of
the wave's fibres), through the C entry points on numpy buffers, against numpy in float64.

Bounds: those of tests/test_attention_host.py::test_three_projections_in_one_launch — largest absolute error <= 1e-5 of the largest reference element for y,
grad_x, grad_weight and grad_bias.  (A numpy model of the MFMA chain — contraction walked four at a time, fp32 running sum — gives 2e-7 .. 1.3e-6 on that
measure at the real stage shapes; an indexing error is orders of magnitude outside it.)

Every MFMA is a rendezvous of 64 fibres and 3 rows C^2 / 1024 of them run per direction, so the rows stay small at C = 512; the real stage shapes run on the
GPU (tests/test_gpu_triple_linear_wide.py)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "contrastboundary_amd", "csrc")
EMUL = os.path.join(HERE, "host_emul", "wave")
GEN = os.path.join(HERE, "host_emul", "host_tu.py")
BUILD = os.path.join(ROOT, "oracle", "_build")

RED = 4096                                                          # bytes behind the workspace that must stay untouched
TOL = 1e-5


def _codes():
    """the CBL_ERR_* values of include/cbl_amd.h"""
    import re
    text = open(os.path.join(ROOT, "include", "cbl_amd.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(CBL_ERR_\w+)\s+\(?(-?\d+)\)?", text)}


def build_host(name, extra=()):
    src = os.path.join(CSRC, "skinny_linear.hip")
    tu, so = os.path.join(BUILD, name + ".cpp"), os.path.join(BUILD, "lib" + name + ".so")
    deps = [src, GEN, os.path.join(CSRC, "cbl_common.h"), os.path.join(EMUL, "amdgcn.h"), os.path.join(EMUL, "hip", "hip_runtime.h")]
    os.makedirs(BUILD, exist_ok=True)
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call([sys.executable, GEN, tu, src])
        subprocess.check_call(["g++", "-x", "c++", "-std=c++17", "-O1", *extra, "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unknown-pragmas",
                               "-I" + EMUL, "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, tu, "-o", so])
    return so


def load(so):
    L = ctypes.CDLL(so)
    L.cbl_triple_linear_workspace_bytes.restype = ctypes.c_size_t
    return L


@pytest.fixture(scope="module")
def host():
    return load(build_host("triple_linear_wide_host"))


def P(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def arr(xs):
    a = (ctypes.c_void_p * 3)()
    for i, v in enumerate(xs):
        a[i] = None if v is None else v.ctypes.data
    return a


def err(got, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max()) / max(float(np.abs(ref).max()), 1e-30)


def run_case(L, rows, C, null_bias=None, grad_bias="all", check=True):
    """one forward + backward call on fresh NaN-filled outputs; null_bias: index of a bias3 entry passed as NULL; grad_bias: "all" | "none" (the array is
    NULL) | an index (that entry is NULL).  Returns every output (for the bit-for-bit comparison of two calls)."""
    rng = np.random.default_rng(1000 * C + rows)
    x = rng.normal(size=(rows, C)).astype(np.float32)
    W = [(rng.normal(size=(C, C)) / np.sqrt(C)).astype(np.float32) for _ in range(3)]
    b = [rng.normal(size=C).astype(np.float32) for _ in range(3)]
    gy = [rng.normal(size=(rows, C)).astype(np.float32) for _ in range(3)]
    b_in = [None if p == null_bias else b[p] for p in range(3)]
    y = [np.full((rows, C), np.nan, np.float32) for _ in range(3)]
    R = ctypes.c_longlong(rows)
    assert L.cbl_triple_linear_forward(R, C, P(x), arr(W), arr(b_in), arr(y), None) == 0
    gx, gW = np.full((rows, C), np.nan, np.float32), [np.full((C, C), np.nan, np.float32) for _ in range(3)]
    gb = [None if (grad_bias == "none" or grad_bias == p) else np.full(C, np.nan, np.float32) for p in range(3)]
    nbytes = L.cbl_triple_linear_workspace_bytes(C)
    assert 0 < nbytes <= 64 << 20                                   # tens of megabytes at most, whatever the number of rows
    ws = np.full(nbytes + RED, 0xA5, np.uint8)
    gb_arg = None if grad_bias == "none" else arr(gb)
    assert L.cbl_triple_linear_backward(R, C, P(x), arr(W), arr(gy), P(gx), arr(gW), gb_arg, P(ws), ctypes.c_size_t(nbytes), None) == 0
    assert np.all(ws[nbytes:] == 0xA5), "the workspace's red zone was written"
    if check:
        x64 = x.astype(np.float64)
        figures = {}
        for p in range(3):
            figures["y%d" % p] = err(y[p], x64 @ W[p].astype(np.float64).T + (0.0 if b_in[p] is None else b[p].astype(np.float64)))
            figures["gW%d" % p] = err(gW[p], gy[p].astype(np.float64).T @ x64)
            if gb[p] is not None:
                figures["gb%d" % p] = err(gb[p], gy[p].astype(np.float64).sum(0))
        figures["gx"] = err(gx, sum(gy[p].astype(np.float64) @ W[p].astype(np.float64) for p in range(3)))
        print("rows %d C %d: %s" % (rows, C, ", ".join("%s %.2e" % kv for kv in sorted(figures.items()))))
        bad = {k: v for k, v in figures.items() if not v <= TOL}     # (a NaN left in an output fails the comparison)
        assert not bad, bad
    return y + [gx] + gW + [g for g in gb if g is not None]


# rows: 1, around one 16-row tile, no multiple of any tile edge (16 / 32 / 64 rows per workgroup, 64-row panels of the weight gradient), and one per width whose weight gradient takes more than one
# row chunk (> 128 rows, > 256 at C = 512: partials + the combine kernel).  The entries give a workgroup 32 or 64 rows once that still leaves ~240 workgroups: at C = 128 that is
# 1300 rows (32 for both directions) and 2563 (64), cheap enough for the emulator (48 MFMAs per row and direction).
CASES = [(1, 128), (15, 128), (16, 128), (17, 128), (77, 128), (333, 128), (1300, 128), (2563, 128),
         (1, 256), (15, 256), (16, 256), (17, 256), (45, 256), (200, 256),
         (1, 512), (15, 512), (16, 512), (17, 512), (37, 512), (150, 512), (260, 512)]


@pytest.mark.parametrize("rows,C", CASES)
def test_wide_projections_forward_and_gradients(host, rows, C):
    run_case(host, rows, C)


@pytest.mark.parametrize("null_bias,grad_bias", [(1, "all"), (None, "none"), (None, 2), (0, 0)])
def test_null_bias_variants(host, null_bias, grad_bias):
    run_case(host, 50, 128, null_bias=null_bias, grad_bias=grad_bias)
    run_case(host, 150, 128, null_bias=null_bias, grad_bias=grad_bias)       # two row chunks: the combine kernel's NULL handling


@pytest.mark.parametrize("rows,C", [(150, 128), (40, 256), (20, 512)])
def test_two_calls_give_identical_bits(host, rows, C):
    a = run_case(host, rows, C, check=False)
    b = run_case(host, rows, C, check=False)
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()


def test_unsupported_widths_and_short_workspace(host):
    codes = _codes()
    rows = 4
    for C in (96, 1024):
        x = np.zeros((rows, C), np.float32)
        W = [np.zeros((C, C), np.float32) for _ in range(3)]
        y = [np.zeros((rows, C), np.float32) for _ in range(3)]
        assert host.cbl_triple_linear_workspace_bytes(C) == 0
        assert host.cbl_triple_linear_forward(ctypes.c_longlong(rows), C, P(x), arr(W), None, arr(y), None) == codes["CBL_ERR_UNSUPPORTED"]
        ws = np.zeros(64, np.uint8)
        assert host.cbl_triple_linear_backward(ctypes.c_longlong(rows), C, P(x), arr(W), arr(y), P(x.copy()), arr(W), None, P(ws), ctypes.c_size_t(64),
                                               None) == codes["CBL_ERR_UNSUPPORTED"]
    for C in (128, 256, 512):
        x = np.zeros((rows, C), np.float32)
        W = [np.zeros((C, C), np.float32) for _ in range(3)]
        gy = [np.zeros((rows, C), np.float32) for _ in range(3)]
        gW = [np.full((C, C), np.nan, np.float32) for _ in range(3)]
        gx = np.full((rows, C), np.nan, np.float32)
        nbytes = host.cbl_triple_linear_workspace_bytes(C)
        ws = np.zeros(nbytes, np.uint8)
        assert host.cbl_triple_linear_backward(ctypes.c_longlong(rows), C, P(x), arr(W), arr(gy), P(gx), arr(gW), None, P(ws), ctypes.c_size_t(nbytes - 1),
                                               None) == codes["CBL_ERR_WORKSPACE"]
        assert np.isnan(gx).all() and all(np.isnan(g).all() for g in gW)     # refused before anything ran


@pytest.mark.skipif(not os.environ.get("CBL_HOST_EMUL_FULL"), reason="a second (sanitizer) build of the host library: set CBL_HOST_EMUL_FULL=1")
def test_wide_kernels_under_address_sanitizer(tmp_path):
    """The same host build with -fsanitize=address in a subprocess (libasan first): the operands are numpy buffers of exactly rows x C floats, so a tile that reads
    or writes past the last row — clamped loads, masked stores, the zero-filled rows of the weight gradient's last panel — is a reported heap overflow."""
    asan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not asan or not os.path.isabs(asan) or not os.path.exists(asan):
        pytest.skip("no libasan beside gcc")
    so = build_host("triple_linear_wide_host_asan", extra=("-g", "-fsanitize=address"))
    script = tmp_path / "run.py"
    script.write_text(
        "import sys\n"
        "sys.path.insert(0, %r)\n"
        "import tests.test_triple_linear_wide_host as T\n"
        "L = T.load(%r)\n"
        "for rows, C in ((1, 128), (17, 128), (77, 128), (161, 128), (17, 256), (45, 256), (1, 512), (17, 512)):\n"
        "    T.run_case(L, rows, C)\n"
        "T.run_case(L, 150, 128, null_bias=1, grad_bias=2)\n"
        "print('ASAN_RUN_DONE')\n" % (ROOT, so))
    env = dict(os.environ, LD_PRELOAD=asan, ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0")
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=1800, env=env)
    assert "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and "ASAN_RUN_DONE" in r.stdout, (r.returncode, r.stderr[-2000:])
