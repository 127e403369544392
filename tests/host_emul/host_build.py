"""TEST INFRASTRUCTURE: the one builder of the host-emulation libraries the tests/test_*_host.py files load — some of OUR kernel files
(contrastboundary_amd/csrc/<file>.hip) compiled for the HOST with wave semantics (tests/host_emul/wave), one translation unit (host_tu.py) and one object per
kernel file as in the product build, linked into oracle/_build/host/lib<name>.so.  What an object depends on is derived here, never listed by a caller; an
object is shared by every library that names its file.  Beside it the array helpers those tests share.  Importing this module does nothing (standard library
and numpy only).  tests/host_emul/full_library.py keeps its own copy of the build recipe for the whole library: the address-sanitized tests that drive it stay
as they are."""
import ctypes
import functools
import glob
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "contrastboundary_amd", "csrc")
EMUL = os.path.join(HERE, "wave")
GEN = os.path.join(HERE, "host_tu.py")
HEADER = os.path.join(ROOT, "include", "cbl_amd.h")
BUILD = os.path.join(ROOT, "oracle", "_build", "host")
INCLUDES = ["-I" + EMUL, "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]


def dependencies(files):
    """everything a host build of csrc/<file>.hip, file in files, reads: those sources, every csrc/*.h, the C header, the whole emulator tree, the generator
    and this module"""
    deps = [os.path.join(CSRC, f + ".hip") for f in files] + sorted(glob.glob(os.path.join(CSRC, "*.h"))) + [HEADER, GEN, os.path.abspath(__file__)]
    return deps + [os.path.join(d, f) for d, _, fs in os.walk(EMUL) for f in fs]


def stale(target, deps):
    return not os.path.exists(target) or os.path.getmtime(target) < max(os.path.getmtime(d) for d in deps)


def _replaced(target, command):
    """run command with a temporary name in the place of its None, then rename that file to target: an interrupted build leaves nothing the stale check
    would accept"""
    os.makedirs(BUILD, exist_ok=True)
    tmp = "%s.%d.tmp" % (target, os.getpid())
    try:
        subprocess.check_call([tmp if c is None else c for c in command])
        os.replace(tmp, target)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return target


def _stem(file, whole):
    return os.path.join(BUILD, file + ("_whole" if whole else "") + "_host")


def translation_unit(file, whole=False):
    """-> path of the generated .cpp of csrc/<file>.hip (whole: through host_tu.py --whole, under a name of its own)"""
    tu = _stem(file, whole) + ".cpp"
    if stale(tu, dependencies([file])):
        _replaced(tu, [sys.executable, GEN] + (["--whole"] if whole else []) + [None, os.path.join(CSRC, file + ".hip")])
    return tu


def _object(file, whole):
    obj = _stem(file, whole) + ".o"
    if stale(obj, dependencies([file])):
        tu = translation_unit(file, whole)
        _replaced(obj, ["g++", "-x", "c++", "-std=c++17", "-O1", "-fPIC", "-c", "-ffp-contract=off", "-Wno-unknown-pragmas"] + INCLUDES + [tu, "-o", None])
    return obj


def objects(files, whole=()):
    """-> one object per kernel file (those in `whole` with the sections their older host build leaves out), rebuilt where stale, compiled side by side"""
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        return list(pool.map(lambda f: _object(f, f in whole), files))


def library(name, files, whole=()):
    """-> path of oracle/_build/host/lib<name>.so, linked again when one of its objects is newer or when it was linked from another list of objects (the
    list is kept beside it)"""
    so, objs = os.path.join(BUILD, "lib%s.so" % name), objects(files, whole)
    listing, linked = so + ".objects", "\n".join(objs)
    if stale(so, objs) or not os.path.exists(listing) or open(listing).read() != linked:
        _replaced(so, ["g++", "-shared"] + objs + ["-o", None])
        with open(listing, "w") as f:
            f.write(linked)
    return so


def sanitizer_program(name, files, beside=False):
    """-> path of the STAND-ALONE program oracle/_build/host/<name>_asan, rebuilt where stale: tests/host_emul/<name>_asan_main.cpp (its main; asan_common.h) and
    the host translation units of `files` under -fsanitize=address,undefined.  The main includes its unit by name (found through -I), or — beside — the units
    are compiled beside it.  Nothing of this is ever loaded into Python"""
    main, exe = os.path.join(HERE, name + "_asan_main.cpp"), os.path.join(BUILD, name + "_asan")
    tus = [translation_unit(f) for f in files]
    if stale(exe, dependencies(files) + tus + [main, os.path.join(HERE, "asan_common.h")]):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
                               "-Wno-unknown-pragmas"] + INCLUDES + (["-x", "c++", main] + tus if beside else ["-I" + BUILD, main]) + ["-o", exe])
    return exe


def run_sanitizer_program(exe):
    """-> its subprocess.CompletedProcess (the emulator keeps its fibre stacks for the life of the process: no leak report)"""
    return subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))


@functools.lru_cache(maxsize=None)
def _size_t_names():
    """the functions include/cbl_amd.h declares with a name ending in _bytes, read as contrastboundary_amd/_lib.py declared_symbols reads them"""
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(cbl_\w+_bytes)\s*\(", txt)))


def size_t_results(L):
    """restype = c_size_t on every such function that L exports (ctypes' default, int, truncates them).  -> L"""
    for name in _size_t_names():
        if hasattr(L, name):
            getattr(L, name).restype = ctypes.c_size_t
    return L


def load(name, files, whole=()):
    """-> the library of those kernel files as a ctypes.CDLL, its size_t results set"""
    return size_t_results(ctypes.CDLL(library(name, files, whole)))


def P(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def aligned(a, off=0):
    """a copy of `a` whose data pointer is 16-byte aligned (feature rows are read as float4; off = 4: deliberately not)"""
    a = np.ascontiguousarray(a)
    raw = np.zeros(a.nbytes + 32, np.uint8)
    o = (-raw.ctypes.data) % 16 + off
    out = raw[o:o + a.nbytes].view(a.dtype).reshape(a.shape)
    out[...] = a
    return out


def nans(*shape):
    return aligned(np.full(shape, np.nan, np.float32))


def transposed_table(idx, n0):
    """cbl_neighbor_transpose's output, restated: for every target row t < n0 the ascending list of the pairs p = i * K + k whose neighbour is t (CSR: inv_start (n0 + 1),
    inv_src); shadow neighbours (== n0) are in no list"""
    flat = idx.reshape(-1)
    keep = np.nonzero(flat < n0)[0]
    order = np.argsort(flat[keep], kind="stable")
    inv_src = keep[order].astype(np.int32)
    inv_start = np.zeros(n0 + 1, np.int32)
    np.add.at(inv_start, flat[keep] + 1, 1)
    return np.cumsum(inv_start).astype(np.int32), inv_src
