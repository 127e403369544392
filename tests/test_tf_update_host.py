"""CPU: the TF-side update kernels (contrastboundary_amd/csrc/tf_update.hip: cbl_tf_update_plan, cbl_tf_weight_loss_*, cbl_tf_clip_update) compiled for the
HOST with wave semantics (tests/host_emul) against the float64 restatement of the reference's update (tests/tf_update_oracle.py; parity unpinned by
execution — TF absent), within the derived bounds of that module: the segment sizes around the vector width, the wave and the chunk in ONE buffer whose
first segment begins one element behind an aligned base, each size alone, buffers that disagree modulo 16 bytes, every mode bit with fold_decay on and off,
the pinned gradient norms, idle segments, a launch past the workgroup cap, determinism, and the documented error codes — those also on the DEVICE build of
the library, whose argument checks come before any launch and need no GPU.  Written outputs are pre-filled with NaN.  A stand-alone AddressSanitizer program
(tests/host_emul/tf_update_asan_main.cpp: its own main, no Python) runs the edge layouts in heap buffers of exactly `total` elements."""
import ctypes

import numpy as np
import pytest

from tests import tf_update_oracle as O
from tests.host_emul.host_build import P, aligned, load, run_sanitizer_program, sanitizer_program


@pytest.fixture(scope="module")
def drv():
    return O.Driver(load("tf_update", ["tf_update"]), lambda a, off=0: aligned(a, 4 * off), lambda x: np.array(x, copy=True), P)


@pytest.fixture(scope="module")
def edge(drv):
    case = O.edge_case()
    return case, drv.layout(case)


def test_plan_lists_every_chunk_of_every_segment(drv):
    case = O.edge_case()
    rc, plan, n = drv.plan(case["total"], case["begin"])
    assert rc == 0 and n == 7 + 1 + 2 + 3                            # seven sizes below a chunk, one chunk, one chunk + 1, two chunks + 5
    assert list(plan[:11]) == [0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 13]
    assert (plan[11 + n:] == -1).all()


def test_every_mode_on_the_edge_buffer(drv):
    O.check_all_modes(drv, O.edge_case(), "edge buffer")


@pytest.mark.parametrize("size", O.EDGE_SIZES)
def test_every_mode_on_one_segment(drv, size):
    O.check_all_modes(drv, O.make_case([size], 100 + size, wd=[0.05]), "S = 1, %d" % size)


@pytest.mark.parametrize("off", [(0, 1, 0), (0, 0, 2), (3, 3, 3)])
def test_buffers_that_disagree_modulo_16_bytes(drv, edge, off):
    case, lay = edge
    for mode, fold in ((O.CLIP | O.STEP, 1), (O.CLIP, 0), (O.STEP, 0)):
        O.check_update(drv, case, lay, mode, fold, off=off, what="bases at %s" % (off,))


def test_weight_loss_value_terms_gradient_and_unread_segments(drv, edge):
    O.check_weight_loss(drv, *edge)
    case = O.make_case([O.CHUNK + 1], 3, wd=[0.3])
    O.check_weight_loss(drv, case, drv.layout(case))


def test_pinned_gradient_norms(drv, edge):
    O.check_pinned_norms(drv, *edge)


def test_idle_segments_keep_value_and_momentum(drv, edge):
    O.check_inactive(drv, *edge, idle={0, 7, 9})


def test_two_calls_give_the_same_bits(drv, edge):
    O.check_deterministic(drv, *edge)


def test_one_chunk_more_than_the_launch_cap(drv):
    """4096 waves at most per launch: 4097 chunks (one segment of 4096 chunks + 1 element behind a segment of 3) make the last wave-trip a second one"""
    case = O.make_case([3, O.CAP_CHUNKS * O.CHUNK - O.CHUNK + 1], 11, wd=[0.0, 0.02])
    lay = drv.layout(case)
    assert lay["nc"].value == O.CAP_CHUNKS + 1
    O.check_update(drv, case, lay, O.CLIP | O.STEP, 1, clip_norm=100.0, what="past the cap")
    O.check_weight_loss(drv, case, lay)


def test_a_plan_of_another_layout_touches_nothing_outside(drv):
    """chunks the device's seg_begin does not bear out are skipped: the plan of a LONGER layout over a shorter buffer writes nothing outside [0, total)"""
    small, big = O.make_case([5, 70], 5), O.make_case([3 * O.CHUNK, 5], 5)
    lay = drv.layout(big)
    lay.update(total=ctypes.c_longlong(small["total"]), S=ctypes.c_longlong(2), begin=drv.put(small["begin"]))
    lay["nc"] = ctypes.c_longlong(2)                                 # what the entry accepts for this total; the plan's chunk 1 is segment 0's SECOND
    w, g, a, _ = drv.clip_update(small, lay, O.CLIP | O.STEP, 0)
    assert np.isfinite(w).all() and np.isfinite(g).all() and np.isfinite(a).all()
    b = int(small["begin"][1])
    assert np.array_equal(w[b:], small["params"][b:]) and np.array_equal(w[:1], small["params"][:1])      # segment 1 has no chunk in that plan


def test_bad_arguments_host_build(drv):
    O.check_arguments(drv.L)


def test_bad_arguments_device_build_without_a_gpu():
    from contrastboundary_amd import _lib
    O.check_arguments(_lib.lib())


def test_sanitizer_program_over_the_edge_layouts():
    r = run_sanitizer_program(sanitizer_program("tf_update", ["tf_update"]))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "cases ok" in r.stdout
