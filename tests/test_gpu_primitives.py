"""The device arithmetic primitives — exp_neg / exp_pair and their table, gauss_record / gauss_logw, the double-double
helpers of the resampling, small_div, the weight bins, the fixed-order reductions and scans, the 3 x 3 algebra — each called
by k_test_primitive (phd_test_primitive) on the inputs of tests/primitive_cases.py and held to that module's reference with
its derived bound: multi-precision or exact rational arithmetic where a bound is claimed, a numpy transcription of the stated
order where the claim is bit equality. The whole-kernel tests see these functions through 1e-9 .. 1e-6; here a table entry
off by 1e-12, a lost pragma or a changed order of additions fails. The kernel calls the very functions the step kernels
call; what is pinned is their source (constants, pragmas, inline assembly, order), not the instructions they become inside
another kernel. tests/test_primitive_refs.py runs the same checks on host transcriptions, without a GPU."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import primitive_cases as pc
from monorfs_amd.abi import prm3d_defaults


@pytest.fixture(scope="module")
def nav():
    from monorfs_amd import navigator
    p = prm3d_defaults(max_particles=4, max_components=600, max_measurements=8)
    n = navigator.PHDNavigator(p, particlecount=4)
    yield n
    n.close()


@pytest.fixture(scope="module")
def run(nav):
    return nav.test_primitive


def test_exp_table(run):
    print("exp table: the largest error of an entry is %.3f ulp" % pc.check_exp_table(run))


def test_exp_neg(run):
    """Measured on an MI355X: see the comment of exp_neg in phd_device.h and DESIGN.md, "Device primitives"."""
    rel, at, part = pc.check_exp(run, pair=False)
    print("exp_neg: max relative error %.4g at x = %r (%.3f of E_NEG = %.4g)" % (rel, at, part, pc.E_NEG))


def test_exp_pair(run):
    rel, at, part = pc.check_exp(run, pair=True)
    print("exp_pair: max relative error %.4g at x = %r (%.3f of its bound)" % (rel, at, part))
    pc.check_exp_pair_dropped(run)


def test_gauss_record(run):
    print("gauss_record: g9 at %.3f of its bound" % pc.check_gauss_record(run))


def test_gauss_logw_and_density(run):
    print("gauss_logw at %.3f of its bound, exp_pair(gauss_logw) at %.3f" % pc.check_gauss_logw(run))


def test_double_double(run):
    pc.check_two_sum(run, quick=False)
    pc.check_two_sum(run, quick=True)
    pc.check_two_sum_of_product(run)
    print("dd_add %.3f, dd_add_d %.3f of their bounds" % (pc.check_dd_add(run), pc.check_dd_add_d(run)))
    print("dd_wave_scan %.3f (64 lanes), %.3f (16); slot_target %.3f" % (pc.check_dd_scan(run, 64), pc.check_dd_scan(run, 16), pc.check_slot_target(run)))


def test_small_div(run):
    pc.check_small_div(run)


@pytest.mark.parametrize("minw", pc.bin_min_weights(), ids=["defaults", "small_minw", "small_minw_wide", "large_minw"])
def test_weight_bins(run, minw):
    pc.check_weight_bins(run, minw)


def test_reductions_and_scans(run):
    pc.check_sums(run)
    pc.check_extrema(run)
    pc.check_incl_scan(run)
    pc.check_first_max(run)


def test_algebra3(run):
    pc.check_algebra3(run)


def test_bad_arguments(nav):
    lib, h = nav._lib, nav._h
    buf = np.zeros(64)
    out = np.zeros(64)
    pi, po = buf.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    bad = 1                                            # PHD_ERR_BAD_ARGUMENT
    assert lib.phd_test_primitive(h, 0, pi, 8, po, 8) == bad                               # no such op
    assert lib.phd_test_primitive(h, pc.OP["PT_OPS_END"], pi, 8, po, 8) == bad
    assert lib.phd_test_primitive(h, pc.OP["PT_EXP_NEG"], pi, 12, po, 8) == bad            # no whole records
    assert lib.phd_test_primitive(h, pc.OP["PT_EXP_NEG"], pi, 16, po, 8) == bad            # two in, one out
    assert lib.phd_test_primitive(h, pc.OP["PT_WAVE_SUM"], pi, 64 * 8, po, 64 * 8) == bad  # not a whole workgroup
    assert lib.phd_test_primitive(h, pc.OP["PT_EXP_TAB"], pi, 8, po, 256 * 8) == bad       # takes no input
    assert lib.phd_test_primitive(h, pc.OP["PT_EXP_NEG"], None, 8, po, 8) == bad
    assert lib.phd_test_primitive(h, pc.OP["PT_EXP_NEG"], pi, 8, po, 8) == 0
    assert out[0] == 1.0
