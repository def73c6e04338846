"""The references and bounds of tests/primitive_cases.py, satisfied without a GPU: exp_neg, exp_pair, gauss_logw, the
double-double helpers, slot_target and small_div transcribed in exactly rounded host arithmetic
(tests/primitive_refs_check.cpp; the exponential's table correctly rounded from mpmath) go through the generators and the
assertion functions the device test uses. A bound the transcription cannot keep would be a wrong derivation, found here
and not on a GPU; and the device test is not the first thing that ever ran its own checks. The families whose claim is
bit equality with a numpy transcription (reductions, 3 x 3 algebra, weight bins) have their references checked for what
they must be able to tell apart."""
import os
import subprocess

import numpy as np
import pytest

import primitive_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = tmp_path_factory.mktemp("primitive_refs")
    exe = str(d / "primitive_refs_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "primitive_refs_check.cpp")])
    table = str(d / "table.bin")
    pc.exp_table_reference().tofile(table)
    names = {v: k for k, v in pc.OP.items()}

    def call(op, in_array, out_dtype, out_count):
        src, dst = str(d / "in.bin"), str(d / "out.bin")
        np.ascontiguousarray(in_array).tofile(src)
        subprocess.check_call([exe, names[op], src, dst, table])
        out = np.fromfile(dst, out_dtype)
        assert len(out) == out_count, (names[op], len(out), out_count)
        return out
    return call


def test_op_numbers_follow_the_header():
    assert pc.OP["PT_EXP_NEG"] == 1 and pc.OP["PT_OPS_END"] == len(pc.OP) and len(set(pc.OP.values())) == len(pc.OP)
    text = open(os.path.join(ROOT, "monorfs_amd", "csrc", "phd_primitives_test.h")).read()
    for name in pc.OP:
        if name != "PT_OPS_END":
            assert "case %s:" % name in text, "%s has no case in primitive_layout / k_test_primitive" % name


def test_exp_inputs_hold_what_the_bounds_are_about():
    x = pc.exp_inputs()
    assert 9e4 < len(x) < 1.2e5
    n = np.rint(x[np.isfinite(x)] * 369.3299304675746)
    r = np.abs(x[np.isfinite(x)] - n * 0.0027076061740622863)
    assert np.count_nonzero(r > 0.99999 * np.log(2) / 512) > 8000, "few inputs at the largest reduced argument"
    assert np.isnan(x).any() and np.isneginf(x).any() and (x == -800.0).any() and np.signbit(x[x == 0]).any()


def test_exp_neg_transcription(run):
    rel, at, frac_of_bound = pc.check_exp(run, pair=False)
    print("exp_neg, host transcription with a correctly rounded table: max relative error %.4g at x = %r (%.3f of the bound)" % (rel, at, frac_of_bound))
    assert rel > 1.5 * pc.U, "the inputs never round against the result: nothing is measured"


def test_exp_pair_transcription(run):
    rel, at, frac_of_bound = pc.check_exp(run, pair=True)
    print("exp_pair, host transcription: max relative error %.4g at x = %r (%.3f of the bound)" % (rel, at, frac_of_bound))
    assert frac_of_bound > 0.5, "the bound is far from what the routine does on these inputs: it would not notice a lost term"
    pc.check_exp_pair_dropped(run)


def test_exp_table_reference(run):
    assert pc.check_exp_table(run) <= 0.5


def test_gauss_logw_transcription(run):
    worst_l, worst_d = pc.check_gauss_logw(run)
    print("gauss_logw, host transcription: %.3f of the bound; density %.3f of its bound" % (worst_l, worst_d))


def test_gauss_record_reference():
    """numpy's own log is within the bound the device's is held to"""
    w, m, Pi, mult, _ = pc.gauss_inputs()
    g = pc.numpy_gauss_record(w, m, Pi, mult)

    def numpy_run(op, rec, dtype, count):
        return g.reshape(-1)
    assert pc.check_gauss_record(numpy_run) <= 1.0


def test_double_double_transcriptions(run):
    pc.check_two_sum(run, quick=False)
    pc.check_two_sum(run, quick=True)
    pc.check_two_sum_of_product(run)
    print("dd_add %.3f, dd_add_d %.3f, scans %.3f / %.3f, slot_target %.3f of their bounds" % (
        pc.check_dd_add(run), pc.check_dd_add_d(run), pc.check_dd_scan(run, 64), pc.check_dd_scan(run, 16), pc.check_slot_target(run)))


def test_two_sum_inputs_need_the_slow_form():
    """dd_quick's sequence on the inputs of dd_two_sum (|a| < |b| among them) is NOT error-free: a two_sum that lost a step
    would be seen"""
    a, b = pc.two_sum_inputs()
    s = a + b
    lo = b - (s - a)
    exact = [pc.frac(s[k]) + pc.frac(lo[k]) == pc.frac(a[k]) + pc.frac(b[k]) for k in range(len(a))]
    assert 0 < sum(exact) < len(a) - 500


def test_small_div_transcription(run):
    pc.check_small_div(run)


def test_weight_bin_reference():
    """the integer arithmetic of the bins against the doubles themselves: 32 bins a binade, counted from MinWeight's"""
    for minw in pc.bin_min_weights():
        base = pc.py_bin_base(minw)

        def py_run(op, rec, dtype, count):
            head, body = rec[:1], rec[1:]
            if op == pc.OP["PT_BIN_EDGE"]:
                return np.array([base] + [(base + b) << 47 for b in range(1, 1024)], np.uint64)
            if op == pc.OP["PT_BIN_OF_KEY"]:
                return np.array([pc.py_bin_of_bits(pc.py_prune_key(v), base) for v in body.view(np.float64)], np.int32)
            return np.array([pc.py_bin_of_bits(v, base) for v in body], np.int32)
        pc.check_weight_bins(py_run, minw)
        w = pc.bin_weights(minw)
        inside = w[(w >= minw) & (w < minw * 2.0 ** 31)]
        want = np.floor(32 * np.log2(inside / minw) + 1e-9).astype(int)
        got = np.array([pc.py_bin_of_bits(b, base) for b in pc.bits(inside)])
        assert np.all(np.abs(got - want) <= 3), "a bin is more than three off 32 log2(w / MinWeight) (bins are linear inside a binade: 32 (log2(1 + f) - f) < 2.76)"
    assert len(set(pc.bin_min_weights())) >= 3


def test_order_references_tell_orders_apart():
    """the numpy transcriptions run on themselves: every check's own distinguishing assertions hold"""
    def numpy_run(op, v, dtype, count):
        name = {n: k for k, n in pc.OP.items()}[op]
        if name == "PT_WAVE_SUM":
            return pc.numpy_wave_sum(v)
        if name in ("PT_BLOCK_SUM_256T", "PT_BLOCK_SUM_512", "PT_BLOCK_SUM_1024"):
            return pc.numpy_block_sum(v, {"PT_BLOCK_SUM_256T": 256, "PT_BLOCK_SUM_512": 512, "PT_BLOCK_SUM_1024": 1024}[name])
        if name == "PT_BLOCK_TREE_SUM":
            return pc.numpy_block_tree_sum(v)
        assert name == "PT_BLOCK_SUM_256"
        return ((v[:, 0] + v[:, 1]) + v[:, 2]) + v[:, 3]
    pc.check_sums(numpy_run)
    v = pc.order_sensitive(2048, 0x50A1)
    assert np.any(pc.numpy_block_sum(v, 256) != pc.numpy_block_tree_sum(v)), "the two 256-thread sums agree on this vector"


def test_algebra_reference_differs_from_fused():
    """the unfused inverse differs from one evaluated in higher precision on a good part of the matrices: a build that
    fused the cofactors would not pass bit equality"""
    S, _, _ = pc.matrices3()
    ref = pc.numpy_inv_sym3(S)
    L = S.astype(np.longdouble)
    assert np.count_nonzero(pc.numpy_inv_sym3(L).astype(np.float64)[:, 6] != ref[:, 6]) > len(S) // 10
