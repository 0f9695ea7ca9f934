"""CPU: the exact-arithmetic fixtures of tests/ref_exact_fnet3d.py before any GPU sees them.  On integer operands within the 2^24
budget the float64 statement, the fp32 statement of tests/ref_ops_fnet3d.py and the fp32 statement in another summation order are
bit-equal; the case tables of the GPU module run through the fp32 statements at reduced size; and the comparison helper the GPU
tests use reports a zeroed tap, dropped input channels and a weight gradient that skips its last 32 voxels."""

import pytest
import torch

from tests import ref_exact_fnet3d as X
from tests import ref_ops_fnet3d as R

CPU = torch.device("cpu")


def _fp32_conv(a, w, grid, cin, cout, stride, role="conv"):
    M = a.shape[0]
    Mo = M * 8 if role == "convT" else M // stride ** 3
    out = torch.zeros((Mo, cout))
    R.c3_conv(a.float(), 0, cin, R.c3_prep(w.float(), role, torch.float32), None, out, 0, cout, grid, stride, role == "convT")
    return out


ORDER_CASES = [  # (grid, cin, cout, stride): small grids, and one level-0 sample of the real net
    ((1, 6, 10, 14), 40, 33, 1), ((3, 5, 7, 9), 12, 65, 1), ((2, 6, 10, 12), 8, 100, 2), ((1, 2, 4, 4), 512, 130, 1),
    ((1, 32, 64, 64), 32, 32, 1),
]


@pytest.mark.parametrize("grid,cin,cout,stride", ORDER_CASES, ids=[str(c) for c in ORDER_CASES])
def test_integer_fixtures_are_order_independent(grid, cin, cout, stride):
    M = grid[0] * grid[1] * grid[2] * grid[3]
    a, w = X.ints((M, cin), -2, 2, 1), X.ints((cout, cin, 3, 3, 3), -2, 2, 2)
    X.assert_exact_precondition(27 * cin, 2, 2, 0, "conv")
    y64 = X.conv_ref("conv", a, w, grid, stride)
    y32 = _fp32_conv(a, w, grid, cin, cout, stride)
    perm = torch.randperm(cin, generator=torch.Generator().manual_seed(3))
    y32p = _fp32_conv(a[:, perm].contiguous(), w[:, perm].contiguous(), grid, cin, cout, stride)
    assert torch.equal(y32.double(), y64) and torch.equal(y32p.double(), y64)
    assert X.mismatch_report(y32, X.expect(y64, torch.float32), (grid[0], grid[1] // stride, grid[2] // stride, grid[3] // stride))[0] == 0
    # weight gradient: P on the output grid, Q the input
    ogrid = (grid[0], grid[1] // stride, grid[2] // stride, grid[3] // stride)
    dy = X.ints((y64.shape[0], cout), -2, 2, 4)
    X.assert_exact_precondition(dy.shape[0], 2, 2, 0, "wgrad")
    dW64 = X.wgrad_ref(dy, a, ogrid, stride)
    dW32 = torch.zeros((cout, cin, 3, 3, 3))
    R.c3_wgrad(dy.float(), 0, cout, a.float(), 0, cin, dW32, ogrid, stride)
    assert torch.equal(dW32.double(), dW64)
    rp = torch.randperm(dy.shape[0], generator=torch.Generator().manual_seed(5))[: dy.shape[0] // 2]
    half = dy.clone()
    half[rp] = 0  # the same sum in two parts: another order
    dW32b = torch.zeros((cout, cin, 3, 3, 3))
    R.c3_wgrad(half.float(), 0, cout, a.float(), 0, cin, dW32b, ogrid, stride)
    R.c3_wgrad((dy - half).float(), 0, cout, a.float(), 0, cin, dW32b, ogrid, stride)
    assert torch.equal(dW32b.double(), dW64)


def test_transposed_statements_agree():
    grid, cin, cout = (2, 3, 5, 6), 40, 33
    a, w = X.ints((180, cin), -2, 2, 1), X.ints((cin, cout, 3, 3, 3), -2, 2, 2)
    y64 = X.conv_ref("convT", a, w, grid, 2)
    assert torch.equal(_fp32_conv(a, w, grid, cin, cout, 2, "convT").double(), y64)
    # the transposed convolution is the adjoint of the stride-2 convolution with the same weight: <convT(a), d> = <a, conv(d)>
    d = X.ints((y64.shape[0], cout), -2, 2, 3)
    back = X.conv_ref("convT_dgrad", d, w, (2, 6, 10, 12))
    assert float((y64 * d).sum()) == float((a * back).sum())


def test_precondition_rejects_operands_beyond_the_budget():
    X.assert_exact_precondition(27 * 512, 2, 2, 16, "widest forward")          # 55 312
    X.assert_exact_precondition(3 * 8 * 32 * 64 * 64, 2, 2, 8, "largest weight gradient")  # 12 582 920 of 16 777 216
    with pytest.raises(AssertionError):
        a, w = X.ints((64, 512), -64, 64, 1), X.ints((8, 512, 3, 3, 3), -64, 64, 2)
        X.assert_exact_precondition(27 * 512, float(a.abs().max()), float(w.abs().max()), 0, "values in -64 .. 64 at Cin 512")
    with pytest.raises(AssertionError):
        X.assert_exact_precondition(4194304, 2, 2, 0, "4 194 304 voxels")
    with pytest.raises(AssertionError):  # a statement that is no fp32 number cannot be an fp32 expectation
        X.expect(torch.tensor([2.0 ** 24 + 1], dtype=torch.float64), torch.float32)


def test_comparison_helper_sees_the_errors_the_old_tolerance_missed():
    """a zeroed tap, the last 8 input channels dropped and a weight gradient without its last 32 voxels: each would pass
    max|err| / max|ref| <= 2.5e-2; each is reported by the helper of the GPU tests"""
    grid, cin, cout = (3, 5, 7, 9), 40, 33
    M = 945
    a, w = X.ints((M, cin), -2, 2, 1), X.ints((cout, cin, 3, 3, 3), -2, 2, 2)
    y = X.conv_ref("conv", a, w, grid)
    for dt in (torch.float32, torch.bfloat16):
        ref = X.expect(y, dt)
        assert X.mismatch_report(ref.clone(), ref, grid)[0] == 0
        w_tap = w.clone()
        w_tap[:, :, 0, 1, 2] = 0
        n, msg = X.mismatch_report(X.conv_ref("conv", a, w_tap, grid).to(dt), ref, grid, what="tap (0, 1, 2) zeroed")
        assert n > 0 and "(b " in msg
        a_cut = a.clone()
        a_cut[:, cin - 8:] = 0
        n, _ = X.mismatch_report(X.conv_ref("conv", a_cut, w, grid).to(dt), ref, grid, what="last 8 channels dropped")
        assert n > 0
        with pytest.raises(AssertionError):
            X.assert_bit_equal(X.conv_ref("conv", a_cut, w, grid).to(dt), y, "last 8 channels dropped", grid)
    dy = X.ints((M, cout), -2, 2, 3)
    dW = X.wgrad_ref(dy, a, grid, 1)
    dy_short = dy.clone()
    dy_short[M - 32:] = 0
    n, _ = X.mismatch_report(X.wgrad_ref(dy_short, a, grid, 1).float().reshape(cout, -1), dW.float().reshape(cout, -1), what="last 32 voxels")
    assert n > 0
    # transposed: an error in one parity class is attributed to it
    yT = X.conv_ref("convT", X.ints((180, 8), -2, 2, 4), X.ints((8, 5, 3, 3, 3), -2, 2, 5), (2, 3, 5, 6), 2)
    bad = yT.clone()
    rows = X.grid_to_rows(X.rows_to_grid(torch.arange(yT.shape[0], dtype=torch.float64)[:, None], (2, 6, 10, 12))[:, :, 1::2, 0::2, 1::2])
    bad[rows.long().reshape(-1), 2] += 1
    n, msg = X.mismatch_report(bad, yT, (2, 6, 10, 12), parity=True)
    assert n == rows.numel() and "{5: %d}" % n in msg


# ------------------------------------------------------------------------------------------------ the GPU module's tables on the CPU
def test_layer_table_is_the_real_net():
    cases = X.layer_cases()
    assert len(cases) == 19 and len({c["name"] for c in cases}) == 19
    by = {c["name"]: c for c in cases}
    assert by["inconv_1_32"]["grid"] == (24, 32, 64, 64) and by["outconv_32_1"]["out_f32"]
    assert by["L0_block_32_32"]["grid"] == (3, 32, 64, 64) and by["L3_block_256_256"]["grid"] == (24, 4, 8, 8)
    assert by["bottleneck_512_512"]["grid"] == (24, 2, 4, 4)
    d = by["L1_down_64_128"]
    assert d["a_layouts"] == [(64, 128)] and (d["dx_ld"], d["dx_coff"], d["dx_acc"]) == (128, 64, True)
    u = by["L2_up_256_128"]
    assert u["grid"] == (3, 4, 8, 8) and (u["ldc"], u["ccoff"], u["dy_ld"]) == (256, 0, 256)
    assert len(X.edge_cases()) == 4 * 6 * 5 + 3


@pytest.mark.parametrize("case", X.layer_cases(patch=(16, 16, 16), b_wide=1, b_deep=1, b_thin=1), ids=lambda c: c["name"])
def test_layer_table_through_the_fp32_statements(case):
    X.run_conv_case(R, case, torch.float32, CPU)


@pytest.mark.parametrize("case", X.edge_cases(), ids=lambda c: c["name"])
def test_edge_table_through_the_fp32_statements(case):
    X.run_conv_case(R, case, torch.float32, CPU)


@pytest.mark.parametrize("M,C", [(min(M, 4096), C) for M, C in X.BN_CASES], ids=str)
def test_batchnorm_table_through_the_fp32_statements(M, C):
    X.run_bn_case(R, M, C, torch.float32, CPU)


@pytest.mark.parametrize("C", [1, 2, 33])
def test_layout_table_through_the_fp32_statements(C):
    X.run_layout_case(R, C, torch.float32, CPU)
