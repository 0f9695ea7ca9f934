"""GPU: the conv3d / bn3d kernels (csrc/conv3d.hip) against float64 on operands for which fp32 arithmetic is exact
(tests/ref_exact_fnet3d.py): small integers, sum |a| |w| < 2^24 asserted per case from the operands.  An fp32 result must equal
the float64 statement bit for bit, a bf16 result the statement rounded once to bf16.  One lost, doubled or misplaced term changes
an integer by at least 1 and fails, at any problem size.

a. every distinct convolution launch of Unet3d(1, 1, depth=4, mult_chan=32) on 32 x 64 x 64 with the engine's operand layout, at
   B = 3 (32- to 128-channel levels; 393 216 voxels at level 0) and B = 24 (256- / 512-channel levels, inconv, outconv;
   3 145 728 voxels): forward with bias and statistics, data gradient, weight gradient (up to 256 splits), bias gradient;
b. edges: non-power-of-two grids with row tails, cin x cout tails, the vector and the element-wise gather on the same values,
   accumulate, output slices between sentinels, single voxels;
c. the epilogue's BatchNorm partials (sum exact; sum of squares within the bound of a sum of 64 non-negative terms);
d. BatchNorm apply / backward / finalize on dyadic tables;  e. the layout kernels.

Every assert is torch.equal / integer equality, except the two derived bounds (sum of squares, training-mode dz) and the
one-rounding checks of bn3d_finalize, each derived next to its assert in tests/ref_exact_fnet3d.py."""

import pytest
import torch

from tests import ref_exact_fnet3d as X

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
# the case is the outer parameter: its two dtypes run back to back and share the float64 statements


@pytest.fixture(scope="module", autouse=True)
def _release_fixtures():
    yield
    X.clear_fixtures()
    torch.cuda.empty_cache()


@DTYPES
@pytest.mark.parametrize("case", X.layer_cases(), ids=lambda c: c["name"])
def test_real_layer_table_is_bit_exact(case, dt):
    from viscy_amd import ops

    X.run_conv_case(ops, case, dt, torch.device("cuda"))
    torch.cuda.empty_cache()


@DTYPES
@pytest.mark.parametrize("case", X.edge_cases(), ids=lambda c: c["name"])
def test_edges_are_bit_exact(case, dt):
    from viscy_amd import ops

    X.run_conv_case(ops, case, dt, torch.device("cuda"))


@DTYPES
@pytest.mark.parametrize("M,C", X.BN_CASES, ids=str)
def test_batchnorm_apply_and_backward_on_dyadic_tables(M, C, dt):
    from viscy_amd import ops

    X.run_bn_case(ops, M, C, dt, torch.device("cuda"))
    torch.cuda.empty_cache()


@pytest.mark.parametrize("C,G", [(1, 1), (33, 7), (100, 300), (512, 2048)])
def test_batchnorm_finalize_on_integer_partials(C, G):
    from viscy_amd import ops

    X.run_bn_finalize_case(ops, C, G, torch.device("cuda"))


@DTYPES
@pytest.mark.parametrize("C", [1, 2, 33])
def test_layout_kernels_are_bit_exact(C, dt):
    from viscy_amd import ops

    X.run_layout_case(ops, C, dt, torch.device("cuda"))
