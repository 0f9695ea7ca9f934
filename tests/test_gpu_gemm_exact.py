"""GPU: the NT / TN GEMM families (csrc/gemm.hip, csrc/gemm_nt2.hip) and the depthwise 7x7 kernels (csrc/dwconv.hip,
csrc/dwconv_mfma.hip) against float64 on operands for which fp32 arithmetic is exact (tests/ref_exact_gemm.py): an fp32 result
must equal the float64 statement bit for bit, a bf16 result the statement rounded once to bf16, the columns around every slice
must keep their sentinel, and every per-sample reduction must land on its own sample.  One product dropped from a K loop, one
pixel row lost or doubled at a split boundary, one row credited to the neighbouring sample or one tap wrong at one image border
fails here at any size; the tolerance tests of tests/test_gpu_ops.py cannot see them (tests/test_gemm_exact_cpu.py shows both).

After every GEMM launch the dispatched kernel family (vsx_last_kernel) is compared with the one the case table names: a case
whose dispatch has moved fails.  Every assert is torch.equal."""

import pytest
import torch

from tests import ref_exact_gemm as X

pytestmark = pytest.mark.gpu

# the case is the outer parameter: its dtypes run back to back and share the float64 statements


def _env():
    from viscy_amd import _lib, ops

    return ops, X.Flags(_lib.lib()), torch.device("cuda")


def _by_dtype(cases):
    return [pytest.param(c, dt, id=f"{c['name']}-{X.dtname(dt)}") for c in cases for dt in c["dts"]]


@pytest.fixture(scope="module", autouse=True)
def _release_fixtures():
    yield
    X.clear_fixtures()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("case,dt", _by_dtype(X.nt_cases()))
def test_gemm_nt_is_bit_exact(case, dt):
    ops, flags, dev = _env()
    X.run_nt_case(ops, case, dt, dev, flags)


@pytest.mark.parametrize("case,dt", _by_dtype(X.tn_cases()))
def test_gemm_tn_is_bit_exact(case, dt):
    ops, flags, dev = _env()
    X.run_tn_case(ops, case, dt, dev, flags)


@pytest.mark.parametrize("dt", X.BOTH, ids=X.dtname)
def test_conv3x3_patch_matrices_are_bit_exact(dt):
    ops, _, dev = _env()
    X.run_im2col_case(ops, dt, dev)


@pytest.mark.parametrize("dt", X.BOTH, ids=X.dtname)
@pytest.mark.parametrize("shape", X.DW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dwconv7_is_bit_exact_under_every_flag(shape, dt):
    ops, flags, dev = _env()
    X.run_dw_case(ops, shape, dt, dev, flags)
