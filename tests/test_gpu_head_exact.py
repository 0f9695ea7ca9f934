"""GPU: the PixelToVoxelHead kernels against float64 on operands for which fp32 arithmetic is exact (tests/ref_exact_head.py): the
direct 3x3x3 convolution of csrc/headconv.hip (forward under both kernels, each with atomics and with fixed-order sums; weight
gradient with unprep_grad; data gradient with its weight pre-pack), the head's pixel shuffle + pad-pool in its strip, tiled and
thread-per-element tiers (csrc/spatial.hip) and the FCMAE voxel shuffle with its narrow backward.  A bf16 result must equal the
statement rounded once to bf16, an fp32 result the statement itself; U and the InstanceNorm sums must be the same bits under
all four forward settings.  One tap's plane offset, a halo column zeroed at one tile or strip border, a tile's statistics
credited to the neighbouring sample, a tile skipped by a persistent loop or the row above a row range missing from the carried
pool sums moves a result by at least 1 (1/4 for the pooled shuffles) and fails here; tests/test_head_exact_cpu.py shows which of
them the tolerance tests of tests/test_gpu_ops.py see.

The stride loop of vsx_voxel_shuffle_bwd is not reached (see ref_exact_head.voxel_cases).  Every assert is torch.equal."""

import pytest
import torch

from tests import ref_exact_head as X

pytestmark = pytest.mark.gpu

# the case is the outer parameter: its parts, directions and flag settings run back to back and share the float64 statements


def _env():
    from viscy_amd import _lib, ops

    return ops, X.Flags(_lib.lib()), torch.device("cuda")


@pytest.fixture(scope="module", autouse=True)
def _release_fixtures():
    yield
    X.clear_fixtures()
    torch.cuda.empty_cache()


def _with(cases, inner):
    return [pytest.param(c, i, id=f"{c['name']}-{i}") for c in cases for i in inner(c)]


@pytest.mark.parametrize("case,part", _with(X.conv_cases(), lambda c: X.CONV_PARTS))
def test_head_conv_is_bit_exact(case, part):
    ops, flags, dev = _env()
    X.run_conv_case(ops, case, part, dev, flags)


@pytest.mark.parametrize("case,direction", _with(X.shuffle_cases(), lambda c: ("fwd", "bwd")))
def test_head_shuffle_is_bit_exact_in_every_tier(case, direction):
    ops, flags, dev = _env()
    X.run_shuffle_case(ops, case, direction, dev, flags)


@pytest.mark.parametrize("case,direction", _with(X.voxel_cases(), lambda c: c["dirs"]))
def test_voxel_shuffle_is_bit_exact(case, direction):
    ops, _, dev = _env()
    X.run_voxel_case(ops, case, direction, dev)
