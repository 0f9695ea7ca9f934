"""GPU: the ten entry points of the narrow-channel (VSCyto2D) kernels (csrc/narrow.hip) through the C-ABI against float64 on operands
for which fp32 arithmetic is exact (tests/ref_exact_narrow.py), at the launch edges the tolerance tests of tests/test_gpu_vscyto2d.py
do not reach: several tiles per workgroup (tpw = 2, a clipped last workgroup), the grid-stride loops of the stem, the projection
and the shuffle adjoint, the stem weight gradient at K = 20, Cin = 3, 128 rows per workgroup and its admission limits, every
projection width from 1 to the full 192, maps smaller than the 7 x 7 window, one pixel, exactly one tile.

torch.equal: stem forward / weight gradient, the shuffle adjoint, the depthwise output and pass C, the projection's dxn / db and
(gamma = 0) out / dW / mean, the block passes with fc1 dead and GELU saturated.  A derived bound K u A (ref_exact_narrow.K_BLOCK,
K_PROJ): the GRN sums, pass 2's output, dW2, P, dy, dW1f, db1f, the projection's rstd / out / dW with live gamma.  Every output lies
between sentinel guards and starts as NaN (stored) or from small integers (accumulated); the partials' scratch has exactly the size
the restated grid needs and is found fully written.  tests/test_narrow_exact_cpu.py runs the same tables on the CPU and shows which
seeded indexing errors the tolerance tests see.  The worst observed ratios are in profiles/narrow_exact_margins.txt."""

import pytest
import torch

from tests import ref_exact_narrow as X

pytestmark = pytest.mark.gpu

CS = (4, 8)
DTN = tuple(X.DTYPES)


def _env():
    from viscy_amd import _lib

    return X.LibEntry(_lib.lib()), torch.device("cuda")


@pytest.fixture(scope="module", autouse=True)
def _release_fixtures():
    yield
    X.clear_fixtures()
    torch.cuda.empty_cache()


def _sid(shape):
    return "x".join(map(str, shape))


@pytest.mark.parametrize("dtn", DTN)
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("shape", X.BLOCK_SHAPES, ids=_sid)
def test_block_passes_are_bit_exact(shape, C, dtn):
    ep, dev = _env()
    X.run_block_exact(ep, shape, C, dtn, dev)


@pytest.mark.parametrize("dtn", DTN)
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("shape", X.BOUNDED_SHAPES, ids=_sid)
def test_block_passes_are_within_their_derived_bounds(shape, C, dtn):
    ep, dev = _env()
    X.run_block_bounded(ep, shape, C, dtn, dev)


_STEM = [pytest.param(c, d, id=f"{c['name']}-{d}") for c in X.stem_cases() for d in c["dts"]]


@pytest.mark.parametrize("case,dtn", _STEM)
def test_stem_forward_and_weight_gradient_are_bit_exact(case, dtn):
    ep, dev = _env()
    X.run_stem_case(ep, case, dtn, dev)


@pytest.mark.parametrize("dtn", DTN)
@pytest.mark.parametrize("ref", X.stem_refusals(), ids=lambda r: r[0])
def test_stem_refuses_one_past_each_limit(ref, dtn):
    ep, dev = _env()
    X.run_stem_refusal(ep, ref, dtn, dev)


@pytest.mark.parametrize("dtn", DTN)
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("Ccat", X.PROJ_CCAT)
def test_projection_is_bit_exact_with_gamma_zero(Ccat, C, dtn):
    ep, dev = _env()
    for M in X.PROJ_M:
        X.run_proj_case(ep, M, Ccat, C, dtn, dev)


def test_projection_forward_past_the_grid_cap():
    """M = 1 048 577 rows: 65537 steps of 16 rows on a grid capped at 65536 workgroups"""
    ep, dev = _env()
    assert X.cdiv(X.PROJ_BIG["M"], 16) == 65537
    X.run_proj_case(ep, X.PROJ_BIG["M"], X.PROJ_BIG["Ccat"], X.PROJ_BIG["C"], "fp32", dev, bwd=False)


@pytest.mark.parametrize("dtn", DTN)
@pytest.mark.parametrize("C", CS)
def test_projection_refuses_ccat_193(C, dtn):
    ep, dev = _env()
    X.run_proj_refusal(ep, C, dtn, dev)


@pytest.mark.parametrize("dtn", DTN)
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("M,Ccat", X.PROJ_BOUNDED)
def test_projection_is_within_its_derived_bounds(M, Ccat, C, dtn):
    ep, dev = _env()
    X.run_proj_bounded(ep, M, Ccat, C, dtn, dev)


@pytest.mark.parametrize("cfg", X.SHUFFLE_CFG, ids=lambda c: f"{c[0]}_{c[1]}_{c[2]}_{'pool' if c[3] else 'nopool'}")
def test_shuffle_adjoint_is_bit_exact(cfg):
    ep, dev = _env()
    for geo in X.SHUFFLE_GEO:
        for dtn in DTN:
            X.run_shuffle_case(ep, cfg, geo, dtn, dev)


def test_shuffle_adjoint_past_the_grid_cap():
    ep, dev = _env()
    (Cout, D, s, _), (B, h, w) = X.SHUFFLE_BIG
    assert B * h * w * Cout * D * s * s > 65536 * X.NB
    X.run_shuffle_case(ep, *X.SHUFFLE_BIG, "fp32", dev)
