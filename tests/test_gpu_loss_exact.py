"""GPU: the seven entry points of the MixedLoss kernels (csrc/loss.hip) against float64 on operands for which fp32 arithmetic is
exact (tests/ref_exact_loss.py): vsx_loss_pool, vsx_loss_tmax, vsx_ssim_scale_fwd, _fwd_dmu and _fwd_fused on the same stacks
against the same statement, a two-scale chain by hand, vsx_ssim_scale_bwd_in from hand-made fields and per-sample factors, and
vsx_loss_finalize.

torch.equal: the pooled stacks, the data ranges (max over the 64 slots), the L1 / L2 sums (float64 sum over the slots), every
slot vsx_loss_tmax writes (and -inf in the others), the sums of the P == T forward (old value + C (H - 10) (W - 10): every output
pixel of every tile counted once), the isolating backward cases.  A derived bound K u A (ref_exact_loss.RE, K_PIXEL): the two
maps' per-sample sums, the three gradient fields, the combined backward case, the finalisation.  Every output buffer starts as
NaN.  A footprint column counted twice, a last tile's rows not pooled, the factor of another sample or slot, a slot left out of
a range, a pooled gradient read at the odd leftover fail here; tests/test_loss_exact_cpu.py shows which of them the tolerance
tests of tests/test_gpu_model.py see.  The worst observed ratios are in profiles/loss_exact_margins.txt."""

import pytest
import torch

from tests import ref_exact_loss as X

pytestmark = pytest.mark.gpu

# the case is the outer parameter: its entry points, flags and directions run back to back and share the float64 statements


def _env():
    from viscy_amd import _lib

    return X.LibEntry(_lib.lib()), torch.device("cuda")


@pytest.fixture(scope="module", autouse=True)
def _release_fixtures():
    yield
    X.clear_fixtures()
    torch.cuda.empty_cache()


def _ids(cases):
    return [c["name"] for c in cases]


def _with(cases, inner):
    return [pytest.param(c, i, id=f"{c['name']}-{i}") for c in cases for i in inner(c)]


@pytest.mark.parametrize("case,direction", _with(X.stack_cases(), lambda c: ("fwd", "bwd") if c["bwd"] else ("fwd",)))
def test_ssim_scale_entry_points_match_the_statement(case, direction):
    """the unaligned views differ from their aligned case in the one-pass forward's load path only: no backward"""
    ep, dev = _env()
    (X.run_forward_case if direction == "fwd" else X.run_backward_case)(ep, case, dev)


@pytest.mark.parametrize("case", X.chain_cases(), ids=_ids(X.chain_cases()))
def test_two_scale_chain_reads_what_the_first_launch_wrote(case):
    ep, dev = _env()
    X.run_chain_case(ep, case, dev)


@pytest.mark.parametrize("case", X.pool_cases(), ids=_ids(X.pool_cases()))
def test_loss_pool_is_bit_exact(case):
    ep, dev = _env()
    X.run_pool_case(ep, case, dev)


@pytest.mark.parametrize("n", X.TMAX_N)
def test_loss_tmax_slots_are_bit_exact(n):
    ep, dev = _env()
    X.run_tmax_case(ep, n, dev)


@pytest.mark.parametrize("case", X.finalize_cases(), ids=_ids(X.finalize_cases()))
def test_loss_finalize_is_within_its_derived_bound(case):
    ep, dev = _env()
    X.run_finalize_case(ep, case, dev)


def test_whole_loss_through_the_entry_points_matches_the_module():
    """the restatement of MixedLossFn that the CPU file drives the seeded defects through (ref_exact_loss.mixed_loss_via) is what
    viscy_amd.losses.MixedLoss does: same loss and gradient on the library's kernels, one-pass and two-pass"""
    from viscy_amd import _lib
    from viscy_amd.losses import MixedLoss

    ep, dev = _env()
    gen = torch.Generator().manual_seed(5)
    target = torch.rand((1, 2, 3, 181, 176), generator=gen)
    pred = target + 0.1 * torch.randn(target.shape, generator=gen)
    flags = X.Flags(_lib.lib())
    for fused in (1, 0):
        with flags.scoped({"loss_fused": fused}):
            assert flags.get("loss_fused") == fused
            p = pred.cuda().requires_grad_(True)
            loss = MixedLoss(0.5, 0.25, 0.5)(p, target.cuda())
            loss.backward()
        l, g = X.mixed_loss_via(ep, pred, target, 0.5, 0.25, 0.5, bool(fused), dev)
        # the same kernels on the same inputs: only the atomics' order differs, which moves a per-sample factor by a few ulp and
        # may flip the bf16 rounding of single products under the 121 D-term window sums
        assert abs(l.item() - loss.item()) <= 2e-6 * abs(loss.item()), (fused, l.item(), loss.item())
        d = (g - p.grad.cpu()).abs().max().item() / p.grad.abs().max().item()
        assert d <= 1e-3, (fused, d)
    assert flags.get("loss_fused") == 1
