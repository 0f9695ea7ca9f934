"""GPU: the radix select, the percentile rescale and the crop + Z-reduction kernels (csrc/boc_transforms.hip) against the CPU:
torch.sort's picks, torch.quantile, and the host paths of the same classes (which tests/test_boc_transforms_cpu.py pins to the
reference's outputs).  Everything is compared with torch.equal except the interpolated percentile bounds, whose bound is the
three roundings of a lerp."""

import itertools
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
SELECT_CASES = [(1, 1), (3, 2), (2, 5), (4, 255), (2, 1027), (3, 4099), (2, 65539), (1, 1000003)]
PAIRS = [(1, 99), (50, 99), (0, 100), (0.1, 99.9)]
KINDS = ["randn", "halves", "mixed", "equal_row", "nan_row"]
_cache: dict = {}


def _data(rows: int, n: int, kind: str) -> torch.Tensor:
    g = torch.Generator().manual_seed(1000 * rows + n)
    x = torch.randn((rows, n), generator=g) * 7.0
    if kind == "halves":                       # heavy ties
        x = (x * 2.0).round() / 2.0
    elif kind == "mixed":                      # both signs, denormals, +0 and -0
        x = x * 1e-3
        sel = torch.rand((rows, n), generator=g)
        x = torch.where(sel < 0.2, x * 1e-38, x)           # denormal magnitudes
        x = torch.where((sel >= 0.2) & (sel < 0.3), torch.zeros(()), x)
        x = torch.where((sel >= 0.3) & (sel < 0.4), -torch.zeros(()), x)
    elif kind == "equal_row":
        x[0] = -2.75
    elif kind == "nan_row":
        x[rows - 1, n // 2] = float("nan")
    return x.contiguous()


def _sorted(rows: int, n: int, kind: str):
    """(input, its rows sorted on the CPU, rows that hold a NaN): computed once, shared, never written to"""
    key = (rows, n, kind)
    if key not in _cache:
        x = _data(rows, n, kind)
        _cache[key] = (x, torch.sort(x, dim=1).values, x.isnan().any(dim=1))
    return _cache[key]


def _ranks(pair, n: int):
    from viscy_amd.transforms import quantile_ranks

    (l0, h0, w0), (l1, h1, w1) = quantile_ranks(pair[0] / 100.0, n), quantile_ranks(pair[1] / 100.0, n)
    return (l0, h0, l1, h1), (w0, w1)


def _same(a: torch.Tensor, b: torch.Tensor) -> bool:
    """equal by value, NaN in the same places (-0.0 == +0.0)"""
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(nan=0.0), b.nan_to_num(nan=0.0))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rows,n", SELECT_CASES)
def test_row_select_picks_what_sort_picks(rows, n, kind):
    from viscy_amd.transforms import row_select

    x, srt, has_nan = _sorted(rows, n, kind)
    xd = x.to(DEV)
    for pair in PAIRS:
        ranks, _ = _ranks(pair, n)
        want = srt[:, list(ranks)].clone()
        want[has_nan] = float("nan")           # a row that holds a NaN yields NaN for all its ranks, as torch.quantile does
        got = row_select(xd, ranks)
        again = row_select(xd, ranks)
        assert got.shape == (rows, 4)
        assert _same(got.cpu(), want), (rows, n, kind, pair, ranks)
        assert torch.equal(got.view(torch.int32), again.view(torch.int32))   # bit-identical from run to run


def test_row_select_above_the_quantile_limit():
    """one row of 2^24 + 1 values: torch.quantile refuses it, the select does not; checked against torch.sort on the CPU"""
    from viscy_amd.transforms import row_select

    n = (1 << 24) + 1
    x = torch.randn((1, n), generator=torch.Generator().manual_seed(24)) * 7.0
    with pytest.raises(RuntimeError):
        torch.quantile(x, 0.5, dim=1)
    ranks, _ = _ranks((1, 99), n)
    ranks = ranks[:2] + (n - 1, 0)
    srt = torch.sort(x, dim=1).values
    got = row_select(x.to(DEV), ranks)
    assert torch.equal(got.cpu(), srt[:, list(ranks)])


def test_row_select_refuses_bad_arguments():
    from viscy_amd.transforms import row_select

    x = torch.zeros((2, 10), device=DEV)
    for ranks in ((10,), (-1,), (0, 1, 2, 3, 4), ()):
        with pytest.raises(RuntimeError, match="row_select"):
            row_select(x, ranks)
    with pytest.raises(RuntimeError, match="no CPU"):
        row_select(x[:, ::2], (0,))


@pytest.mark.parametrize("kind", ["randn", "halves"])
@pytest.mark.parametrize("rows,n", SELECT_CASES)
def test_percentile_bounds_against_quantile(rows, n, kind):
    """exact where the rank is integral; elsewhere within 4 * 2^-23 * max(|s_lo|, |s_hi|): a lerp is three rounded operations
    (a difference, a product, a sum), each within 2^-24 relative of a magnitude no larger than twice that maximum, and a device
    compiler may contract them differently from the CPU's"""
    from viscy_amd.transforms import percentile_bounds

    x, srt, _ = _sorted(rows, n, kind)
    xd = x.to(DEV)
    for pair in PAIRS:
        ranks, (w0, w1) = _ranks(pair, n)
        want = torch.quantile(x, torch.tensor([pair[0] / 100.0, pair[1] / 100.0], dtype=torch.float32), dim=1)
        a_min, a_max = percentile_bounds(xd, pair[0] / 100.0, pair[1] / 100.0)
        for got, ref, w, (lo, hi) in ((a_min.cpu(), want[0], w0, ranks[:2]), (a_max.cpu(), want[1], w1, ranks[2:])):
            if w == 0.0:
                assert torch.equal(got, ref), (rows, n, kind, pair)
            else:
                bound = 4.0 * 2.0 ** -23 * torch.maximum(srt[:, lo].abs(), srt[:, hi].abs())
                assert ((got - ref).abs() <= bound).all(), (rows, n, kind, pair, (got - ref).abs().max().item(), bound.min().item())


def _scale_host(x2d, a_min, a_max, deg, b_min, b_max, clip):
    """the reference's lines on (rows, n) with per-row bounds; ``deg`` (rows,) picks the degenerate formula"""
    lo, hi = a_min.view(-1, 1), a_max.view(-1, 1)
    shifted = x2d - lo if b_min is None else x2d - lo + b_min
    y = (x2d - lo) / (hi - lo)
    if (b_min is not None) and (b_max is not None):
        y = y * (b_max - b_min) + b_min
    if clip:
        y = y.clip(b_min, b_max)
    return torch.where(deg.view(-1, 1), shifted, y)


def test_percentile_scale_kernel_is_the_host_formula():
    from viscy_amd.transforms import BatchedScaleIntensityRangePercentiles, percentile_scale

    g = torch.Generator().manual_seed(7)
    for rows, n, offset in ((3, 1027, 0), (2, 4096, 0), (5, 1, 0), (3, 1027, 1), (4, 255, 3)):
        buf = torch.randn(rows * n + offset, generator=g) * 7.0 + 3.0
        x = buf[offset:].view(rows, n)
        x[0, n // 2] = float("nan")
        x[rows - 1, 0] = float("inf")
        a_min = torch.randn(rows, generator=g) * 2.0 - 8.0
        a_max = a_min + torch.rand(rows, generator=g) * 20.0 + 1.0
        xd = buf.to(DEV)[offset:].view(rows, n)                 # offset != 0: the rows start off the 16-byte grid
        assert xd.is_contiguous() and xd.data_ptr() % 16 == (4 * offset) % 16
        degs = [torch.zeros(rows, dtype=torch.bool), torch.ones(rows, dtype=torch.bool), torch.arange(rows) % 2 == 0]
        for (b_min, b_max), clip, relative, deg in itertools.product(((0.0, 1.0), (-1.5, 2.25), (None, None), (0.5, None)),
                                                                     (False, True), (False, True), degs):
            if relative and (b_min is None or b_max is None):
                continue
            if clip and b_min is None and b_max is None:
                continue
            _, _, bl, bh = BatchedScaleIntensityRangePercentiles(2, 98, b_min, b_max, clip, relative)._targets()
            want = _scale_host(x, a_min, a_max, deg, bl, bh, clip)
            got = percentile_scale(xd, a_min.to(DEV), a_max.to(DEV), deg.to(DEV), bl, bh, clip)
            assert _same(got.cpu(), want), (rows, n, offset, b_min, b_max, clip, relative, deg.tolist())


@pytest.mark.parametrize("channel_wise", [False, True])
def test_percentile_transform_equals_the_host_path(channel_wise):
    """(2, C, 1, 73, 137): 10001 values per row, so the 1 % and 99 % ranks are 100 and 9900 exactly (w == 0, asserted) and the
    device bounds equal torch.quantile's: the whole output is bit-equal to the host path"""
    from viscy_amd.transforms import BatchedScaleIntensityRangePercentilesd, quantile_ranks

    C = 2 if channel_wise else 1
    assert quantile_ranks(0.01, 10001)[2] == 0.0 and quantile_ranks(0.99, 10001)[2] == 0.0
    if not channel_wise:
        assert quantile_ranks(0.01, C * 10001)[2] == 0.0
    g = torch.Generator().manual_seed(73)
    x = torch.randn((2, C, 1, 73, 137), generator=g) * 7.0 + 3.0
    x_const = x.clone()
    x_const[1, C - 1] = 2.5
    for kw in (dict(b_min=0.0, b_max=1.0, clip=True), dict(b_min=0.0, b_max=1.0, clip=False), dict(b_min=None, b_max=None),
               dict(b_min=-1.0, b_max=3.0, clip=True, relative=True)):
        t = BatchedScaleIntensityRangePercentilesd(["a"], lower=1, upper=99, channel_wise=channel_wise, **kw)
        for inp in (x, x_const):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                want = t({"a": inp.clone()})["a"]
            got = t({"a": inp.to(DEV)})["a"]
            assert got.is_cuda and got.shape == inp.shape
            assert torch.equal(got.cpu(), want), (channel_wise, kw, inp is x_const)


# ------------------------------------------------------------------------------------------------ crop + Z-reduction
def _host_crop_zreduce(x, starts, size, labelfree):
    from viscy_amd.transforms import BatchedChannelWiseZReduction, BatchedRandSpatialCrop

    return BatchedChannelWiseZReduction()(BatchedRandSpatialCrop(list(size))(x, params=starts), is_labelfree=labelfree)


def test_z_reduction_full_size_and_edges():
    from viscy_amd.transforms import BatchedChannelWiseZReduction, BatchedChannelWiseZReductiond

    g = torch.Generator().manual_seed(9)
    x = torch.randn((3, 2, 5, 7, 9), generator=g)
    x[1, 0, 3, 2, 4] = float("nan")            # one NaN voxel: the maximum keeps it, the centre plane (z = 2) does not see it
    mask = torch.tensor([True, False, True])
    for strategy, m in (("mip", None), ("center", None), ("mip", mask), ("mip", ~mask)):
        t = BatchedChannelWiseZReduction(strategy)
        want = t(x.clone(), is_labelfree=m)
        got = t(x.to(DEV), is_labelfree=None if m is None else m.to(DEV))
        assert got.shape == (3, 2, 1, 7, 9) and _same(got.cpu(), want), (strategy, m)
    assert BatchedChannelWiseZReduction("mip")(x.to(DEV)).isnan().sum() == 1
    for Z in (1, 2):
        xz = x[:, :, :Z].contiguous()
        for strategy in ("mip", "center"):
            assert torch.equal(BatchedChannelWiseZReduction(strategy)(xz.to(DEV)).cpu(), BatchedChannelWiseZReduction(strategy)(xz.clone()))
    xd = x[:, :, :1].contiguous().to(DEV)
    assert BatchedChannelWiseZReduction()(xd) is xd
    d = BatchedChannelWiseZReductiond(["a", "b"], labelfree_keys=["b"])({"a": x.to(DEV), "b": x.to(DEV), "_is_labelfree": mask})
    assert "_is_labelfree" not in d
    assert _same(d["a"].cpu(), x.amax(dim=2, keepdim=True)) and torch.equal(d["b"].cpu(), x[:, :, 2:3])


def test_crop_and_fused_crop_z_reduction():
    from viscy_amd import transforms as T

    g = torch.Generator().manual_seed(10)
    x = torch.randn((2, 3, 6, 37, 70), generator=g)
    x[0, 1, 4, 20, 33] = float("nan")
    size = (4, 32, 63)
    xd = x.to(DEV)
    top = [6 - 4, 37 - 32, 70 - 63]
    for starts, held in (([[0, 0, 0], [0, 0, 0]], None), ([top, top], None), ([[1, 2, 3], top], None),
                         ([[9, 50, 99], [-3, -1, -7]], [top, [0, 0, 0]])):      # outside the volume: clamped, a defined result
        st = torch.tensor(starts)
        inside = torch.tensor(held) if held is not None else st
        want_crop = T.BatchedRandSpatialCrop(list(size))(x.clone(), params=inside)
        assert torch.equal(T.BatchedRandSpatialCrop(list(size))(xd, params=st).cpu().nan_to_num(nan=5.0), want_crop.nan_to_num(nan=5.0))
        for labelfree in (None, torch.tensor([True, False]), torch.tensor([False, True])):
            want = _host_crop_zreduce(x.clone(), inside, size, labelfree)
            mode = T._z_modes(2, labelfree, False)
            got = T.crop_zreduce(xd, st, size, mode)
            assert got.shape == (2, 3, 1, 32, 63) and _same(got.cpu(), want), (starts, labelfree)
            # the fused object of the recipes' pair against the pair itself, same starts
            crop, zred = T.BatchedRandSpatialCropd(["a"], list(size)), T.BatchedChannelWiseZReductiond(["a"], allow_missing_keys=True)
            (fused,) = T.fuse_crop_zreduce([crop, zred])
            batch = {"a": xd} if labelfree is None else {"a": xd, "_is_labelfree": labelfree}
            pair = zred(crop(dict(batch), params=st))["a"]
            one = fused(dict(batch), params=st)["a"]
            assert _same(one.cpu(), want) and torch.equal(one.view(torch.int32), pair.view(torch.int32))
    # drawn, not injected: the fused call and the pair consume the same stream
    crop, zred = T.BatchedRandSpatialCropd(["a"], list(size)), T.BatchedChannelWiseZReductiond(["a"])
    (fused,) = T.fuse_crop_zreduce([crop, zred])
    crop.cropper.generator = torch.Generator().manual_seed(4)
    a = fused({"a": xd})["a"]
    crop.cropper.generator = torch.Generator().manual_seed(4)
    b = zred(crop({"a": xd}))["a"]
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # a Z window of one plane: the pair passes the crop through, the fused kernel returns the same plane
    crop1 = T.BatchedRandSpatialCropd(["a"], [1, 32, 63])
    (fused1,) = T.fuse_crop_zreduce([crop1, T.BatchedChannelWiseZReductiond(["a"])])
    st = torch.tensor([[3, 1, 2], [5, 5, 7]])
    assert torch.equal(fused1({"a": xd}, params=st)["a"].cpu(), T.BatchedRandSpatialCrop([1, 32, 63])(x.clone(), params=st))
