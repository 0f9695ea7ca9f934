"""GPU: vsx_patch_gather behind viscy_amd.ops.patch_gather — every case bit-equal to the numpy slice
``frame[:, :, y0:y0 + Yp, x0:x0 + Xp].astype(np.float32)``, compared through an int32 view, with the output sitting between
guard rows that must come back untouched.

Shapes: frame widths 37 and 40 (for a patch wider than that: Xp + 37 and Xp + 40, the same two residues of W mod 8 with room for
every x0), x0 over every residue mod 8 plus the patch flush with the frame's last row and column, Xp in {2, 6, 8, 10, 64, 66,
160}, Yp in {2, 5}, C and Z in {1, 3}.  float32 frames are filled with random BIT patterns (NaNs with payloads, infinities,
denormals among them) and carry the named special values at fixed places; integer frames carry both ends of their range."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
XPS = [2, 6, 8, 10, 64, 66, 160]
GUARD_BITS = 0x7FC0DEAD
SPECIAL_F32 = np.array([0x7FC12345, 0xFFC00001, 0x7F800001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF],
                       dtype=np.uint32).view(np.float32)   # quiet / negative / signalling NaN payloads, +-inf, -0.0, denormals
DTYPES = {"float32": np.float32, "uint16": np.uint16, "int16": np.int16, "uint8": np.uint8}


def make_frame(rng, dtype, shape):
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        a = rng.integers(0, 2 ** 32, size=shape, dtype=np.uint32).view(np.float32)
        flat = a.reshape(-1)
        flat[: SPECIAL_F32.size] = SPECIAL_F32
        flat[-SPECIAL_F32.size:] = SPECIAL_F32[::-1]
        return a
    info = np.iinfo(dtype)
    a = rng.integers(info.min, info.max + 1, size=shape, dtype=dtype)
    a.reshape(-1)[:2] = (info.min, info.max)
    a.reshape(-1)[-2:] = (info.max, info.min)
    return a


def bits(t):
    return t.contiguous().view(torch.int32)


def check(sources, arrays, origins, size):
    """sources[i]: device tensor (C, Z, H, W) (any view), arrays[i]: the same values as numpy.  Launches once into a guarded
    buffer and compares bits."""
    from viscy_amd import ops

    yp, xp = size
    n, (C, Z) = len(sources), arrays[0].shape[:2]
    shape = (n, C, Z, yp, xp)
    total, guard = int(np.prod(shape)), 4 * xp   # a multiple of four floats: the output stays 16-byte aligned
    buf = torch.full((guard + total + guard,), GUARD_BITS, dtype=torch.int32, device=DEV).view(torch.float32)
    out = ops.patch_gather(sources, origins, size, out=buf[guard : guard + total].view(shape))
    want = np.stack([a[:, :, y0 : y0 + yp, x0 : x0 + xp].astype(np.float32) for a, (y0, x0) in zip(arrays, origins)])
    assert out.dtype == torch.float32 and tuple(out.shape) == shape
    got = buf.view(torch.int32).cpu()
    assert bool((got[:guard] == GUARD_BITS).all()) and bool((got[guard + total:] == GUARD_BITS).all()), "guard rows were written"
    assert torch.equal(got[guard : guard + total].view(shape), torch.from_numpy(want).view(torch.int32)), (size, origins)
    return out


def origins_for(H, W, yp, xp):
    """x0 over every residue mod 8 that fits (y0 varying with it), and the patch flush with the last row and column"""
    o = [(r % (H - yp + 1), r) for r in range(min(8, W - xp + 1))]
    o.append((H - yp, W - xp))
    return o


@pytest.mark.parametrize("xp", XPS)
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_bit_equal_over_widths_residues_and_extents(dtype, xp):
    rng = np.random.default_rng(1000 * XPS.index(xp) + list(DTYPES).index(dtype))
    for base in (37, 40):
        W = base if xp <= 10 else xp + base
        for yp in (2, 5):
            for C in (1, 3):
                for Z in (1, 3):
                    H = yp + 4
                    a = make_frame(rng, DTYPES[dtype], (C, Z, H, W))
                    f = torch.from_numpy(a).to(DEV)
                    o = origins_for(H, W, yp, xp)
                    assert {x0 % 8 for _, x0 in o} >= set(range(8)) and (H - yp, W - xp) in o
                    check([f] * len(o), [a] * len(o), o, (yp, xp))


def test_special_float_values_survive():
    """the named values at known places of a 40-wide frame, read at every alignment of the source row"""
    a = np.zeros((1, 1, 3, 40), np.float32)
    a[0, 0, 1, 3 : 3 + SPECIAL_F32.size] = SPECIAL_F32
    a[0, 0, 2, -SPECIAL_F32.size:] = SPECIAL_F32
    f = torch.from_numpy(a).to(DEV)
    for xp in (10, 16):
        o = [(1, x0) for x0 in range(0, 9)] + [(1, 40 - xp)]
        out = check([f] * len(o), [a] * len(o), o, (2, xp))
        got = bits(out[3])[0, 0, 0, : SPECIAL_F32.size].cpu().numpy().view(np.uint32)   # x0 = 3: the row starts at the specials
        assert (got == SPECIAL_F32.view(np.uint32)).all()
        assert bits(out[3])[0, 0, 0, 5].item() == -(2 ** 31)   # -0.0 keeps its sign bit


@pytest.mark.parametrize("dtype", ["uint16", "int16", "uint8"])
def test_integer_range_ends_convert_exactly(dtype):
    info = np.iinfo(DTYPES[dtype])
    a = np.zeros((1, 1, 2, 37), DTYPES[dtype])
    a[0, 0, 0, ::2], a[0, 0, 1, 1::2] = info.max, info.min
    f = torch.from_numpy(a).to(DEV)
    o = [(0, x0) for x0 in range(0, 12)]
    out = check([f] * len(o), [a] * len(o), o, (2, 26))
    assert out.max().item() == float(info.max) and out.min().item() == float(min(info.min, 0))
    if dtype == "uint16":
        assert sorted(out.unique().tolist()) == [0.0, 65535.0]


@pytest.mark.parametrize("dtype", ["float32", "uint16"])
def test_strided_views_packed_blocks_and_repeats_in_one_launch(dtype):
    """frames that are views into a larger block (strides of the block), contiguous packed (C, Z, Yp, Xp) blocks with origin
    (0, 0), a frame of another height and width, and the same descriptor twice, mixed in ONE launch"""
    rng = np.random.default_rng(7)
    C, Z, yp, xp = 3, 3, 5, 10
    block = make_frame(rng, DTYPES[dtype], (2, C, Z + 2, 15, 45))
    block_d = torch.from_numpy(block).to(DEV)
    view, view_d = block[1, :, 1 : 1 + Z, 2:13, 3:40], block_d[1, :, 1 : 1 + Z, 2:13, 3:40]   # (3, 3, 11, 37)
    assert not view_d.is_contiguous() and view_d.stride() == (5 * 15 * 45, 15 * 45, 45, 1)
    packed = make_frame(rng, DTYPES[dtype], (4, C, Z, yp, xp))
    packed_d = torch.from_numpy(packed).to(DEV)
    other = make_frame(rng, DTYPES[dtype], (C, Z, 9, 40))
    other_d = torch.from_numpy(other).to(DEV)
    sources = [view_d, packed_d[0], view_d, other_d, packed_d[3], view_d, packed_d[0], other_d, view_d]
    arrays = [view, packed[0], view, other, packed[3], view, packed[0], other, view]
    origins = [(6, 27), (0, 0), (1, 5), (4, 30), (0, 0), (6, 27), (0, 0), (0, 1), (6, 27)]
    out = check(sources, arrays, origins, (yp, xp))
    assert torch.equal(bits(out[0]), bits(out[5])) and torch.equal(bits(out[0]), bits(out[8]))   # anchor and positive
    assert torch.equal(bits(out[1]), bits(out[6]))


def test_rows_past_one_pass_of_the_bounded_grid():
    """the grid is capped at eight workgroups per compute unit; a workgroup takes 256 / lanes-per-row rows per pass.  Both lane
    groupings loop here: 16 lanes per row (Xp = 2) with 49 500 rows, 64 lanes per row (Xp = 160, float32) with 11 250"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(11)
    for dtype, xp, n, lanes in (("uint16", 2, 1100, 16), ("float32", 160, 250, 64)):
        C, Z, yp = 3, 3, 5
        assert n * C * Z * yp > 1.3 * cus * 8 * (256 // lanes), "the case no longer leaves one pass: raise n"
        frames = [make_frame(rng, DTYPES[dtype], (C, Z, 8, xp + 37)) for _ in range(3)]
        dev = [torch.from_numpy(a).to(DEV) for a in frames]
        pick = rng.integers(0, 3, size=n)
        origins = [(int(rng.integers(0, 4)), int(rng.integers(0, 38))) for _ in range(n)]
        origins[-1] = (3, 37)
        check([dev[i] for i in pick], [frames[i] for i in pick], origins, (yp, xp))


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_single_patch(dtype):
    rng = np.random.default_rng(3)
    a = make_frame(rng, DTYPES[dtype], (1, 1, 2, 37))
    check([torch.from_numpy(a).to(DEV)], [a], [(0, 35)], (2, 2))
    a = make_frame(rng, DTYPES[dtype], (3, 3, 7, 40))
    check([torch.from_numpy(a).to(DEV)], [a], [(2, 7)], (5, 26))


def test_bad_descriptors_raise_before_any_launch():
    from viscy_amd import ops

    f = torch.zeros(1, 1, 8, 37, device=DEV)
    for origin in ((-1, 0), (5, 0), (0, -1), (0, 32)):
        with pytest.raises(ValueError, match="leave the frame"):
            ops.patch_gather([f], [origin], (4, 6))
    with pytest.raises(NotImplementedError, match="float64"):
        ops.patch_gather([f.double()], [(0, 0)], (4, 6))
    with pytest.raises(TypeError, match="patch_gather: out"):
        ops.patch_gather([f], [(0, 0)], (4, 6), out=torch.empty(1, 1, 1, 4, 8, device=DEV))
