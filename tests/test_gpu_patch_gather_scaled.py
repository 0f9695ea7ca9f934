"""GPU: vsx_patch_gather_scaled behind viscy_amd.ops.patch_gather_scaled — every case bit-equal to the numpy box cut followed by
CPU ``F.interpolate(patch[None].float(), size=target, mode="nearest-exact")``, compared through an int32 view (NaN payloads and
signed zeros count), with the frames sitting between poisoned guard rows and the output in front of a guard region that must
come back untouched.

Shapes: frames [3, 7, 37, 41] of float32 (random BIT patterns), uint16, int16 and uint8; targets (5, 16, 24) and (1, 1, 13)
(odd Xt, one row, one plane); native boxes per target: the identity, an upscale from (3, 11, 17) and a downscale from the whole
frame (7, 37, 41), so that the first and the last plane, row and column are read; one box at every frame corner; channel lists
C = 1 (another channel per patch), C = 2 as [2, 0], C = 3 in order; n = 1, n = 7 with repeated descriptors over two frames (one
a strided view into a larger block), and an n whose work units leave one pass of the bounded grid."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD_BITS = 0x7FC0DEAD
FRAME = (3, 7, 37, 41)
TARGETS = [(5, 16, 24), (1, 1, 13)]
DTYPES = {"float32": np.float32, "uint16": np.uint16, "int16": np.int16, "uint8": np.uint8}
POISON = {"float32": np.uint32(GUARD_BITS).view(np.float32), "uint16": 0xDEAD, "int16": -0x2153, "uint8": 0xAD}
SPECIAL_F32 = np.array([0x7FC12345, 0xFFC00001, 0x7F800001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF],
                       dtype=np.uint32).view(np.float32)


def make_frame(rng, dtype, shape=FRAME, guard_rows=2):
    """-> (device frame, numpy frame): the frame is the middle of a block whose first and last ``guard_rows`` planes-worth of rows
    hold a poison value; a load outside the frame brings poison (or the neighbouring plane) into the output"""
    np_dtype = np.dtype(DTYPES[dtype])
    C, Z, H, W = shape
    block = np.full((C * Z * H + 2 * guard_rows, W), POISON[dtype], dtype=np_dtype)
    if dtype == "float32":
        a = rng.integers(0, 2 ** 32, size=shape, dtype=np.uint32).view(np.float32)
        a.reshape(-1)[: SPECIAL_F32.size] = SPECIAL_F32
        a.reshape(-1)[-SPECIAL_F32.size:] = SPECIAL_F32[::-1]
    else:
        info = np.iinfo(np_dtype)
        a = rng.integers(info.min, info.max + 1, size=shape, dtype=np_dtype)
        a.reshape(-1)[:2] = (info.min, info.max)
        a.reshape(-1)[-2:] = (info.max, info.min)
    block[guard_rows:-guard_rows] = a.reshape(-1, W)
    dev = torch.from_numpy(block).to(DEV)[guard_rows:-guard_rows].view(shape)
    return dev, a


def tables_for(origin, native, target, shared=None):
    """absolute (z, y, x) tables of a native box at ``origin`` resampled to ``target``; the identity keeps the positions.
    ``shared``: a dict through which equal tables of one axis become ONE array object (one table in the launch)"""
    from viscy_amd.data import nearest_exact_index

    identity = tuple(native) == tuple(target)
    out = []
    for axis, (o, n, t) in enumerate(zip(origin, native, target)):
        key = (axis, o, n, t, identity)
        table = None if shared is None else shared.get(key)
        if table is None:
            table = o + (np.arange(n, dtype=np.int64) if identity else nearest_exact_index(n, t))
            if shared is not None:
                shared[key] = table
        out.append(table)
    return tuple(out)


def expected(array, channels, origin, native, target):
    """the reference's procedure: numpy box cut, then CPU nearest-exact interpolation of the float32 patch"""
    (z0, y0, x0), (nz, ny, nx) = origin, native
    patch = array[list(channels), z0 : z0 + nz, y0 : y0 + ny, x0 : x0 + nx].astype(np.float32)
    if tuple(native) == tuple(target):
        return patch
    return F.interpolate(torch.from_numpy(patch)[None], size=tuple(target), mode="nearest-exact")[0].numpy()


def corners(native, frame=FRAME):
    """the box flush with each of the four row / column corners, the first and the last planes alternating"""
    dz, dy, dx = (f - n for f, n in zip(frame[1:], native))
    return list(dict.fromkeys([(0, 0, 0), (dz, 0, dx), (0, dy, 0), (dz, dy, dx)]))


def boxes_for(target):
    """(origin, native) pairs: identity, upscale and whole-frame downscale, each at every corner"""
    out = []
    for native in (target, (3, 11, 17), FRAME[1:]):
        native = tuple(min(n, f) for n, f in zip(native, FRAME[1:]))
        out += [(o, native) for o in corners(native)]
    return out


def channel_lists(C, n):
    if C == 1:
        return [(p % 3,) for p in range(n)]
    return [(2, 0)] * n if C == 2 else [(0, 1, 2)] * n


def launch_and_check(sources, arrays, channels, origins, natives, target, share=False):
    from viscy_amd import ops

    n, C = len(sources), len(channels[0])
    shared = {} if share else None
    tabs = [tables_for(o, nat, target, shared) for o, nat in zip(origins, natives)]
    shape = (n, C, *target)
    total, guard = int(np.prod(shape)), 64
    pad = (-total) % 4  # the guard behind an output whose size is no multiple of four floats starts right at its end
    buf = torch.full((guard + total + pad + guard,), GUARD_BITS, dtype=torch.int32, device=DEV).view(torch.float32)
    out = ops.patch_gather_scaled(sources, [np.asarray(c) for c in channels], [t[0] for t in tabs], [t[1] for t in tabs],
                                  [t[2] for t in tabs], out=buf[guard : guard + total].view(shape))
    want = np.stack([expected(a, c, o, nat, target) for a, c, o, nat in zip(arrays, channels, origins, natives)])
    got = buf.view(torch.int32).cpu()
    assert bool((got[:guard] == GUARD_BITS).all()) and bool((got[guard + total:] == GUARD_BITS).all()), "guard region was written"
    assert torch.equal(got[guard : guard + total].view(shape), torch.from_numpy(want).view(torch.int32)), (target, origins, natives)
    return out


@pytest.mark.parametrize("C", [1, 2, 3])
@pytest.mark.parametrize("target", TARGETS)
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_bit_equal_to_box_cut_and_nearest_exact(dtype, target, C):
    """every box kind at every corner in one launch; then each box alone (n = 1)"""
    rng = np.random.default_rng(100 * list(DTYPES).index(dtype) + 10 * TARGETS.index(target) + C)
    dev, a = make_frame(rng, dtype)
    boxes = boxes_for(target)
    n = len(boxes)
    ch = channel_lists(C, n)
    launch_and_check([dev] * n, [a] * n, ch, [b[0] for b in boxes], [b[1] for b in boxes], target)
    for kind in (0, n // 2, n - 1):  # identity, upscale, whole frame
        launch_and_check([dev], [a], ch[kind : kind + 1], [boxes[kind][0]], [boxes[kind][1]], target)


@pytest.mark.parametrize("dtype", ["float32", "uint16"])
def test_seven_patches_repeats_two_frames_one_strided(dtype):
    rng = np.random.default_rng(7)
    dev, a = make_frame(rng, dtype)
    np_dtype = DTYPES[dtype]
    block = (rng.integers(0, 2 ** 32, size=(2, 3, 9, 40, 48), dtype=np.uint32).view(np.float32) if dtype == "float32"
             else rng.integers(0, 65536, size=(2, 3, 9, 40, 48), dtype=np_dtype))
    block_d = torch.from_numpy(block).to(DEV)
    view, view_d = block[1, :, 1:8, 2:39, 5:46], block_d[1, :, 1:8, 2:39, 5:46]   # (3, 7, 37, 41) inside the block
    assert tuple(view_d.shape) == FRAME and not view_d.is_contiguous() and view_d.stride() == (9 * 40 * 48, 40 * 48, 48, 1)
    for target in TARGETS:
        b = boxes_for(target)
        picks = [b[0], b[5], b[0], b[-1], b[5], b[0], b[-1]]
        sources = [dev, view_d, dev, view_d, view_d, dev, dev]
        arrays = [a, view, a, view, view, a, a]
        for C in (1, 2, 3):
            ch = channel_lists(C, 7)
            ch[5] = ch[2] = ch[0]  # patches 0, 2 and 5: the same descriptor three times
            out = launch_and_check(sources, arrays, ch, [p[0] for p in picks], [p[1] for p in picks], target)
            o = out.contiguous().view(torch.int32)
            assert torch.equal(o[0], o[2]) and torch.equal(o[0], o[5])


@pytest.mark.parametrize("target", TARGETS)
def test_work_units_past_one_pass_of_the_bounded_grid(target):
    """the grid is capped at eight workgroups per compute unit; a work unit is (patch, channel, plane, block of rows), the block
    being 256 / lanes-per-row row groups times PGS_ROWS_PER_GROUP rows.  Both targets take 16 lanes per row (at most 16
    16-byte vectors per row), so a block holds 64 rows and every (patch, channel, plane) is one unit."""
    from viscy_amd import _lib

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cap = cus * 8
    Zt, Yt, Xt = target
    lanes = 16
    assert (Xt + 3) // 4 <= 16
    rows_per_unit = (256 // lanes) * _lib.PGS_ROWS_PER_GROUP
    C = 1
    n = int(1.3 * cap / (C * Zt * -(-Yt // rows_per_unit))) + 1
    assert n * C * Zt * -(-Yt // rows_per_unit) > 1.3 * cap
    rng = np.random.default_rng(11)
    frames = [make_frame(rng, d) for d in ("uint16", "uint16")]
    boxes = boxes_for(target)
    pick = rng.integers(0, len(boxes), size=n)
    which = rng.integers(0, 2, size=n)
    launch_and_check([frames[w][0] for w in which], [frames[w][1] for w in which], channel_lists(C, n),
                     [boxes[i][0] for i in pick], [boxes[i][1] for i in pick], target)
    # the same with ONE x table object for every patch (boxes of one native size whose x origin is 0, other planes, rows, frames
    # and channels): a workgroup that comes round again finds the table it holds in LDS and skips the reload
    same_x = [b for b in boxes if b[0][2] == 0 and b[1] == boxes[0][1]]
    assert len(same_x) >= 2 and len({b[0][:2] for b in same_x}) >= 2
    pick = rng.integers(0, len(same_x), size=n)
    shared = {}
    assert len({id(tables_for(b[0], b[1], target, shared)[2]) for b in same_x}) == 1
    launch_and_check([frames[w][0] for w in which], [frames[w][1] for w in which], channel_lists(C, n),
                     [same_x[i][0] for i in pick], [same_x[i][1] for i in pick], target, share=True)


def test_x_table_as_long_as_the_lds_holds():
    """Xt = PGS_MAX_XT: 64 KiB of dynamic LDS, 64 lanes per row; one entry more is refused on the host"""
    from viscy_amd import _lib, ops
    from viscy_amd.data import nearest_exact_index

    Xt, W = _lib.PGS_MAX_XT, 5000
    rng = np.random.default_rng(13)
    a = rng.integers(0, 65536, size=(1, 2, 3, W), dtype=np.uint16)
    dev = torch.from_numpy(a).to(DEV)
    xs = 7 + nearest_exact_index(W - 7, Xt)   # an upscale that reads the last column
    assert xs[0] == 7 and xs[-1] == W - 1
    got = ops.patch_gather_scaled([dev, dev], [np.arange(1)] * 2, [np.array([1, 0])] * 2, [np.array([2, 0, 1]), np.array([1, 1, 2])], [xs, xs])
    for p, ys in enumerate(([2, 0, 1], [1, 1, 2])):
        want = a[:, [1, 0]][:, :, ys][:, :, :, xs].astype(np.float32)
        assert torch.equal(got[p].cpu().view(torch.int32), torch.from_numpy(want).view(torch.int32))
    with pytest.raises(ValueError, match="x tables of at most"):
        ops.patch_gather_scaled([dev], [np.arange(1)], [np.arange(2)], [np.arange(3)], [np.zeros(Xt + 1, dtype=np.int64)])


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_arange_tables_equal_patch_gather(dtype):
    """identity tables over all channels in order: the bits of ``vsx_patch_gather`` on the same boxes"""
    from viscy_amd import ops

    rng = np.random.default_rng(5)
    dev, a = make_frame(rng, dtype)
    C, Z, H, W = FRAME
    for yp, xp in ((16, 24), (2, 6), (36, 40)):
        origins = [(0, 0), (H - yp, W - xp), (min(1, H - yp), min(3, W - xp)), (H - yp, 0), (0, W - xp)]
        n = len(origins)
        chans, zs = [np.arange(C)] * n, [np.arange(Z)] * n
        got = ops.patch_gather_scaled([dev] * n, chans, zs, [y0 + np.arange(yp) for y0, _ in origins],
                                      [x0 + np.arange(xp) for _, x0 in origins])
        want = ops.patch_gather([dev] * n, origins, (yp, xp))
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_table_entries_outside_the_frame_raise_before_any_launch():
    from viscy_amd import ops

    f = torch.zeros(FRAME, device=DEV)
    good = [np.arange(2), np.arange(3), np.arange(4), np.arange(5)]
    out = torch.full((1, 2, 3, 4, 5), 7.0, device=DEV)
    for axis, name in enumerate(("channel", "z", "y", "x")):
        for bad_value in (FRAME[axis], -1):  # one past the axis, one in front of it
            tabs = [t.copy() for t in good]
            tabs[axis][-1] = bad_value
            with pytest.raises(ValueError, match=f"patch 0 {name} table"):
                ops.patch_gather_scaled([f], *[[t] for t in tabs], out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "something was launched"
    with pytest.raises(ValueError, match="patch 1 x table has 4 entries"):
        ops.patch_gather_scaled([f, f], [good[0]] * 2, [good[1]] * 2, [good[2]] * 2, [good[3], np.arange(4)])
    with pytest.raises(NotImplementedError, match="float64"):
        ops.patch_gather_scaled([f.double()], *[[t] for t in good])
    with pytest.raises(TypeError, match="patch_gather_scaled: out"):
        ops.patch_gather_scaled([f], *[[t] for t in good], out=torch.empty(1, 2, 3, 4, 6, device=DEV))
