"""CPU: viscy_amd.data.feed.PatchCutter, the one procedure both DynaCLR feeds cut their batches with, run with a real
``FrameCache(device="cpu")`` and a launch written in numpy: the mixed resident / packed path, the split by storage dtype and the
host shortcut.  Plus the launch geometry of the two gather entries against the formulas they replaced, and
``transform_channel_wise`` against the triplet module's former version."""

import os
import subprocess

import numpy as np
import pytest
import torch

from viscy_amd.data.feed import FrameCache, PatchCutter, transform_channel_wise
from viscy_amd.data.multi_experiment import host_gather
from viscy_amd.data.triplet import host_cut

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAME, YP, XP = (2, 3, 8, 10), 4, 6
A, B, C = ("fov", 0), ("fov", 1), ("fov", 2)
# the cache takes A and B; C, the third distinct frame, does not fit.  One request three times, C through two distinct requests.
BATCH = [(A, 1, 2), (B, 4, 4), (C, 0, 0), (A, 0, 3), (C, 0, 0), (C, 3, 1), (C, 0, 0)]


def make_frames(dtypes, seed=0):
    rng = np.random.default_rng(seed)
    frames = {}
    for key, dtype in zip((A, B, C), dtypes):
        dtype = np.dtype(dtype)
        if dtype == np.float32:
            f = rng.standard_normal(FRAME).astype(np.float32)
            # (y, x) = (2, 4) and (3, 4) lie in both patches of A and in C's (0, 0); (5, 5) and (6, 6) in B's patch and in C's (3, 1)
            f[0, 0, 2, 4], f[1, 2, 6, 6] = -0.0, -0.0
            f.view(np.uint32)[0, 0, 3, 4] = 0x7FC12345   # NaNs with payloads
            f.view(np.uint32)[1, 1, 5, 5] = 0xFFC00001
        else:
            info = np.iinfo(dtype)
            f = rng.integers(info.min, info.max, size=FRAME, dtype=dtype, endpoint=True)
        frames[key] = f
    return frames


def bits(a):
    """the bytes of an array, so that NaN payloads and signed zeros count"""
    return np.ascontiguousarray(a).view(np.uint8)


class Harness:
    """a cutter over ``frames`` with every call counted; ``style``: requests described by origins (the triplet feed) or by index
    tables (the multi-experiment feed)"""

    def __init__(self, frames, style, budget=None, cached=True):
        self.frames, self.style = frames, style
        self.loads, self.gathers, self.begins, self.launches = [], [], [], []
        self.cache = None
        if cached:
            self.cache = FrameCache(self.load, lambda key: frames[key].nbytes, "cpu", budget)
            begin = self.cache.begin_batch

            def begin_batch(keys):
                self.begins.append(begin(keys))
                return self.begins[-1]

            self.cache.begin_batch = begin_batch
        self.cutter = PatchCutter("cpu", self.cache, self.load)

    def load(self, key):
        self.loads.append(key)
        return self.frames[key]

    def tables(self, y0, x0):
        return (np.arange(FRAME[0]), np.arange(FRAME[1]), y0 + np.arange(YP), x0 + np.arange(XP))

    def describe(self, r):
        return (r[1], r[2]) if self.style == "origin" else self.tables(r[1], r[2])

    def plain(self):
        return (0, 0) if self.style == "origin" else self.tables(0, 0)

    def host_patch(self, frame, r):
        self.gathers.append(r)
        return host_cut(frame, r[1], r[2], YP, XP) if self.style == "origin" else host_gather(frame, *self.tables(r[1], r[2]))

    def launch(self, sources, descriptors):
        """what ops.patch_gather / ops.patch_gather_scaled compute, in numpy"""
        self.launches.append((sources, descriptors))
        assert len({s.dtype for s in sources}) == 1, "one launch reads one storage dtype"
        rows = []
        for s, d in zip(sources, descriptors):
            a = s.numpy()
            rows.append(a[:, :, d[0] : d[0] + YP, d[1] : d[1] + XP] if self.style == "origin" else a[np.ix_(*d)])
        return torch.from_numpy(np.stack(rows).astype(np.float32))

    def cut(self, batch, kinds=None):
        return self.cutter.cut(batch, [r[0] for r in batch], [self.describe(r) for r in batch], self.host_patch, self.plain, self.launch,
                               kinds=kinds)

    def want(self, batch):
        return np.stack([self.frames[k][:, :, y0 : y0 + YP, x0 : x0 + XP] for k, y0, x0 in batch]).astype(np.float32)


def same_descriptor(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want)) and len(got) == len(want)


@pytest.mark.parametrize("style", ["origin", "tables"])
@pytest.mark.parametrize("dtype", [np.float32, np.uint16, np.int16, np.uint8])
def test_mixed_resident_and_packed_batch(style, dtype):
    frames = make_frames([dtype] * 3)
    h = Harness(frames, style, budget=2 * frames[A].nbytes)
    got = h.cut(BATCH)
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(BATCH), FRAME[0], FRAME[1], YP, XP)
    assert np.array_equal(bits(got.numpy()), bits(h.want(BATCH)))          # request order, bit for bit
    if dtype == np.float32:
        assert np.isnan(h.want(BATCH)).any() and (h.want(BATCH).view(np.uint32) == 0x80000000).any()   # the payloads and -0.0 are in the patches
    assert sorted(h.loads) == [A, B, C]                                     # A, B staged by the cache; C read once for two requests
    assert h.gathers == [(C, 0, 0), (C, 3, 1)]                              # each distinct host request once
    assert len(h.begins) == 1 and len(h.launches) == 1                      # one begin_batch, one launch
    resident = h.begins[0]
    assert resident[C] is None and A in h.cache and B in h.cache and C not in h.cache
    sources, descriptors = h.launches[0]
    packed_rows = {}
    for r, s, d in zip(BATCH, sources, descriptors):
        if r[0] == C:                                                       # a packed row: the patch itself, described whole
            assert same_descriptor(d, h.plain()) and tuple(s.shape) == (FRAME[0], FRAME[1], YP, XP) and s.dtype == torch.from_numpy(frames[C]).dtype
            assert np.array_equal(bits(s.numpy()), bits(frames[C][:, :, r[1] : r[1] + YP, r[2] : r[2] + XP]))
            packed_rows.setdefault(r, s.data_ptr())
            assert packed_rows[r] == s.data_ptr()                           # equal requests name the same packed row
        else:                                                               # the cache's own tensor, the request's own descriptor
            assert s is resident[r[0]] and same_descriptor(d, h.describe(r))
    assert len(set(packed_rows.values())) == 2
    h.cut(BATCH[:2])                                                        # a resident batch: nothing read, nothing packed
    assert len(h.begins) == 2 and sorted(h.loads) == [A, B, C] and len(h.gathers) == 2
    assert all(s is resident[r[0]] for r, s in zip(BATCH[:2], h.launches[1][0]))


@pytest.mark.parametrize("style", ["origin", "tables"])
def test_a_batch_of_two_storage_dtypes_takes_one_launch_per_dtype(style):
    frames = make_frames([np.uint16, np.uint8, np.uint16])
    h = Harness(frames, style, budget=frames[A].nbytes + frames[B].nbytes)   # C, uint16, is gathered on the host
    got = h.cut(BATCH, kinds=[frames[r[0]].dtype for r in BATCH])
    assert np.array_equal(bits(got.numpy()), bits(h.want(BATCH)))
    assert len(h.begins) == 1 and h.begins[0][C] is None                     # the cache is asked once for the whole batch
    assert [{s.dtype for s in sources} for sources, _ in h.launches] == [{torch.uint16}, {torch.uint8}]
    assert [len(sources) for sources, _ in h.launches] == [6, 1]
    assert h.loads.count(C) == 1 and h.gathers == [(C, 0, 0), (C, 3, 1)]


@pytest.mark.parametrize("style", ["origin", "tables"])
@pytest.mark.parametrize("dtype", [np.float32, np.uint16])
def test_without_a_cache_every_patch_is_taken_on_the_host(style, dtype):
    frames = make_frames([dtype] * 3)
    h = Harness(frames, style, cached=False)
    got = h.cut(BATCH)
    assert got.dtype == torch.float32 and np.array_equal(bits(got.numpy()), bits(h.want(BATCH)))
    assert h.launches == [] and sorted(h.loads) == [A, B, C] and len(h.gathers) == len(set(BATCH))


def _parent_triplet_transform_channel_wise(transform, channel_names, patch, norm_meta):
    """``viscy_amd.data.triplet._transform_channel_wise`` as it stood before the feeds shared one"""
    def collate(norm_metas):
        out = {}
        for ch, levels in norm_metas[0].items():
            out[ch] = {}
            for level, stats in levels.items():
                out[ch][level] = None if stats is None else {st: torch.stack([m[ch][level][st] for m in norm_metas]) for st in stats}
        return out

    channels = {name: patch[:, c : c + 1].contiguous() for c, name in zip(range(patch.shape[1]), channel_names)}
    if norm_meta is not None:
        channels["norm_meta"] = collate(norm_meta)
    channels = transform(channels)
    channels.pop("norm_meta", None)
    return torch.cat(list(channels.values()), dim=1)


def test_transform_channel_wise_without_extras_is_the_triplet_version(tmp_path):
    from tests.test_triplet_feed_cpu import golden, make_dataset, write_plate
    from viscy_amd.data.hcs import Compose
    from viscy_amd.transforms import NormalizeSampled

    g = golden()
    case = g["cases"]["t1_neg"]
    ds = make_dataset(write_plate(tmp_path), fit=True, **case["kwargs"])
    np.random.seed(case["seed"])
    sample = ds.__getitems__(case["indices"])
    names = g["source_channel"]
    transform = Compose([NormalizeSampled(names, "fov_statistics")])
    for key in ("anchor", "positive", "negative"):
        patch, norm = sample[key], sample[f"{key}_norm_meta"]
        assert all(t.device == patch.device for m in norm for t in m[names[0]]["fov_statistics"].values())   # already where the patch is
        want = _parent_triplet_transform_channel_wise(transform, names, patch.clone(), norm)
        got = transform_channel_wise(transform, names, patch.clone(), norm)
        assert not torch.equal(want, patch) and torch.equal(got, want)
    assert torch.equal(transform_channel_wise(Compose([]), names, sample["anchor"], None), sample["anchor"])


# ------------------------------------------------------------------------------------------------ launch geometry
_GEOMETRY_MAIN = r"""
#include <stdio.h>
#include "patch_gather.hip"
static int g_cus;
int vsx_cu_count() { return g_cus; }
void vsx_set_error(const char*, ...) {}
int main() {
  const long rows_of[] = {1, 7, 4096, 100000, 3000000};
  const int xs[] = {2, 64, 65, 128, 129, 16384}, cus[] = {256, 8};
  for (int cu : cus)
    for (long rows : rows_of)
      for (int xp : xs)
        for (int code = VSX_PG_F32; code <= VSX_PG_U8; ++code) {
          g_cus = cu;
          // vsx_patch_gather: rows = n C Z Yp output rows
          const int lpr = pg_lanes_per_row(vsx_cdiv(xp, vsx_src_vec_elems(code)));
          const unsigned grid = vsx_capped_grid(rows, 256 / lpr, 8);
          // vsx_patch_gather_scaled: rows = n C Zt planes of Yt = 37 rows each
          const int lprs = pg_lanes_per_row(vsx_cdiv(xp, 4));
          const int rb = (256 / lprs) * VSX_PGS_ROWS_PER_GROUP;
          const unsigned grids = vsx_capped_grid(rows * vsx_cdiv(37, rb), 1, 8);
          printf("%d %ld %d %d %d %u %d %d %u\n", cu, rows, xp, code, lpr, grid, lprs, rb, grids);
        }
  return 0;
}
"""


def test_gather_launch_geometry_is_what_the_entries_computed_before(tmp_path):
    """the helpers the two gather entries now share (pg_lanes_per_row, vsx_src_vec_elems, vsx_capped_grid), compiled for the host,
    against the arithmetic that stood in ``vsx_patch_gather`` and ``vsx_patch_gather_scaled`` before, restated here"""
    from viscy_amd import _lib

    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    (tmp_path / "geometry.hip").write_text(_GEOMETRY_MAIN)
    exe = str(tmp_path / "geometry")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O0", "-I", os.path.join(ROOT, "viscy_amd", "csrc"), "-o", exe,
                    str(tmp_path / "geometry.hip")], check=True, capture_output=True)
    lines = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")

    def old_lpr(vecs):
        return 16 if vecs <= 16 else (32 if vecs <= 32 else 64)

    want = []
    for cu in (256, 8):
        for rows in (1, 7, 4096, 100000, 3000000):
            for xp in (2, 64, 65, 128, 129, 16384):
                for code in (_lib.PG_F32, _lib.PG_U16, _lib.PG_I16, _lib.PG_U8):
                    ve = 4 if code == _lib.PG_F32 else (16 if code == _lib.PG_U8 else 8)
                    lpr = old_lpr(-(-xp // ve))
                    grid = min(-(-rows // (256 // lpr)), cu * 8)
                    lprs = old_lpr(-(-xp // 4))
                    rb = (256 // lprs) * _lib.PGS_ROWS_PER_GROUP
                    grids = min(rows * -(-37 // rb), cu * 8)
                    want.append(f"{cu} {rows} {xp} {code} {lpr} {grid} {lprs} {rb} {grids}")
    assert lines == want + [""]
    assert {int(w.split()[4]) for w in want} == {16, 32, 64} and {int(w.split()[7]) for w in want} == {64, 32, 16}
