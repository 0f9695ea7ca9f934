"""The device patch feed under ``triplet.py`` and ``multi_experiment.py``: time-point frames resident in device memory in their
storage dtype (``FrameCache``), and ONE procedure that cuts a batch of patches out of them (``PatchCutter``).

The cutter asks the cache once per batch.  A frame the budget cannot hold is read on the host (distinct frames on up to
``MAX_READ_THREADS`` threads), its patches are taken there, packed into one pinned buffer, uploaded in one copy and described to
the same launch as the resident frames, so the device has one code path and both sources give the same bits.  Without a cache
(no HIP device) every patch is taken on the host.  A dataset supplies what differs: the frame key of a request, its descriptor
in a resident frame and in a packed row, how to take it out of a host frame, and the launch.

Also here, once: the batch-side helpers both data modules share (``collate_norm_meta``, ``transform_channel_wise``, ``tree_to``,
``identity``).
"""

from __future__ import annotations

from collections import OrderedDict
from concurrent.futures import ThreadPoolExecutor
from typing import Callable, Hashable, Sequence

import numpy as np
import torch
from torch import Tensor

from ..ops import STORAGE_DTYPES  # numpy storage dtype -> torch dtype of what the gather kernels read

MAX_READ_THREADS = 16


def default_device(device=None) -> torch.device:
    """where a feed makes its batches: ``device``, else the current HIP device, else the CPU"""
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    return torch.device(device)


def check_storage_dtype(dtype, where: str) -> None:
    if np.dtype(dtype) not in STORAGE_DTYPES:
        raise NotImplementedError(f"{where}: images stored as {np.dtype(dtype)} are not built (float32, uint16, int16 and uint8 are)")


def read_frames(load: Callable[[Hashable], np.ndarray], keys: list) -> dict:
    """host reads of distinct frames, at most MAX_READ_THREADS at a time"""
    if len(keys) <= 1:
        return {k: load(k) for k in keys}
    with ThreadPoolExecutor(max_workers=min(len(keys), MAX_READ_THREADS)) as pool:
        return dict(zip(keys, pool.map(load, keys)))


class FrameCache:
    """Time-point frames resident on ``device``: key -> (C, Z, H, W) tensor in its storage dtype, at most ``budget_bytes`` in all.

    ``begin_batch(keys)`` answers, per distinct key, the resident tensor or ``None`` (cut that frame's patches on the host).  A
    missing frame is staged through pinned memory when it fits after evicting least recently used frames that the batch does
    NOT need; a frame the batch needs is never evicted, so what ``begin_batch`` hands out stays valid for the whole batch.
    ``load(key)`` reads a frame as a numpy array, ``nbytes(key)`` tells its size without reading it.  Pure host policy over
    torch tensors: ``device`` may be the CPU."""

    def __init__(self, load: Callable[[Hashable], np.ndarray], nbytes: Callable[[Hashable], int], device, budget_bytes: int):
        self._load, self._nbytes = load, nbytes
        self.device, self.budget_bytes = torch.device(device), max(int(budget_bytes), 0)
        self._frames: OrderedDict = OrderedDict()  # least recently used first
        self._sizes: dict = {}
        self.bytes_used = 0
        self.uploads = self.hits = self.evictions = self.refused = 0

    def keys(self) -> list:
        """resident keys, least recently used first"""
        return list(self._frames)

    def __contains__(self, key) -> bool:
        return key in self._frames

    def _stage(self, key) -> Tensor:
        host = torch.from_numpy(np.ascontiguousarray(self._load(key)))
        if self.device.type != "cuda":
            return host
        pinned = torch.empty(host.shape, dtype=host.dtype, pin_memory=True)
        pinned.copy_(host)
        return pinned.to(self.device, non_blocking=True)

    def begin_batch(self, keys: Sequence[Hashable]) -> dict:
        needed = list(dict.fromkeys(keys))
        pinned = set(needed)
        out = {}
        for key in needed:
            if key in self._frames:
                self._frames.move_to_end(key)
                self.hits += 1
                out[key] = self._frames[key]
                continue
            size = int(self._nbytes(key))
            evictable = sum(self._sizes[k] for k in self._frames if k not in pinned)
            if self.bytes_used - evictable + size > self.budget_bytes:
                self.refused += 1
                out[key] = None
                continue
            for victim in [k for k in self._frames if k not in pinned]:
                if self.bytes_used + size <= self.budget_bytes:
                    break
                del self._frames[victim]
                self.bytes_used -= self._sizes.pop(victim)
                self.evictions += 1
            frame = self._stage(key)
            self._frames[key], self._sizes[key] = frame, size
            self.bytes_used += size
            self.uploads += 1
            out[key] = frame
        return out


class PatchCutter:
    """Cuts batches for a dataset on ``device``: ``cache`` is its ``FrameCache`` (``None``: no HIP device, every patch is taken on
    the host), ``load_frame(key)`` reads a frame as a numpy array."""

    def __init__(self, device, cache: FrameCache | None, load_frame: Callable[[Hashable], np.ndarray]):
        self.device, self.cache, self.load_frame = torch.device(device), cache, load_frame

    def cut(self, requests: list, keys: list, descriptors: list, host_patch: Callable, plain: Callable, launch: Callable,
            kinds: list | None = None) -> Tensor:
        """float32 (n, C, Z, Y, X) on ``device``, row ``i`` the patch of ``requests[i]`` (hashable; equal requests are taken once):

        ``keys[i]``               the cache key of the frame request ``i`` reads
        ``descriptors[i]``        where it lies in that frame when resident, as ``launch`` wants it (an origin, index tables)
        ``host_patch(frame, r)``  the (C, Z, Y, X) patch of request ``r`` out of the numpy frame, in its storage dtype
        ``plain()``               the descriptor of a whole packed row
        ``launch(sources, descriptors)``  one gather over (C, Z, H, W) device tensors of one storage dtype
        ``kinds[i]``              the storage dtype of request ``i``'s frame where a batch may span stores of different dtypes: one
                                  launch per dtype, each writing its rows of the batch

        The cache is asked ONCE for the whole batch, so no launch of the batch loses a frame to another's."""
        resident = self.cache.begin_batch(keys) if self.cache is not None else dict.fromkeys(keys)
        pin = self.device.type == "cuda"

        def one_dtype(rows) -> Tensor:  # rows: positions in ``requests``
            host = {requests[i]: keys[i] for i in rows if resident[keys[i]] is None}  # distinct requests: taken and sent once
            slot = {r: j for j, r in enumerate(host)}
            packed = None
            if host:
                frames = read_frames(self.load_frame, list(dict.fromkeys(host.values())))
                for j, (r, key) in enumerate(host.items()):
                    patch = host_patch(frames[key], r)
                    if packed is None:
                        packed = torch.empty((len(host), *patch.shape), dtype=STORAGE_DTYPES[patch.dtype], pin_memory=pin)
                        view = packed.numpy()
                    view[j] = patch
            if self.cache is None:
                return torch.from_numpy(view[[slot[requests[i]] for i in rows]].astype(np.float32))
            whole = None
            if packed is not None:
                packed = packed.to(self.device, non_blocking=True)  # one copy for every host-taken patch of the batch
                whole = plain()
            sources, described = [], []
            for i in rows:
                frame = resident[keys[i]]
                if frame is None:
                    sources.append(packed[slot[requests[i]]])
                    described.append(whole)
                else:
                    sources.append(frame)
                    described.append(descriptors[i])
            return launch(sources, described)

        distinct = list(dict.fromkeys(kinds or ()))
        if len(distinct) <= 1:
            return one_dtype(range(len(requests)))
        out = None
        for k in distinct:
            rows = [i for i, v in enumerate(kinds) if v == k]
            part = one_dtype(rows)
            if out is None:
                out = torch.empty((len(requests), *part.shape[1:]), dtype=torch.float32, device=part.device)
            out[torch.tensor(rows, device=part.device)] = part
        return out


# ------------------------------------------------------------------------------------------------ batch-side helpers
def identity(batch):
    return batch


def tree_to(tree, device):
    """the statistics of a normalisation tree on ``device``; a tensor that is there already stays the same object"""
    if isinstance(tree, dict):
        return {k: tree_to(v, device) for k, v in tree.items()}
    return tree.to(device) if torch.is_tensor(tree) else tree


def collate_norm_meta(norm_metas: list) -> dict:
    """per-sample ``{channel: {level: {stat: 0-d tensor}}}`` -> the same tree of (B,) tensors (_utils.py:174-191)"""
    out = {}
    for ch, levels in norm_metas[0].items():
        out[ch] = {}
        for level, stats in levels.items():
            out[ch][level] = None if stats is None else {st: torch.stack([m[ch][level][st] for m in norm_metas]) for st in stats}
    return out


def transform_channel_wise(transform, channel_names: list[str], patch: Tensor, norm_meta: list | None, extra: dict | None = None) -> Tensor:
    """_utils.py:194-229 with ``extra``: channels go into a dict under their names (B, 1, Z, Y, X) with the collated statistics
    (moved to the patch's device) and the extra entries (the ``_is_labelfree`` mask), through the dict transform, and back
    together in the dict's order without the extras"""
    channels = {name: patch[:, c : c + 1].contiguous() for name, c in zip(channel_names, range(patch.shape[1]))}
    if norm_meta is not None:
        channels["norm_meta"] = tree_to(collate_norm_meta(norm_meta), patch.device)
    if extra is not None:
        channels.update(extra)
    channels = transform(channels)
    for k in ("norm_meta",) + tuple(extra or ()):
        channels.pop(k, None)
    return torch.cat(list(channels.values()), dim=1)
