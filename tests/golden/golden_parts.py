"""npz fixtures too large for one committed file (at most 1 MiB each) are kept as <name>_part<i>.npz: consecutive slices
of one key list.  save_parts writes them, GoldenParts reads them back as one read-only mapping with np.load's `files`."""
import glob
import os
import re

import numpy as np

MAX_PART_BYTES = 1000 * 1000       # below the 1 MiB limit


def part_paths(stem):
    paths = glob.glob(glob.escape(stem) + "_part*.npz")
    num = lambda p: int(re.search(r"_part(\d+)\.npz$", p).group(1))  # noqa: E731
    return sorted((p for p in paths if re.search(r"_part\d+\.npz$", p)), key=num)


def save_parts(stem, arrays, max_bytes=MAX_PART_BYTES):
    """np.savez_compressed of `arrays` (a dict, key order kept) as the fewest consecutive parts that each stay below
    max_bytes; returns the paths written.  Earlier parts of `stem` are removed first."""
    for p in part_paths(stem):
        os.remove(p)
    keys = list(arrays)
    total = sum(np.asarray(arrays[k]).nbytes for k in keys)
    for n in range(1, len(keys) + 1):
        chunks, cur, acc = [], [], 0
        for k in keys:
            nb = np.asarray(arrays[k]).nbytes
            if cur and acc + nb > total / n:
                chunks.append(cur)
                cur, acc = [], 0
            cur.append(k)
            acc += nb
        chunks.append(cur)
        paths = [f"{stem}_part{i + 1}.npz" for i in range(len(chunks))]
        for path, chunk in zip(paths, chunks):
            np.savez_compressed(path, **{k: arrays[k] for k in chunk})
        if all(os.path.getsize(p) < max_bytes for p in paths):
            return paths
        for p in paths:
            os.remove(p)
    raise ValueError(f"{stem}: an array alone compresses to {max_bytes} bytes or more")


class GoldenParts:
    """The arrays of every part of `stem`, looked up by key like an NpzFile."""

    def __init__(self, stem):
        self._data = {}
        self.files = []
        paths = part_paths(stem)
        if not paths:
            raise FileNotFoundError(f"no {stem}_part<i>.npz")
        for p in paths:
            with np.load(p) as z:
                for k in z.files:
                    self._data[k] = z[k]
                    self.files.append(k)

    def __getitem__(self, key):
        return self._data[key]

    def __contains__(self, key):
        return key in self._data
