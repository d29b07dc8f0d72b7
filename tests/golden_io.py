"""Golden fixtures under tests/golden/ are .npz files of at most 1 MiB each.  A fixture too large for one file is stored as
<name>.part0.npz, <name>.part1.npz, ... (consecutive runs of its arrays, in the original order); ``load`` reads either form."""
import glob
import io
import os
import re

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PART_BYTES = 1000 * 1000            # compressed bytes per part file (< 1 MiB with the zip directory)


class Golden:
    """the arrays of a (possibly split) fixture: g[key], key in g, g.files in the original order"""

    def __init__(self, arrays):
        self._arrays = arrays
        self.files = list(arrays)

    def __getitem__(self, key):
        return self._arrays[key]

    def __contains__(self, key):
        return key in self._arrays


def _parts(path):
    stem = path[:-len(".npz")]
    found = glob.glob(glob.escape(stem) + ".part*.npz")
    idx = {int(re.search(r"\.part(\d+)\.npz$", p).group(1)): p for p in found}
    assert sorted(idx) == list(range(len(idx))), f"{stem}: parts {sorted(idx)} are not 0..n-1"
    return [idx[i] for i in range(len(idx))]


def load(name):
    """tests/golden/<name>.npz, or its parts"""
    path = os.path.join(GOLDEN, name + ".npz")
    if os.path.exists(path):
        return np.load(path)
    parts = _parts(path)
    if not parts:
        raise FileNotFoundError(path)
    arrays = {}
    for p in parts:
        with np.load(p) as z:
            for k in z.files:
                arrays[k] = z[k]
    return Golden(arrays)


def save(path, **arrays):
    """np.savez_compressed(path, **arrays), split into parts of at most PART_BYTES when one file would be larger"""
    for p in _parts(path) + ([path] if os.path.exists(path) else []):
        os.remove(p)

    def size(d):
        buf = io.BytesIO()
        np.savez_compressed(buf, **d)
        return buf.tell()

    if size(arrays) <= PART_BYTES:
        np.savez_compressed(path, **arrays)
        return [path]
    groups, cur = [], {}
    for k, v in arrays.items():
        if cur and size({**cur, k: v}) > PART_BYTES:
            groups.append(cur)
            cur = {}
        cur[k] = v
    groups.append(cur)
    out = []
    for i, g in enumerate(groups):
        assert size(g) <= PART_BYTES, f"{path}: array {list(g)} alone is larger than {PART_BYTES} bytes compressed"
        out.append(path[:-len(".npz")] + f".part{i}.npz")
        np.savez_compressed(out[-1], **g)
    return out
