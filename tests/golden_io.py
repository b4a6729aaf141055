"""Reading and writing the golden fixtures (tests/golden/*.npz).

No file in the repository may exceed 1 MiB, so a fixture whose compressed archive would is stored as parts
`<stem>.part0.npz`, `<stem>.part1.npz`, ... that split its arrays by key, in order; `load_golden` reads either form
back as one mapping with the `.files` list of an `np.load` result.
"""
import glob
import os

import numpy as np

PART_BYTES = 900 * 1000     # raw array bytes per part: its compressed archive stays below 1 MiB


class Golden(dict):
    @property
    def files(self):
        return list(self)


def load_golden(golden_dir, name):
    """The arrays of fixture `name` ("x.npz"), whether stored as one archive or in parts."""
    stem = os.path.join(golden_dir, name[:-len(".npz")])
    paths = [stem + ".npz"] if os.path.exists(stem + ".npz") else \
        sorted(glob.glob(glob.escape(stem) + ".part*.npz"), key=lambda p: int(p[len(stem) + 5:-4]))
    if not paths:
        raise FileNotFoundError(stem + ".npz")
    out = Golden()
    for p in paths:
        with np.load(p) as z:
            for k in z.files:
                out[k] = z[k]
    return out


def save_golden(path, arrays):
    """Write `arrays` as `path` ("x.npz"), or as x.partN.npz when that one archive would exceed 1 MiB.  An array
    larger than PART_BYTES gets a part of its own (which must still compress below the limit)."""
    stem = path[:-len(".npz")]
    for old in [path] + glob.glob(glob.escape(stem) + ".part*.npz"):
        if os.path.exists(old):
            os.remove(old)
    np.savez_compressed(path, **arrays)
    if os.path.getsize(path) <= 1 << 20:
        return [path]
    os.remove(path)
    parts, cur, size = [], {}, 0
    for k, v in arrays.items():
        n = np.asarray(v).nbytes
        if cur and size + n > PART_BYTES:
            parts.append(cur)
            cur, size = {}, 0
        cur[k] = v
        size += n
    parts.append(cur)
    paths = []
    for i, part in enumerate(parts):
        paths.append(f"{stem}.part{i}.npz")
        np.savez_compressed(paths[-1], **part)
        assert os.path.getsize(paths[-1]) <= 1 << 20, paths[-1]
    return paths
