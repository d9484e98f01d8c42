"""TEST INFRASTRUCTURE ONLY -- reading and writing the fixture files under ``tests/golden/``.

A fixture over the 1 MiB limit of a committed file is stored as ``<stem>.npz`` plus ``<stem>_part<k>.npz``, and a matrix
``<key>`` that is symmetric only up to round-off (an LU inverse) as its upper triangle ``<key>__triu`` plus the residual
``<key>__tril_resid`` = lower - upper^T, which restores every bit of the lower triangle.  ``load`` returns the merged
arrays under their original names; a fixture stored whole comes back as ``np.load`` gives it.
"""
import glob
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


def encode_nearly_symmetric(m):
    """(upper triangle incl. diagonal, lower triangle - upper^T) of a square matrix: lossless for an LU inverse."""
    n = m.shape[0]
    il = np.tril_indices(n, -1)
    return m[np.triu_indices(n)], m[il] - m.T[il]


def decode_nearly_symmetric(upper, resid):
    n = int(round((np.sqrt(8 * upper.size + 1) - 1) / 2))
    m = np.zeros((n, n), dtype=upper.dtype)
    m[np.triu_indices(n)] = upper
    il = np.tril_indices(n, -1)
    m[il] = m.T[il] + resid
    return m


def save_split(path, parts, nearly_symmetric=()):
    """Write the dicts of ``parts`` to <path> and <stem>_part2.npz, ... (compressed), every key of ``nearly_symmetric``
    in the triangle + residual form."""
    stem = path[:-len(".npz")]
    for k, part in enumerate(parts):
        out = {}
        for key, v in part.items():
            if key in nearly_symmetric:
                out[key + "__triu"], out[key + "__tril_resid"] = encode_nearly_symmetric(v)
            else:
                out[key] = v
        np.savez_compressed(path if k == 0 else f"{stem}_part{k + 1}.npz", **out)


def load(name, root=GOLDEN):
    """Fixture ``name`` (a file name under tests/golden/), its parts merged and its split matrices rebuilt."""
    path = os.path.join(root, name)
    z = np.load(path)
    parts = sorted(glob.glob(path[:-len(".npz")] + "_part*.npz"))
    if not parts and not any(k.endswith("__triu") for k in z.files):
        return z
    d = dict(z)
    for p in parts:
        d.update(np.load(p))
    for k in [k for k in d if k.endswith("__triu")]:
        key = k[:-len("__triu")]
        d[key] = decode_nearly_symmetric(d.pop(k), d.pop(key + "__tril_resid"))
    return d
