"""Data sets of the HDBSCAN tests and helpers shared by them and by tests/golden/make_hdbscan.py.

Every set is generated from its seed with elementwise float64 operations only (no library reduction whose order could
depend on the build), then rounded to fp32; the fixture stores a SHA-256 of the fp32 bytes and, for the small sets, the
array itself."""
import hashlib

import numpy as np

# name -> generator arguments and the clustering parameters of the fixture (min_samples is the hdbscan package's: the row
# itself is not counted)
CASES = {
    "blobs2000": dict(kind="blobs", n=2000, dim=32, blobs=6, spread=0.03, seed=11, eps=0.01, single=False),
    "blobs6000a": dict(kind="blobs", n=6000, dim=32, blobs=12, spread=0.05, seed=12, eps=0.01, single=False),
    "blobs6000b": dict(kind="blobs", n=6000, dim=32, blobs=12, spread=0.12, seed=13, eps=0.01, single=False),
    "noisy1500": dict(kind="noisy", n=1500, dim=32, seed=14, eps=0.01, single=False),
    "small3d": dict(kind="blobs", n=300, dim=3, blobs=4, spread=0.05, seed=15, eps=0.01, single=False),
    "eps0": dict(kind="blobs", n=600, dim=32, blobs=5, spread=0.08, seed=16, eps=0.0, single=False),
    "single": dict(kind="blobs", n=400, dim=32, blobs=1, spread=0.05, seed=17, eps=0.0, single=True),
}
MIN_CLUSTER_SIZE = 10
MIN_SAMPLES = 10
STORE_X_UP_TO = 2000        # larger sets are regenerated from the seed and checked against the stored digest


def _unit(X):
    s = np.zeros(X.shape[0])
    for d in range(X.shape[1]):
        s = s + X[:, d] * X[:, d]
    return X / np.sqrt(s)[:, None]


def make_points(kind, n, dim, seed, blobs=0, spread=0.0, **_):
    """fp32 (n, dim) unit rows."""
    rng = np.random.default_rng(seed)
    if kind == "blobs":
        centres = _unit(rng.standard_normal((blobs, dim)))
        which = rng.integers(0, blobs, n)
        X = centres[which] + spread * rng.standard_normal((n, dim))
    elif kind == "noisy":
        # five blobs of unequal density and size, close enough to each other that they join into one component before
        # any point of the uniform background reaches them: the background is noise whichever point it links to (a
        # background point that met one blob first would belong to whichever blob the spanning tree's tie order gave it)
        spreads = np.array([0.008, 0.012, 0.02, 0.03, 0.04])
        sizes = [400, 300, 250, 150, 100]
        centres = _unit(_unit(rng.standard_normal((1, dim))) + 0.08 * rng.standard_normal((5, dim)))
        parts = [centres[b] + spreads[b] * rng.standard_normal((sizes[b], dim)) for b in range(5)]
        parts.append(rng.standard_normal((n - sum(sizes), dim)))
        X = np.concatenate(parts)[rng.permutation(n)]
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(_unit(X).astype(np.float32))


def digest(X):
    return hashlib.sha256(np.ascontiguousarray(X).tobytes()).hexdigest()


def case_points(name, golden):
    """The fp32 rows of a case: from the fixture when stored, else regenerated -- and checked against the digest either way."""
    key = f"{name}_X"
    X = golden[key] if key in golden.files else make_points(**CASES[name])
    assert digest(X) == str(golden[f"{name}_sha256"]), f"{name}: the regenerated rows differ from the fixture's"
    return X


def same_partition(a, b):
    """True when the labellings agree on every point up to a renaming of the cluster ids; noise (-1) must match noise."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or not np.array_equal(a < 0, b < 0):
        return False
    pairs = np.unique(np.stack([a, b], 1), axis=0)
    return len(np.unique(pairs[:, 0])) == len(pairs) == len(np.unique(pairs[:, 1]))
