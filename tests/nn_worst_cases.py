"""Point clouds on which the box bounds of the nearest-neighbour work lists (csrc/mm_ccta.cpp: NnPlan; kernels
csrc/mm_nn_kernels.hip) are easiest to get wrong, shared by tests/test_nn_plan_host.py (the work lists, host only) and
tests/test_gpu_prune_worst_cases.py (the device results against the oracle).

Each case is (name, queries, points, r2): r2 is one grid spacing squared where the case has a grid, so that neighbours
sit exactly on the radius."""
import numpy as np

SORT_MIN = 4096   # sets of this many points or more are staged in slab order (kSortMin)


def _tube(rng, n, length=60.0, radius=2.0, centre=(0.0, 0.0, 0.0)):
    t = rng.uniform(0.0, length, n)
    a = rng.uniform(0.0, 2.0 * np.pi, n)
    return np.stack([radius * np.cos(a), radius * np.sin(a), t], axis=1) + np.asarray(centre)


def flat(rng, axes):
    """One (axes = 1) or two (axes = 2: collinear) constant coordinates."""
    a = rng.normal(0.0, 5.0, size=(5000, 3))
    b = rng.normal(0.0, 5.0, size=(4600, 3))
    a[:, 3 - axes:] = 1.25
    b[:, 3 - axes:] = 1.25
    return a, b


def grid():
    """Integer grids one spacing apart: every gap between boxes and every neighbour distance is exact, and each query
    has neighbours exactly on the radius (r2 = 1)."""
    g = np.stack(np.meshgrid(np.arange(17.0), np.arange(17.0), np.arange(17.0), indexing="ij"), axis=-1).reshape(-1, 3)
    return g[g[:, 0] < 16] + [0.0, 0.0, 1.0], g


def offset(rng, off):
    """Sub-mm clouds far from the origin: the boxes' gaps are a few ulps of the coordinates."""
    a = rng.normal(0.0, 3e-4, size=(4500, 3)) + [off, -off, 0.5 * off]
    b = rng.normal(0.0, 3e-4, size=(5200, 3)) + [off, -off, 0.5 * off]
    b[:4000:3] = a[:4000:3]                       # exact coincidences: minima of 0
    return a, b


def duplicates(rng):
    """Every point three times: the copies land on both sides of chunk and block borders."""
    u = _tube(rng, 1700)
    b = np.repeat(u, 3, axis=0)[rng.permutation(5100)]
    a = np.concatenate([u, u + [0.0, 0.0, 0.01], u[:1200]])
    return a, b


def clusters(rng):
    """Two clusters 1000 mm apart in each cloud."""
    a = np.concatenate([rng.normal(0, 2, (2500, 3)), rng.normal(0, 2, (2500, 3)) + [1000.0, 0.0, 0.0]])
    b = np.concatenate([rng.normal(0, 2, (2100, 3)) + [0.0, 0.0, 3.0], rng.normal(0, 2, (2600, 3)) + [1003.0, 0.0, 0.0]])
    return a, b


def nonfinite(rng):
    """NaN and +-inf coordinates among finite points, in both clouds (a NaN distance never lowers a minimum)."""
    a = rng.normal(0, 4, (4700, 3))
    b = rng.normal(0, 4, (4400, 3))
    for m in (a, b):
        rows = rng.choice(len(m), 60, replace=False)
        for k, r in enumerate(rows):
            m[r, k % 3] = (np.nan, np.inf, -np.inf)[k % 3]
        m[rows[:4]] = np.nan                      # whole rows
    return a, b


def block_max(rng):
    """Only the rule "skip an item when lb2 >= the LARGEST current minimum of its query block" gets this right: one
    query block holds queries right on the point line (pass A's chunk brings their minima to ~0) and queries 60 mm
    above it whose nearest points are a cluster in a chunk 40 mm further along.  Both clouds are longest along x, so
    the slab order keeps the two kinds of queries in one block."""
    x = np.linspace(0.0, 100.0, 8000)
    b = np.concatenate([np.stack([x, np.zeros_like(x), np.zeros_like(x)], axis=1),
                        np.stack([90.0 + rng.uniform(0, 0.1, 200), 50.0 + rng.uniform(0, 0.1, 200), np.zeros(200)], axis=1)])
    xa = np.linspace(0.0, 100.0, 6000)
    a = np.stack([xa, np.full_like(xa, 0.5), np.zeros_like(xa)], axis=1)
    far = np.stack([50.0 + np.arange(8) * 1e-3, np.full(8, 60.0), np.zeros(8)], axis=1)
    return np.concatenate([a[:3000], far, a[3000:]]), b


def sized(rng, nq, np_):
    a = _tube(rng, nq)
    b = _tube(rng, np_) + [0.0, 0.0, 0.5]
    return a, b


def cases():
    rng = np.random.default_rng(20261016)
    out = [("flat1", *flat(rng, 1), 1.0), ("flat2", *flat(rng, 2), 1.0), ("grid", *grid(), 1.0)]
    for off in (1e4, 1e6):
        out.append((f"offset{off:g}", *offset(rng, off), 1e-7))
    out += [("duplicates", *duplicates(rng), 0.25), ("clusters", *clusters(rng), 1.0),
            ("nonfinite", *nonfinite(rng), 1.0), ("block_max", *block_max(rng), 1.0)]
    for nq, np_ in ((4095, 4097), (4096, 4096), (4097, 4095), (511, 4096), (512, 1000), (513, 1500), (4100, 1500)):
        out.append((f"n{nq}x{np_}", *sized(rng, nq, np_), 0.5))
    return out


def radial(rng, n):
    """Unit vectors and move flags for the morphed copies of a cloud (as the scaling searches build them)."""
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return u, (rng.uniform(size=n) < 0.8).astype(np.uint8)
