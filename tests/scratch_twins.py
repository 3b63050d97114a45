"""Inputs that dirty the engine's grow-only scratch for tests/test_gpu_scratch_state.py, built on the host.

A twin has the counts of its original and other content: a call on the twin carves the same planes at the same offsets
and leaves in every one of them words that look valid to a call on the original -- owners that name real faces, corners
in range, keys of edges the original does not have.  A big input has at least twice the counts: the buffers grow, and the
original's planes then lie inside its leftovers."""
import dataclasses

import numpy as np

from test_refine_host import same_bits
from test_gpu_refine import bits_equal

# report fields that are no function of the input alone: the order in which the checked items of a pruned
# triangle search ran, and the rounds of the winding stage's pointer jumping
VOLATILE = ("items_run", "items_skipped", "items_skipped_step0", "winding_rounds")
JITTER = 0.01                                                             # well below the shortest edge of the test meshes


def twin_perm(n, seed):
    """The fixed relabelling of twin() and twin_points(): old index k becomes perm[k]; never the identity for n > 1."""
    perm = np.random.default_rng([seed, n, 1]).permutation(n)
    if n > 1 and np.array_equal(perm, np.arange(n)):
        perm = np.roll(perm, 1)
    return perm


def twin(v, f, seed):
    """(vertices, faces) with the nv and nf of (v, f): the vertices relabelled by twin_perm(nv, seed), the faces shuffled
    and each rolled (its winding kept), the coordinates jittered."""
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(f, dtype=np.int64).reshape(-1, 3)
    r = np.random.default_rng([seed, len(v), 2])
    perm = twin_perm(len(v), seed)
    tv = np.empty_like(v)
    tv[perm] = v + JITTER * r.standard_normal(v.shape)
    tf = perm[f][r.permutation(len(f))] if len(f) else f.copy()
    shift = r.integers(0, 3, len(tf))
    tf = np.take_along_axis(tf, (np.arange(3)[None, :] + shift[:, None]) % 3, axis=1) if len(tf) else tf
    return tv, np.ascontiguousarray(tf, dtype=np.int64)


def twin_points(p, seed, permute=True):
    """A point set (or a centerline's points) with the count of p: permuted by twin_perm and jittered.  permute=False
    keeps the order, for a centerline whose order is its meaning."""
    p = np.asarray(p, dtype=np.float64)
    flat = p.reshape(-1, p.shape[-1]) if p.ndim > 1 else p.reshape(-1, 1)
    r = np.random.default_rng([seed, len(flat), 3])
    moved = flat + JITTER * r.standard_normal(flat.shape)
    out = np.empty_like(moved)
    out[twin_perm(len(flat), seed) if permute else np.arange(len(flat))] = moved
    return out.reshape(p.shape)


def big(v, f):
    """(vertices, faces) with every face cut in four at its edge midpoints: nf -> 4 nf, nv -> nv + the edges (at least
    2 nv on a mesh without boundary; a mesh with fewer edges than vertices is cut again).  Shared edges share their
    midpoint, so closed manifolds stay closed and manifold."""
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(f, dtype=np.int64).reshape(-1, 3)
    nv0, nf0 = len(v), len(f)
    assert nf0 > 0
    while len(v) < 2 * nv0 or len(f) < 2 * nf0:
        e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
        uniq, inv = np.unique(e, axis=0, return_inverse=True)
        mid = len(v) + inv.reshape(3, len(f)).T                          # column k: the midpoint of corner k -> k + 1
        v = np.concatenate([v, 0.5 * (v[uniq[:, 0]] + v[uniq[:, 1]])])
        a, b, c = f[:, 0], f[:, 1], f[:, 2]
        ab, bc, ca = mid[:, 0], mid[:, 1], mid[:, 2]
        f = np.concatenate([np.stack(t, axis=1) for t in ((a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca))])
    return v, np.ascontiguousarray(f, dtype=np.int64)


def big_points(p, seed=0):
    """A point set of three times the count: p, and two shifted twins of it."""
    p = np.asarray(p, dtype=np.float64)
    return np.concatenate([p, twin_points(p, seed + 1) + 0.37, twin_points(p, seed + 2) - 0.41])


# ---- bit-for-bit comparison of whole results ------------------------------------------------------------------------------

def leaves(x, path="r"):
    """(path, leaf) over tuples, lists, dicts, dataclasses and plain objects; a leaf is an array or a scalar."""
    if isinstance(x, dict):
        for k in sorted(x, key=str):
            if k not in VOLATILE:
                yield from leaves(x[k], f"{path}[{k!r}]")
    elif isinstance(x, (tuple, list)):
        yield path + ".len", len(x)
        for k, y in enumerate(x):
            yield from leaves(y, f"{path}[{k}]")
    elif dataclasses.is_dataclass(x):
        for fld in dataclasses.fields(x):
            yield from leaves(getattr(x, fld.name), f"{path}.{fld.name}")
    elif isinstance(x, (np.ndarray, np.generic, int, float, bool, str, type(None))):
        yield path, x
    else:
        yield from leaves({k: v for k, v in vars(x).items() if not k.startswith("_")}, path)


def same_leaf(x, y):
    """Bit for bit: same_bits on f64 arrays, bits_equal on floats (a NaN equals only a NaN of its own bits), the bytes of
    any other array with its dtype and shape, == on integers, flags, strings and None."""
    if isinstance(x, np.ndarray) or isinstance(y, np.ndarray):
        if not (isinstance(x, np.ndarray) and isinstance(y, np.ndarray)) or x.dtype != y.dtype or x.shape != y.shape:
            return False
        if x.dtype == np.float64:
            return bool(same_bits(x, y))
        return np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes()
    floats = (float, np.floating)
    if isinstance(x, floats) or isinstance(y, floats):
        return isinstance(x, floats) and isinstance(y, floats) and bool(bits_equal(x, y))
    if isinstance(x, (bool, np.bool_, int, np.integer)) and isinstance(y, (bool, np.bool_, int, np.integer)):
        return int(x) == int(y)
    return type(x) is type(y) and x == y


def differences(a, b):
    """The paths at which two results differ in a bit (or in shape, type or structure)."""
    la, lb = list(leaves(a)), list(leaves(b))
    if [p for p, _ in la] != [p for p, _ in lb]:
        return ["structure: " + ", ".join(sorted({p for p, _ in la} ^ {p for p, _ in lb})[:8])]
    return [p for (p, x), (_, y) in zip(la, lb) if not same_leaf(x, y)]


def uploads(x):
    return [v for p, v in leaves(x) if p.endswith("['bytes_uploaded']") or p.endswith(".bytes_uploaded")]
