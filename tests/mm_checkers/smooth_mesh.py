"""Numpy restatement of the CCTA mesh finishing (multimodars/ccta/fixing_functions.py:52-92: the filter_taubin that ends
the post-processing; trimesh.smoothing.filter_taubin / filter_laplacian with equal weights): the yardstick for
csrc/mm_smooth_kernels.hip and csrc/mm_smooth.cpp.  trimesh is not available and its row order is a graph library's
insertion order, so the rules below are this package's definition (include/mm_ccta.h states the same).

* adjacency: the neighbours of v are the distinct w != v sharing a corner pair with v in some face; a face (a, a, b)
  gives a-b only, repeated faces nothing; row v ascending; deg(v) = its length, deg == 0 is isolated.
* one step with factor f, f64, per coordinate of a vertex with deg > 0:  w = 1.0 / deg;  acc = +0.0;  acc = acc + w * x_j
  over the neighbours ascending (the product is rounded, then the sum: numpy multiplies and adds elementwise, nothing is
  fused);  d = acc - x;  x' = x + f * d.  Every step reads the step before only.  Isolated and pinned vertices keep their
  bits; pinned vertices still feed their neighbours.
* filter_taubin: the factors lamb, -nu, lamb, ... (step 0 takes lamb); filter_laplacian: lamb every step.
* ring[v] = the fewest edges to a seed (0 at a seed), -1 beyond max_ring or unreachable.
* the report: stitch_mesh's pair-tree volume on the input and the output, max (dx dx + dy dy) + dz dz, and the launch
  counts include/mm_ccta.h states.
"""
import numpy as np

from . import stitch_mesh as SM

CSR_LAUNCHES = 7                # edge table, degrees, scan (3), fill, row sort


def csr(faces, nv):
    """(off (nv + 1), nb, info): info = entries, max_degree, isolated, n_edges, launches."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    pairs = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]) if f.shape[0] else np.zeros((0, 2), dtype=np.int64)
    pairs = pairs[pairs[:, 0] != pairs[:, 1]]
    both = np.unique(np.concatenate([pairs, pairs[:, ::-1]]), axis=0)      # sorted by (v, w): rows ascending
    deg = np.bincount(both[:, 0], minlength=nv).astype(np.int64) if nv else np.zeros(0, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    info = {"entries": int(both.shape[0]), "max_degree": int(deg.max()) if nv else 0, "isolated": int((deg == 0).sum()),
            "n_edges": int(both.shape[0]) // 2, "launches": CSR_LAUNCHES if nv and f.shape[0] else 0}
    return off, np.ascontiguousarray(both[:, 1]), info


def step(x, off, nb, factor, pinned=None):
    """One step on (nv, 3) coordinates; a new array."""
    deg = np.diff(off)
    order = np.argsort(-deg, kind="stable")                                 # the rows, longest first
    sdeg = deg[order]
    acc = np.zeros_like(x)
    with np.errstate(all="ignore"):
        w = 1.0 / np.maximum(deg, 1).astype(np.float64)
        for k in range(int(sdeg[0]) if len(sdeg) else 0):
            rows = order[:int(np.searchsorted(-sdeg, -k, side="left"))]     # the rows with deg > k
            prod = w[rows, None] * x[nb[off[rows] + k]]
            acc[rows] = acc[rows] + prod
        d = acc - x
        fd = np.float64(factor) * d
        out = x + fd
    keep = deg == 0
    if pinned is not None:
        keep = keep | (np.asarray(pinned).reshape(-1) != 0)
    out[keep] = x[keep]
    return out


def taubin_factors(lamb=0.5, nu=0.5, iterations=10):
    return [float(lamb) if i % 2 == 0 else -float(nu) for i in range(int(iterations))]


def volume(v, f):
    with np.errstate(all="ignore"):
        return SM.pair_tree_sum(SM.volume_terms(v, f)) / 6.0 if len(f) else 0.0


def volume_launches(nf):
    levels = 0
    while (1 << levels) < nf:
        levels += 1
    return 1 + max(1, (levels + 7) // 8)


def smooth(v, f, factors, pinned=None):
    """(vertices, report) after the steps `factors`."""
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(f, dtype=np.int64).reshape(-1, 3)
    nv, nf = v.shape[0], f.shape[0]
    off, nb, info = csr(f, nv)
    x = v.copy()
    for fac in factors:
        x = step(x, off, nb, fac, pinned)
    with np.errstate(all="ignore"):
        d = x - v
        disp = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    device = nv > 0 and nf > 0
    report = {"n_vertices": nv, "n_faces": nf, "n_edges": info["n_edges"], "n_isolated": info["isolated"],
              "n_pinned": int(np.count_nonzero(pinned)) if pinned is not None else 0, "max_degree": info["max_degree"],
              "steps_run": len(factors),
              "launches": CSR_LAUNCHES + len(factors) + 2 * volume_launches(nf) + 1 if device else 0,
              "volume_before": volume(v, f), "volume_after": volume(x, f),
              "max_displacement_sq": float(disp.max()) if device else 0.0}
    return x, report


def rings(f, nv, seeds, max_ring):
    """(ring (nv,) int32, info): info = reached, rounds (ring launches: the last may reach nothing), launches."""
    off, nb, cinfo = csr(f, nv)
    ring = np.full(nv, -1, dtype=np.int32)
    seeds = np.asarray(seeds, dtype=np.int64).reshape(-1)
    ring[seeds] = 0
    rounds = 0
    device = nv > 0 and len(np.asarray(f).reshape(-1, 3)) > 0 and seeds.size > 0
    src = np.repeat(np.arange(nv), np.diff(off))
    if device:
        for r in range(1, int(max_ring) + 1):
            rounds += 1
            hit = np.zeros(nv, dtype=bool)
            hit[src[ring[nb] == r - 1]] = True
            new = hit & (ring == -1)
            if not new.any():
                break
            ring[new] = r
    info = {"reached": int((ring >= 0).sum()), "rounds": rounds,
            "launches": CSR_LAUNCHES + 1 + rounds if device else 0}
    return ring, info
