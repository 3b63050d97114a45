"""What tests/test_clip_host.py and tests/test_gpu_clip.py share: the meshes and cuts of "mesh clipping", the checker's
result of each (computed once), and the comparison of a ClippedMesh with it, array for array and bit for bit."""
import functools

import numpy as np

from mm_checkers import mesh_clip as Y
from test_section_host import CASES as SECTION_CASES
from test_section_host import cube, tilted_planes, tube

import multimoda_rs_amd as mm

KEEP, SCOPE = mm.clip.KEEP, mm.clip.SCOPE


def torus(n_major, n_minor, R=3.0, r=1.0, jitter=0.0, seed=0):
    """A torus around the z axis: vertex i n_minor + j at major angle i, minor angle j."""
    a = 2.0 * np.pi * np.arange(n_major) / n_major
    b = 2.0 * np.pi * np.arange(n_minor) / n_minor
    v = np.array([[(R + r * np.cos(y)) * np.cos(x), (R + r * np.cos(y)) * np.sin(x), r * np.sin(y)] for x in a for y in b])
    f = []
    for i in range(n_major):
        for j in range(n_minor):
            p, q = i * n_minor + j, i * n_minor + (j + 1) % n_minor
            s, t = ((i + 1) % n_major) * n_minor + j, ((i + 1) % n_major) * n_minor + (j + 1) % n_minor
            f += [(p, s, t), (p, t, q)]
    if jitter:
        v = v + np.random.default_rng(seed).uniform(-jitter, jitter, v.shape)
    return v, np.array(f, dtype=np.int64)


def _cases():
    """name -> (v, f, origins, normals, keep, scope, cap, extension)"""
    c = {}
    c["cube_plane_cap"] = (*cube(), [[0.5, 0.5, 0.5]], [[1.0, 0, 0]], "below", "plane", True, None)
    v, f, o, n = SECTION_CASES["two_arms"]
    c["two_arms_loop"] = (v, f, o[:1], n[:1], "below", "loop", False, None)
    c["two_arms_plane"] = (v, f, o[:1], n[:1], "below", "plane", False, None)
    v, f, o, n = SECTION_CASES["jittered_tube"]
    c["tube_both_ends"] = (v, f, o[[3, 20]], n[[3, 20]], ["above", "below"], "loop", True, (2.0, 3))
    c["tube_inward"] = (v, f[:, ::-1].copy(), o[[3, 20]], n[[3, 20]], ["above", "below"], "loop", True, (2.0, 3))
    v, f, o, n = SECTION_CASES["grid_tube"]
    c["grid_tube"] = (v, f, o[[38, 25]], n[[38, 25]], ["above", "below"], "loop", True, None)
    vt, ft = torus(24, 10, jitter=0.01, seed=2)
    c["torus_one_cut"] = (vt, ft, [[3.0, 0.1, 0.0]], [[0.05, 1.0, 0.0]], "below", "loop", False, None)
    c["torus_two_cuts"] = (vt, ft, [[3.0, 0.1, 0.0], [-3.0, 0.1, 0.0]], [[0.05, 1.0, 0.0], [-0.05, -1.0, 0.0]], ["below", "above"], "loop", True, None)
    c["torus_overlap"] = (vt, ft, [[3.0, 0.1, 0.0], [3.0, 0.11, 0.0]], [[0.05, 1.0, 0.0], [0.05, 1.0, 0.0]], ["below", "above"], "loop", False, None)
    c["torus_miss"] = (vt, ft, [[3.0, 0.1, 0.0], [0.0, 0.0, 9.0]], [[0.05, 1.0, 0.0], [0.0, 0.0, 1.0]], "below", "loop", False, None)
    # the smallest sizes at which the kernels take another path
    v, f = tube(8, 18, 1.0, 0.25, jitter=0.02, seed=6)
    c["faces_257"] = (v, f[:257], [[1.1, 0.0, 0.0]], [[1.0, 0.1, 0.0]], "below", "plane", True, None)
    v, f = tube(17, 241, 1.0, 0.1, jitter=0.004, seed=9)                  # 4097 vertices, 8160 faces: one past a scan tile
    c["scan_tiles"] = (v, f, [[3.03, 0.0, 0.0], [20.07, 0.0, 0.0]], [[1.0, 0.05, 0.0], [1.0, 0.0, 0.1]], ["above", "below"], "loop", True, (0.5, 2))
    v, f = tube(8, 600, 1.0, 0.05, jitter=0.002, seed=10)                 # long and thin: the unions leave chains to flatten
    c["long_thin"] = (v, f, [[15.02, 0.0, 0.0]], [[1.0, 0.02, 0.0]], "below", "loop", True, None)
    v, f = SECTION_CASES["two_arms"][:2]                                  # both ends of one arm, and the other arm dropped whole
    c["three_cuts"] = (v, f, [[0.6, 2.0, 0.5], [3.4, 2.0, 0.5], [2.0, 0.0, 0.0]], [[1.0, 0.05, 0.0], [1.0, 0.0, 0.05], [0.0, 2.0, 0.0]],
                       ["above", "below", "above"], ["loop", "loop", "plane"], True, (1.0, 2))
    c["open_tube_plane"] = (*tube(12, 4), [[0.2, 0.0, 0.0]], [[1.0, 0.0, 1.0]], "above", "plane", True, None)
    return c


CASES = _cases()


def codes(value, names, K):
    return [names[x] for x in ([value] * K if isinstance(value, str) else value)]


def check(v, f, o, n, keep, scope, cap, extension):
    K = len(o)
    return Y.clip(v, f, o, n, codes(keep, KEEP, K), codes(scope, SCOPE, K), int(cap), extension[0] if extension else 0.0,
                  extension[1] if extension else 0)


@functools.lru_cache(maxsize=None)
def checked(name):
    return check(*CASES[name])


def same_as_checker(got, want):
    """Every array equal in dtype, shape and bits; every count equal."""
    rim_off = np.concatenate([[0], np.cumsum([len(r) for rims in got.rims for r in rims])]).astype(np.int64)
    rim_index = np.concatenate([r for rims in got.rims for r in rims] + [np.zeros(0, dtype=np.int64)])
    status = np.stack([got.cut_status, got.cut_points, got.cut_loops, got.cut_faces], 1).reshape(-1, 4)
    measures = np.concatenate([got.cut_area[:, None], got.cut_length[:, None], got.cut_centroid], 1).reshape(-1, 5)
    mine = dict(vertices=got.vertices, faces=got.faces, vertex_origin=got.vertex_origin, face_origin=got.face_origin,
                face_kind=got.face_kind, cut_status=status, cut_measures=measures, rim_off=rim_off, rim_index=rim_index)
    for k in Y.ARRAYS:
        a, b = np.asarray(mine[k]), np.asarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
    for k in Y.COUNT_KEYS:
        assert got.report[k] == want["counts"][k], (k, got.report[k], want["counts"][k])
    return got


def run(name, fn, **kw):
    v, f, o, n, keep, scope, cap, extension = CASES[name]
    return same_as_checker(fn((v, f), o, n, keep=keep, scope=scope, cap=cap, extension=extension, **kw), checked(name))


def edge_report(faces):
    """(open, non-manifold, inconsistently oriented) edges of a face list, by counting directed edges."""
    f = np.asarray(faces)
    count = {}
    for a, b in np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).tolist():
        fwd, back = count.setdefault((min(a, b), max(a, b)), [0, 0])
        count[(min(a, b), max(a, b))] = [fwd + (a < b), back + (a > b)]
    n_open = sum(x + y == 1 for x, y in count.values())
    n_nonmanifold = sum(x + y > 2 for x, y in count.values())
    n_conflict = sum(x + y == 2 and x != y for x, y in count.values())
    return n_open, n_nonmanifold, n_conflict
