"""The culled screen's split layout (csrc/mm_tile_bound.h: mm_tile_slot_point, mm_tile_split_main), checked on the host.

A search set is lumen ++ catheter.  Cut into tiles of 32 consecutive points it has a tile that holds the end of the lumen
and the start of the catheter, whose bounding circle is far from no other tile.  The split layout gives each run tiles of
its own: slot j holds point min(j, main - 1) below 32 ceil(main / 32) and main + min(j - 32 ceil(main / 32), n - main - 1)
from there on.  Checked here: the mapping for every small (main, n) (mm_tile_slot_map), when the engine takes it, and the
tile bound of the split layout (mm_tile_bound_probe_split) through the f64 containment and thr <= low checks of
tests/test_tile_bound_host.py on a contour with a catheter ring."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

U = 2.0 ** -24


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as ge
    ge.build()
    import multimoda_rs_amd as mm
    return mm._native


def _slot_map(native, n, main, slots):
    out = np.full(slots, -7, dtype=np.int32)
    rc = native.lib().mm_tile_slot_map(int(n), int(main), int(slots), out.ctypes.data_as(C.c_void_p))
    assert rc >= 0, native.last_error()
    return out, rc


def test_mapping_exhaustive(native):
    """Every (main, n) with n <= 100 and 0 < main < n, over the slots of one tile more than the layout needs: every point
    has a slot, a padding slot repeats a point of its own run, the runs sit in order and each starts a tile."""
    for n in range(2, 101):
        for main in range(1, n):
            edge = (main + 31) // 32 * 32
            tiles = edge // 32 + (n - main + 31) // 32
            slots = 32 * (tiles + 1)
            m, _ = _slot_map(native, n, main, slots)
            assert m.min() >= 0 and m.max() == n - 1
            assert set(m[:32 * tiles].tolist()) == set(range(n))                 # every point appears
            assert (m[:main] == np.arange(main)).all()                            # the first run in order, from slot 0
            assert (m[main:edge] == main - 1).all()                               # its padding: its own last point
            assert (m[edge:edge + n - main] == np.arange(main, n)).all()          # the second run from a tile edge
            assert (m[edge + n - main:] == n - 1).all()                           # its padding: its own last point
            assert (np.diff(m) >= 0).all()


def test_no_split_is_the_identity_clamp(native):
    for n in (1, 2, 31, 32, 33, 64, 73, 521, 544):
        m, take = _slot_map(native, n, 0, 32 * ((n + 31) // 32) + 40)
        assert take == 0
        assert (m == np.minimum(np.arange(len(m)), n - 1)).all()


def test_split_is_taken_where_it_adds_no_tile(native):
    """The engine's condition: ceil(main / 32) + ceil((n - main) / 32) == ceil(n / 32)."""
    t = lambda k: (k + 31) // 32
    for n in range(2, 200):
        for main in range(1, n):
            _, take = _slot_map(native, n, main, 0)
            assert take == (main if t(main) + t(n - main) == t(n) else 0), (n, main, take)
    shapes = {(501, 20): True, (53, 20): True, (64, 20): True, (53, 32): True, (200, 23): False, (40, 20): False,
              (44, 20): False, (53, 40): False, (85, 40): False, (90, 70): False, (60, 36): False}
    for (lum, cath), ok in shapes.items():
        assert (_slot_map(native, lum + cath, lum, 0)[1] == lum) == ok, (lum, cath)
    # a catheter run of two tiles (33 .. 64 points) that qualifies needs a lumen run whose remainder and the catheter's
    # sum past 32: 60 + 37 (97 points: 4 tiles, split 2 + 2)
    assert _slot_map(native, 97, 60, 0)[1] == 60


def test_bad_arguments(native):
    out = np.zeros(4, dtype=np.int32)
    P = out.ctypes.data_as(C.c_void_p)
    for n, main, slots in ((0, 0, 4), (10, -1, 4), (10, 10, 4), (10, 11, 4), (10, 3, -1)):
        assert native.lib().mm_tile_slot_map(n, main, slots, P) < 0


# ---- the tile bound of the split layout against f64 (the checks of tests/test_tile_bound_host.py) ----

def _f32_fma(a, b, c):
    return (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(np.float32)


def _probe(native, ref, tgt, mains, e, c, s, e2):
    rx, ry = (np.ascontiguousarray(ref[:, k], dtype=np.float32) for k in (0, 1))
    tx, ty = (np.ascontiguousarray(tgt[:, k], dtype=np.float32) for k in (0, 1))
    nrt, nct = (len(rx) + 31) // 32, (len(tx) + 31) // 32
    circ = np.zeros(4 * (nrt + nct), dtype=np.float32)
    thr = np.zeros(nrt * nct, dtype=np.float32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = native.lib().mm_tile_bound_probe_split(P(rx), P(ry), len(rx), P(tx), P(ty), len(tx), int(mains[0]), int(mains[1]),
                                                int(e), C.c_float(c), C.c_float(s), float(e2), P(circ), P(thr))
    assert rc == 0, native.last_error()
    return (rx, ry, tx, ty), circ.reshape(-1, 4), thr.reshape(nrt, nct)


def _check(native, ref, tgt, mains, angles):
    """ref, tgt: f64 sets around the rotation centre (0, 0), laid out by `mains`; every circle and threshold against f64."""
    ref32, tgt32 = ref.astype(np.float32), tgt.astype(np.float32)
    ra = np.hypot(ref32[:, 0].astype(np.float64), ref32[:, 1].astype(np.float64)).max()
    rb = np.hypot(tgt32[:, 0].astype(np.float64), tgt32[:, 1].astype(np.float64)).max()
    e = 9 - int(np.frexp(max(ra, rb) * (1.0 + 1e-6))[1])
    R = ra + rb
    e2 = U * (47 * R * R + 6 * ra * ra + 27 * rb * rb)
    S = np.float32(2.0 ** e)
    nrt, nct = (len(ref) + 31) // 32, (len(tgt) + 31) // 32
    rmap, _ = _slot_map(native, len(ref), mains[0], 32 * nrt)
    cmap, _ = _slot_map(native, len(tgt), mains[1], 32 * nct)
    skipped = 0
    for ang in angles:
        c, s = np.float32(np.cos(ang)), np.float32(np.sin(ang))
        (rx, ry, tx, ty), circ, thr = _probe(native, ref32, tgt32, mains, e, c, s, e2)
        ax, ay = (S * rx).astype(np.float64), (S * ry).astype(np.float64)
        bx, by = S * tx, S * ty
        ex = bx.astype(np.float64) * np.float64(c) - by.astype(np.float64) * np.float64(s)
        ey = bx.astype(np.float64) * np.float64(s) + by.astype(np.float64) * np.float64(c)
        kx = _f32_fma(bx, c, -(by * s)).astype(np.float64)
        ky = _f32_fma(bx, s, by * c).astype(np.float64)
        e2s = e2 * 2.0 ** (2 * e)
        for i in range(nrt):
            idx = rmap[32 * i:32 * i + 32]
            assert (np.hypot(ax[idx] - circ[i, 0], ay[idx] - circ[i, 1]) <= circ[i, 2]).all()
        for j in range(nct):                                               # the rotated circle holds the rotated points
            idx = cmap[32 * j:32 * j + 32]
            assert (np.hypot(ex[idx] - circ[nrt + j, 0], ey[idx] - circ[nrt + j, 1]) <= circ[nrt + j, 2] + 2.0 ** -11).all()
        for i in range(nrt):
            ri = rmap[32 * i:32 * i + 32]
            for j in range(nct):
                if not thr[i, j] > 0:
                    continue
                skipped += 1
                cj = cmap[32 * j:32 * j + 32]
                d2e = (ax[ri, None] - ex[None, cj]) ** 2 + (ay[ri, None] - ey[None, cj]) ** 2
                d2k = (ax[ri, None] - kx[None, cj]) ** 2 + (ay[ri, None] - ky[None, cj]) ** 2
                low = min(d2e.min(), d2k.min()) - e2s
                assert float(thr[i, j]) <= low, (ang, i, j, float(thr[i, j]), low)
    return skipped, thr


def _lumen_and_catheter(rng, n_lumen, n_cath, r=2.2, shift=(0.3, -0.2)):
    """A wobbling lumen contour around the rotation centre and a catheter ring of radius 0.5 off its middle."""
    t = np.linspace(0, 2 * np.pi, n_lumen, endpoint=False)
    rr = r * (1 + 0.1 * np.sin(3 * t + rng.uniform(0, 6)))
    lum = np.stack([rr * np.cos(t), 0.8 * rr * np.sin(t)], axis=1)
    u = np.linspace(0, 2 * np.pi, n_cath, endpoint=False)
    cath = np.stack([shift[0] + 0.5 * np.cos(u), shift[1] + 0.5 * np.sin(u)], axis=1)
    return np.concatenate([lum, cath])


ANGLES = np.concatenate([np.linspace(-np.pi, np.pi, 13)[:-1], [0.0, 1e-7, np.pi / 2, 0.7853981633974483]])


@pytest.mark.parametrize("lum,cath", [(501, 20), (53, 20), (64, 20), (53, 32), (60, 37)])
def test_split_bound_holds_on_a_contour_with_a_catheter(native, lum, cath):
    rng = np.random.default_rng(lum + cath)
    a = _lumen_and_catheter(rng, lum, cath)
    b = _lumen_and_catheter(rng, lum, cath, r=2.3, shift=(-0.2, 0.25))
    for mains in ((lum, lum), (lum, 0), (0, lum)):
        _check(native, a, b, mains, ANGLES)


def test_split_frees_the_lumens_last_tile(native):
    """501 + 20: in consecutive tiles, tile 15 (lumen end and catheter start) is close to far more column tiles than in
    the split layout, where the catheter has tile 16 to itself -- the reason for the layout."""
    rng = np.random.default_rng(7)
    a = _lumen_and_catheter(rng, 501, 20)
    b = _lumen_and_catheter(rng, 501, 20, r=2.3, shift=(-0.2, 0.25))
    n0, thr0 = _check(native, a, b, (0, 0), [0.3])
    n1, thr1 = _check(native, a, b, (501, 501), [0.3])
    assert n1 > n0
    assert (~(thr1[15] > 0)).sum() < (~(thr0[15] > 0)).sum()
    # the probe without a split is the existing probe, bit for bit
    rx, ry = (np.ascontiguousarray(a[:, k], dtype=np.float32) for k in (0, 1))
    tx, ty = (np.ascontiguousarray(b[:, k], dtype=np.float32) for k in (0, 1))
    circ = np.zeros(4 * 34, dtype=np.float32)
    thr = np.zeros(17 * 17, dtype=np.float32)
    P = lambda v: v.ctypes.data_as(C.c_void_p)
    c, s = np.float32(np.cos(0.3)), np.float32(np.sin(0.3))
    _, circ0, thr_s = _probe(native, a.astype(np.float32), b.astype(np.float32), (0, 0), 6, c, s, 1e-6)
    assert native.lib().mm_tile_bound_probe(P(rx), P(ry), 521, P(tx), P(ty), 521, 6, C.c_float(c), C.c_float(s), 1e-6,
                                            P(circ), P(thr)) == 0
    assert (circ.view(np.uint32) == circ0.ravel().view(np.uint32)).all()
    assert (thr.view(np.uint32) == thr_s.ravel().view(np.uint32)).all()
