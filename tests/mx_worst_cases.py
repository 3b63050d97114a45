"""Worst-case inputs for the f16 hi + lo matrix-pipe kernels (the screen, k_screen_mx, and the bound rounds, k_bound_mx): the
constructions of the directed error search, shared by tests/test_gpu_mx_error_bound.py and
tests/test_gpu_bound_worst_cases.py.  Coordinates are in the kernels' scaled units (larger radius in [256, 512))."""
import numpy as np


def angles_far_from_unit_norm(n=96):
    a = np.linspace(-np.pi, np.pi, 200001)[:-1]
    c, s = np.cos(a).astype(np.float32).astype(np.float64), np.sin(a).astype(np.float32).astype(np.float64)
    dev = np.abs(c * c + s * s - 1.0)
    pick = np.argsort(dev)[-n:]
    return np.sort(a[pick])


def on_ties(rng, n, rmax, jitter):
    """n points on a rough circle of radius <= rmax (scaled units): both coordinates snapped to f16 ties at their own
    magnitude (spacing of f16 at |v|: 2^(floor(log2 |v|) - 10); a tie is an odd multiple of half of it), then moved by
    `jitter` f32 ulps."""
    t = np.sort(rng.uniform(0, 2 * np.pi, n))
    r = rmax * (1.0 - 0.3 * rng.uniform(0, 1, n) ** 4)
    p = np.stack([r * np.cos(t), r * np.sin(t)], axis=1)
    mag = np.maximum(np.abs(p), 2.0 ** -10)
    sp = 2.0 ** (np.floor(np.log2(mag)) - 10)
    q = (np.floor(p / sp) + 0.5) * sp                                   # odd multiples of sp / 2: exactly between two f16 values
    ulp32 = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(q), 2.0 ** -100))) - 23)
    q = q + jitter * ulp32
    # keep inside the radius
    nr = np.hypot(q[:, 0], q[:, 1])
    q[nr > rmax] *= (rmax / nr[nr > rmax])[:, None] * (1 - 1e-7)
    return q


def cases(rng):
    """(name, ref, tgt) in scaled units around the centre (0, 0)."""
    out = []
    for n in (64, 223, 449, 544, 600):
        for rmax in (511.9, 300.0, 256.01):
            for jit in (-1, 0, 1):
                out.append((f"ties n={n} r={rmax} jitter={jit}", on_ties(rng, n, rmax, jit), on_ties(rng, n, rmax, jit)))
        # tgt = ref moved by a fraction of the f16 spacing: tiny true distances out of large coordinates (cancellation)
        a = on_ties(rng, n, 511.9, 0)
        out.append((f"near-identical n={n}", a, a + rng.choice([-0.0625, 0.0625, 0.03125], size=a.shape)))
        # one far outlier fixes rho; everything else tiny (lo pieces below f16's normal range after scaling)
        small = rng.normal(0, 2.0 ** -9, (n, 2))
        far = small.copy(); far[0] = (500.0, -100.0)
        out.append((f"outlier-in-ref n={n}", far, small + 2.0 ** -11))
        out.append((f"outlier-in-tgt n={n}", small + 2.0 ** -11, far))
        # one pair decides: a ring of reference points, the targets ON them except one pushed out radially
        ring = on_ties(rng, n, 511.9, 0)
        tg = ring.copy()
        tg[n // 2] *= 0.75
        out.append((f"single-deciding-pair n={n}", ring, tg))
    return out
