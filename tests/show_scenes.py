"""Inputs shared by tests/test_show_cli.py and tests/test_show_gpu.py: the unit cube as a mesh and as a wireframe, and random primitives
placed in screen space under a given camera."""
import numpy as np


def cube(half=0.5):
    """-> verts [8,3], faces [12,3] int32, edges [12,2,3]."""
    v = np.array([[x, y, z] for x in (-half, half) for y in (-half, half) for z in (-half, half)], dtype=np.float64)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    faces = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], dtype=np.int32)
    pairs = [(i, j) for i in range(8) for j in range(i + 1, 8) if np.sum(v[i] != v[j]) == 1]
    return v, faces, np.stack([v[[i, j]] for i, j in pairs])


def unproject(w2c, K, xy, z):
    """Screen points xy [n,2] at camera depth z [n] -> world [n,3]."""
    xy, z = np.asarray(xy, dtype=np.float64), np.asarray(z, dtype=np.float64)
    c = np.stack([(xy[:, 0] - K[0, 2]) * z / K[0, 0], (xy[:, 1] - K[1, 2]) * z / K[1, 1], z, np.ones_like(z)], 1)
    return (np.linalg.inv(w2c) @ c.T).T[:, :3]


def random_segments(rng, n, w2c, K, W, H, margin=20.0):
    """n segments whose ends lie up to `margin` pixels outside the W x H frame, at depths 1.5 .. 4."""
    xy = rng.uniform([-margin, -margin], [W - 1 + margin, H - 1 + margin], size=(2 * n, 2))
    return unproject(w2c, K, xy, rng.uniform(1.5, 4.0, 2 * n)).reshape(n, 2, 3)


def random_triangles(rng, n, w2c, K, W, H, size=14.0, margin=10.0):
    """n triangles -> verts [3n,3], faces [n,3]: a centre anywhere in the frame (and a little outside), corners within `size` pixels of it."""
    c = rng.uniform([-margin, -margin], [W - 1 + margin, H - 1 + margin], size=(n, 1, 2))
    xy = (c + rng.uniform(-size, size, size=(n, 3, 2))).reshape(-1, 2)
    z = (rng.uniform(1.5, 4.0, (n, 1)) + rng.uniform(-0.3, 0.3, (n, 3))).reshape(-1)
    return unproject(w2c, K, xy, z), np.arange(3 * n, dtype=np.int32).reshape(n, 3)
