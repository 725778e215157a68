"""Scenes of the mesh gradient tests (tests/test_mesh_grad_cpu.py, tests/test_gpu_mesh_grad.py): clip-space positions and triangles in
the manner of tests/mesh_render_inputs.py."""
import numpy as np

import mesh_render_inputs as inputs
import mesh_render_reference as ref

# NDC corners, z/w and faces of the silhouette scene.  Two quads overlap at different depths over an empty background (their outlines
# are boundaries, their diagonals regular interior edges, one quad has both windings); a folded pair: the faces (8, 9, 10) and
# (9, 8, 11) share the edge (8, 9) and lie on the same side of it; three faces share the edge (12, 13).
_NDC = np.array([[-0.8, -0.7], [0.3, -0.75], [0.35, 0.4], [-0.75, 0.45],             # the far quad
                 [-0.2, -0.3], [0.85, -0.2], [0.8, 0.8], [-0.25, 0.7],               # the near quad
                 [-0.9, 0.55], [-0.5, 0.95], [-0.95, 0.95], [-0.82, 0.88],           # the fold
                 [0.5, -0.9], [0.9, -0.5], [0.95, -0.95], [0.4, -0.55], [0.62, -0.35]])      # the three-face edge
_ZW = np.array([0.7, 0.72, 0.68, 0.7, 0.3, 0.32, 0.28, 0.3, 0.5, 0.5, 0.55, 0.4, 0.5, 0.5, 0.5, 0.45, 0.55])
TRI = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [7, 6, 4], [8, 9, 10], [9, 8, 11], [12, 13, 14], [13, 12, 15], [12, 13, 16]], np.int32)
TAGS = {"far": (0, 1), "near": (2, 3), "fold": (4, 5), "three": (6, 7, 8)}


def silhouette_views(B=2, seed=5):
    """(pos [B, 17, 4], tri [9, 3]): view 0 has w in 1 .. 2, every further view jitters the corners and has w spread over 1 .. 20 (strong
    perspective)."""
    rng = np.random.default_rng(seed)
    views = []
    for b in range(B):
        ndc = _NDC + (rng.uniform(-0.03, 0.03, _NDC.shape) if b else 0)
        w = rng.permutation(np.linspace(1, 20, len(_NDC))) if b else rng.uniform(1, 2, len(_NDC))
        views.append(inputs._clip(ndc, _ZW, w))
    return np.stack(views), TRI.copy()


def on_the_grid(pos, H, W):
    """pos with every vertex moved onto the sub-pixel grid point it snaps to (float32 positions that snap to the same integers), and
    those integers (X, Y)."""
    X, Y, ok = ref.snap(pos, H, W)
    assert ok.all()
    w = pos[..., 3].astype(np.float64)
    out = pos.astype(np.float64).copy()
    out[..., 0] = (2 * (X / 256) / W - 1) * w
    out[..., 1] = (2 * (Y / 256) / H - 1) * w
    out = out.astype(np.float32)
    X2, Y2, _ = ref.snap(out, H, W)
    assert np.array_equal(X, X2) and np.array_equal(Y, Y2)
    return out, X, Y


def rectangle(x_lo, x_hi, y_lo, y_hi, w, H, W, zw=0.5):
    """(pos [1, 4, 4], tri [2, 3]) of an axis-aligned rectangle with corners at the given snapped integer coordinates (1/256 pixel),
    corners in the order top-left, top-right, bottom-right, bottom-left, split along the diagonal (0, 2)."""
    XY = np.array([[x_lo, y_lo], [x_hi, y_lo], [x_hi, y_hi], [x_lo, y_hi]], np.float64) / 256
    ndc = np.stack((2 * XY[:, 0] / W - 1, 2 * XY[:, 1] / H - 1), 1)
    pos = inputs._clip(ndc, np.full(4, zw), np.full(4, float(w)))[None]
    X, Y, ok = ref.snap(pos, H, W)
    assert ok.all() and np.array_equal(X[0], [x_lo, x_hi, x_hi, x_lo]) and np.array_equal(Y[0], [y_lo, y_lo, y_hi, y_hi])
    return pos, np.array([[0, 1, 2], [0, 2, 3]], np.int32)
