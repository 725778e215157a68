"""Marching tetrahedra and tet_sdf_diff restated as a chain of torch operations, in the dtype and on the device of their arguments: the
algorithm of threestudio/models/isosurface.py:168-227 and threestudio/utils/ops.py:302-313 in this project's words.  It is the
reference of the tests (tests/test_isosurface_cpu.py pins it to tests/golden/isosurface.npz: faces exactly, values to 1e-12 in float64)
and the op chain that tools/bench_isosurface.py times the kernels against.  Like the reference it sorts on every call: a row-wise
`unique` over the six edges of every surface tetrahedron.

The two tables are the reference's triangle_table and num_triangles_table; they are data."""
import torch
import torch.nn.functional as F

TRIANGLE_TABLE = ((-1, -1, -1, -1, -1, -1), (1, 0, 2, -1, -1, -1), (4, 0, 3, -1, -1, -1), (1, 4, 2, 1, 3, 4), (3, 1, 5, -1, -1, -1),
                  (2, 3, 0, 2, 5, 3), (1, 4, 0, 1, 5, 4), (4, 2, 5, -1, -1, -1), (4, 5, 2, -1, -1, -1), (4, 1, 0, 4, 5, 1),
                  (3, 2, 0, 3, 5, 2), (1, 3, 5, -1, -1, -1), (4, 1, 2, 4, 3, 1), (3, 0, 4, -1, -1, -1), (2, 0, 1, -1, -1, -1),
                  (-1, -1, -1, -1, -1, -1))
NUM_TRIANGLES = (0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0)
EDGE_CORNERS = (0, 1, 0, 2, 0, 3, 1, 2, 1, 3, 2, 3)


def all_edges(tets):
    """[Ne, 2] int64: the unique edges of the tetrahedra, smaller index first, in lexicographic order."""
    pairs = tets.long()[:, list(EDGE_CORNERS)].reshape(-1, 2)
    return torch.unique(torch.sort(pairs, dim=1)[0], dim=0)


def marching_tetrahedra(pos, sdf, tets):
    """(v_pos [V, 3], faces [F, 3] int64) of pos [Nv, 3], sdf [Nv] or [Nv, 1] and tets [Ft, 4]; differentiable in pos and sdf."""
    dev = pos.device
    s = sdf.reshape(-1)
    tets = tets.long()
    with torch.no_grad():
        occ = s > 0
        corner_occ = occ[tets]                                                   # [Ft, 4]
        inside = corner_occ.sum(1)
        surface = (inside > 0) & (inside < 4)
        tets_s, corner_occ = tets[surface], corner_occ[surface]
        pairs = tets_s[:, list(EDGE_CORNERS)].reshape(-1, 2)
        pairs = torch.stack((pairs.min(1).values, pairs.max(1).values), 1)
        uniq, inverse = torch.unique(pairs, dim=0, return_inverse=True)
        crossing = occ[uniq[:, 0]] != occ[uniq[:, 1]]
        vertex_of = torch.full((uniq.shape[0],), -1, dtype=torch.long, device=dev)
        vertex_of[crossing] = torch.arange(int(crossing.sum()), dtype=torch.long, device=dev)
        tet_vertex = vertex_of[inverse].reshape(-1, 6)                           # per surface tetrahedron the vertex on each of its edges
        ends = uniq[crossing]
    a, b = ends[:, 0], ends[:, 1]
    s_a, n_b = s[a], -s[b]
    d = s_a + n_b
    v_pos = pos[a] * (n_b / d)[:, None] + pos[b] * (s_a / d)[:, None]
    case = (corner_occ.long() * torch.tensor([1, 2, 4, 8], device=dev)).sum(1)
    count = torch.tensor(NUM_TRIANGLES, device=dev)[case]
    table = torch.tensor(TRIANGLE_TABLE, device=dev)
    one, two = count == 1, count == 2
    faces = torch.cat((torch.gather(tet_vertex[one], 1, table[case[one]][:, :3]).reshape(-1, 3),
                       torch.gather(tet_vertex[two], 1, table[case[two]]).reshape(-1, 3)))
    return v_pos, faces


def normalize_grid_deformation(deformation, resolution, points_range=(0, 1)):
    return (points_range[1] - points_range[0]) / resolution * torch.tanh(deformation)


def tet_sdf_diff(vert_sdf, edges):
    """The scalar over the edges whose ends differ in torch.sign: mean bce_with_logits(s_a, s_b > 0) + mean bce_with_logits(s_b, s_a > 0)."""
    s = vert_sdf.reshape(-1)
    s_a, s_b = s[edges[:, 0]], s[edges[:, 1]]
    differ = torch.sign(s_a) != torch.sign(s_b)
    s_a, s_b = s_a[differ], s_b[differ]
    return (F.binary_cross_entropy_with_logits(s_a, (s_b > 0).to(s.dtype)) +
            F.binary_cross_entropy_with_logits(s_b, (s_a > 0).to(s.dtype)))


def scale_tensor(dat, inp_scale, tgt_scale):
    dat = (dat - inp_scale[0]) / (inp_scale[1] - inp_scale[0])
    return dat * (tgt_scale[1] - tgt_scale[0]) + tgt_scale[0]
