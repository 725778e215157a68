"""Iso-surface of a regular grid as an indexed triangle mesh (csrc/field.hip: marching tetrahedra on the Kuhn decomposition;
include/gip_model.h gip_surface_count / gip_surface_emit), and Wavefront OBJ / binary PLY writers and readers for it, with optional
per-vertex colours and normals.  Also the cleaning and decimation of such a mesh on the GPU (csrc/mesh_clean.hip): connected_components,
clean_mesh, cluster_decimate, decimate_mesh.

The reference hands its density grid to the third-party `mcubes` (gs_renderer.py:338-340); here the surface is extracted on the
GPU.  There is no CPU path: a tensor that is not a float32 GPU tensor is an error."""
import numpy as np
import torch

from .._lib import call_model, ptr


def extract_surface(field, threshold):
    """(vertices [V, 3] float32 in grid-index units, faces [F, 3] int32) of the surface field == threshold.

    A grid point is inside when field >= threshold; a vertex sits on a grid edge (cube edge, face diagonal or body diagonal) whose
    ends differ, at t = (threshold - f0) / (f1 - f0); normals point toward decreasing values; the surface is closed wherever it does
    not reach the grid boundary.  Vertex and face order are fixed by the grid, so two calls return identical tensors."""
    if not (isinstance(field, torch.Tensor) and field.is_cuda and field.dtype == torch.float32 and field.dim() == 3 and
            field.shape[0] == field.shape[1] == field.shape[2]):
        raise ValueError("extract_surface needs an [R, R, R] float32 GPU tensor")
    R = int(field.shape[0])
    if R < 2 or 7 * R ** 3 > 2 ** 31 - 1:
        raise ValueError("extract_surface: resolution %d is outside 2 .. 674" % R)
    field = field.detach().contiguous()
    dev = field.device
    with torch.cuda.device(dev):
        edge_flag = torch.empty(R ** 3 * 7, dtype=torch.int32, device=dev)
        tri_count = torch.empty((R - 1) ** 3, dtype=torch.int32, device=dev)
        call_model(dev, "gip_surface_count", ptr(field), R, float(threshold), ptr(edge_flag), ptr(tri_count))
        edge_end = torch.cumsum(edge_flag, 0, dtype=torch.int32)
        tri_end = torch.cumsum(tri_count, 0, dtype=torch.int32)
        V, F = (int(n) for n in torch.stack((edge_end[-1], tri_end[-1])).cpu())      # the host read that sizes the outputs
        vertices = torch.empty((V, 3), dtype=torch.float32, device=dev)
        faces = torch.empty((F, 3), dtype=torch.int32, device=dev)
        if V == 0 or F == 0:
            return vertices, faces
        edge_index, tri_offset = edge_end - edge_flag, tri_end - tri_count           # exclusive scans
        call_model(dev, "gip_surface_emit", ptr(field), R, float(threshold), ptr(edge_flag), ptr(edge_index), ptr(tri_offset), ptr(vertices),
                   ptr(faces))
    return vertices, faces


# ---------------------------------------------------------------------------------------------------------------- clean, decimate
_CC_BATCH = 4             # rounds of hook + compress between two reads of the `changed` flag
MAX_GRID = 2048
MAX_CLUSTER_VERTICES = 2 ** 21 - 1      # three ids are packed into one 63-bit sort key
PLACE_LANES = 16          # lanes per cell of the placement kernel (DESIGN.md "Cleaning and decimating the mesh" has the measurement)


def _mesh_args(what, vertices, faces):
    """The argument checks of the functions below, made before the library is touched; (vertices or None, faces), contiguous."""
    if vertices is not None and not (isinstance(vertices, torch.Tensor) and vertices.is_cuda and vertices.dtype == torch.float32 and
                                     vertices.dim() == 2 and vertices.shape[1] == 3):
        raise ValueError("%s needs a [V, 3] float32 GPU tensor of vertices" % what)
    if not (isinstance(faces, torch.Tensor) and faces.is_cuda and faces.dtype == torch.int32 and faces.dim() == 2 and faces.shape[1] == 3):
        raise ValueError("%s needs an [F, 3] int32 GPU tensor of faces" % what)
    if vertices is not None and vertices.device != faces.device:
        raise ValueError("%s: vertices and faces must be on one device" % what)
    if int(faces.shape[0]) > (2 ** 31 - 1) // 3 or (vertices is not None and int(vertices.shape[0]) > 2 ** 31 - 1):
        raise ValueError("%s: at most 2^31 - 1 vertices and face corners" % what)
    return (None if vertices is None else vertices.detach().contiguous()), faces.detach().contiguous()


def settle_labels(step, limit, batch, what):
    """The host loop of a label propagation (csrc/mesh_common.h "Labels"): step() launches `batch` rounds and returns the `changed` flag
    tensor, which the caller creates as 0 and the loop zeroes again before every further call.  Returns once a call changed nothing;
    RuntimeError("<what> did not settle in %d rounds") after more than limit + 1 + batch rounds (whole batches, and the batch that
    confirms), which cannot happen for `limit` items because labels only decrease."""
    rounds = 0
    while True:
        changed = step()
        rounds += batch
        if int(changed.item()) == 0:
            return
        if rounds > limit + 1 + batch:
            raise RuntimeError("%s did not settle in %d rounds" % (what, rounds))
        changed.zero_()


def _compact(keep, rank, count, values):
    """The rows of `values` where `keep`, in order, given rank = cumsum(keep) - 1 and their number: a scatter into count + 1 rows (the
    last one takes the dropped rows and is cut off), so no host read beyond the one that gave `count`."""
    out = values.new_empty((count + 1,) + tuple(values.shape[1:]))
    out.index_copy_(0, torch.where(keep, rank, torch.full_like(rank, count)), values)
    return out[:count]


def connected_components(faces, num_vertices):
    """labels [V] int32: labels[v] is the smallest vertex index of v's connected component.  Two vertices are connected when a face
    names both (so components that touch at one vertex are one component, and a face with a repeated index connects what it names); a
    vertex that no face names is its own component; a face with an index outside [0, V) is ignored.  The result depends on nothing
    but `faces`.  Rounds of a hook and a compress kernel (csrc/mesh_clean.hip; csrc/mesh_common.h says why the fixed point is the
    minimum) until one changes nothing; the flag is read once every %d rounds.  RuntimeError if that takes more than V + 1 rounds (whole
    batches, and the batch that confirms): it cannot, because labels only decrease."""
    _, faces = _mesh_args("connected_components", None, faces)
    V, F = int(num_vertices), int(faces.shape[0])
    if V < 0 or V > 2 ** 31 - 1:
        raise ValueError("connected_components: num_vertices must lie in 0 .. 2^31 - 1")
    dev = faces.device
    labels = torch.arange(V, dtype=torch.int32, device=dev)
    if F == 0 or V == 0:
        return labels
    changed = torch.zeros(1, dtype=torch.int32, device=dev)

    def rounds():
        call_model(dev, "gip_mesh_components_rounds", ptr(faces), F, V, ptr(labels), ptr(changed), _CC_BATCH)
        return changed
    settle_labels(rounds, V, _CC_BATCH, "connected_components")
    return labels


connected_components.__doc__ %= _CC_BATCH


def _sq_diagonal(d):
    return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]      # float32, left to right


def clean_mesh(vertices, faces, min_faces=8, min_diameter=0.05, keep_largest=False, validate=True):
    """(vertices, faces, info): the mesh without its floaters, in place of kiui's clean_mesh (gs_renderer.py:346-349; its defaults
    min_f = 8, min_d = 5 percent are the defaults here); remeshing is not part of it.

    A component (connected_components) is kept when it has at least `min_faces` faces and the squared diagonal of its bounding box,
    dx dx + dy dy + dz dz in float32, is at least (min_diameter * D)^2 (float32: min_diameter times the square root of the squared
    diagonal, squared), D the diagonal of the box of all referenced vertices.  keep_largest=True keeps only the kept component with the most
    faces, the lowest label on a tie.  The output faces are the input faces of kept components in input order, re-indexed; the output
    vertices the referenced vertices of kept components in input order: two calls return identical tensors.
    info: "labels" [V_in] int32, "vertex_map" [V_in] int32 (the new index, -1 for a dropped vertex), "face_map" [F_out] int32 (the input
    face), "num_components" (components with at least one face) and "num_kept".
    validate: one host read checks that every index lies in [0, V) (ValueError otherwise); the kernels skip such a face regardless,
    and it is dropped.  F == 0 returns empty tensors without a launch.  One host read sizes the outputs."""
    vertices, faces = _mesh_args("clean_mesh", vertices, faces)
    if int(min_faces) < 0 or not float(min_diameter) >= 0:
        raise ValueError("clean_mesh: min_faces and min_diameter must not be negative")
    V, F = int(vertices.shape[0]), int(faces.shape[0])
    dev = vertices.device
    if F == 0:
        return vertices.new_empty((0, 3)), faces.new_empty((0, 3)), dict(
            labels=torch.arange(V, dtype=torch.int32, device=dev), vertex_map=torch.full((V,), -1, dtype=torch.int32, device=dev),
            face_map=torch.empty(0, dtype=torch.int32, device=dev), num_components=0, num_kept=0)
    if validate:
        lo, hi = (int(x) for x in torch.stack((faces.min(), faces.max())).cpu())
        if lo < 0 or hi >= V:
            raise ValueError("clean_mesh: face indices must lie in [0, %d)" % V)
    if V == 0:
        return clean_mesh(vertices, faces[:0], min_faces, min_diameter, keep_largest, False)
    labels = connected_components(faces, V)
    count = torch.empty(V, dtype=torch.int32, device=dev)
    box = torch.empty((V, 6), dtype=torch.float32, device=dev)
    call_model(dev, "gip_mesh_component_stats", ptr(vertices), ptr(faces), F, V, ptr(labels), ptr(count), ptr(box))
    has = count > 0
    inf = torch.full_like(box[:, :3], float("inf"))
    mn, mx = torch.where(has[:, None], box[:, :3], inf), torch.where(has[:, None], box[:, 3:], -inf)
    d2 = _sq_diagonal(torch.where(has[:, None], mx - mn, torch.zeros_like(mn)))
    whole = torch.sqrt(_sq_diagonal(mx.amax(0) - mn.amin(0)))
    bar = torch.tensor(float(min_diameter), dtype=torch.float32, device=dev) * whole
    keep = has & (count >= int(min_faces)) & (d2 >= bar * bar)
    ids = torch.arange(V, dtype=torch.int64, device=dev)
    if keep_largest:
        size = torch.where(keep, count, torch.full_like(count, -1))
        first = torch.where(size == size.max(), ids, torch.full_like(ids, V)).amin()
        keep = keep & (ids == first)
    fl = faces.long()
    valid = ((fl >= 0) & (fl < V)).all(1)
    face_keep = valid & keep[labels.long()[fl[:, 0].clamp(0, V - 1)]]
    used = torch.zeros(V, dtype=torch.int32, device=dev).index_add_(0, fl.clamp(0, V - 1).reshape(-1),
                                                                     face_keep.repeat_interleave(3).to(torch.int32)) > 0
    vrank, frank = torch.cumsum(used, 0) - 1, torch.cumsum(face_keep, 0) - 1
    V_out, F_out, found, kept = (int(x) for x in torch.stack((vrank[-1] + 1, frank[-1] + 1, has.sum(), keep.sum())).cpu())      # the host read
    vertex_map = torch.where(used, vrank, torch.full_like(vrank, -1)).to(torch.int32)
    out_faces = _compact(face_keep, frank, F_out, vertex_map[fl.clamp(0, V - 1)])
    face_map = _compact(face_keep, frank, F_out, torch.arange(F, dtype=torch.int32, device=dev))
    return _compact(used, vrank, V_out, vertices), out_faces, dict(labels=labels, vertex_map=vertex_map, face_map=face_map,
                                                                  num_components=found, num_kept=kept)


def _grid_arg(what, grid):
    if isinstance(grid, bool) or int(grid) != grid or not 1 <= int(grid) <= MAX_GRID:
        raise ValueError("%s: grid must be an integer in 1 .. %d" % (what, MAX_GRID))
    return int(grid)


def _grid_frame(what, vertices):
    """(lo [3] float32 numpy, L float32): the per-axis minimum and the largest axis extent of the vertices; one host read."""
    lo = vertices.amin(0)
    frame = torch.cat((lo, (vertices.amax(0) - lo).amax().reshape(1))).cpu().numpy()
    if not frame[3] > 0 or not np.isfinite(frame).all():
        raise ValueError("%s: the vertices have no extent (or are not finite)" % what)
    return frame[:3], frame[3]


def _cell_size(L, n):
    return float(np.float32(L) / np.float32(n))      # float32 on the host: what the kernels and the restatement are given


def cluster_face_count(vertices, faces, grid, frame=None):
    """The faces whose three corners fall in three different cells of cluster_decimate's grid: what decimate_mesh bisects on (before the
    removal of duplicates, so an upper bound of cluster_decimate's face count).  One kernel and one host read."""
    vertices, faces = _mesh_args("cluster_face_count", vertices, faces)
    n = _grid_arg("cluster_face_count", grid)
    if int(faces.shape[0]) == 0:
        return 0
    lo, L = _grid_frame("cluster_face_count", vertices) if frame is None else frame
    dev = vertices.device
    count = torch.empty(1, dtype=torch.int32, device=dev)
    call_model(dev, "gip_mesh_cluster_count", ptr(vertices), int(vertices.shape[0]), ptr(faces), int(faces.shape[0]), float(lo[0]),
               float(lo[1]), float(lo[2]), _cell_size(L, n), n, ptr(count))
    return int(count.item())


def _cluster_runs(vertices, faces, n):
    """What the placement kernel walks: the occupied cells' keys in ascending order, every vertex's cell id, and the face corners and
    the vertices stably sorted by cell with the cells' offsets (csrc/mesh_clean.hip mc_place_kernel)."""
    V, dev = int(vertices.shape[0]), vertices.device
    lo, L = _grid_frame("cluster_decimate", vertices)
    frame = (float(lo[0]), float(lo[1]), float(lo[2]), _cell_size(L, n), n)
    keys = torch.empty(V, dtype=torch.int64, device=dev)
    call_model(dev, "gip_mesh_cluster_keys", ptr(vertices), V, *frame, ptr(keys))
    cell_key, cell_of = torch.unique(keys, sorted=True, return_inverse=True)      # the host read for the count is in here
    C = int(cell_key.shape[0])
    fl = faces.long()
    valid = ((fl >= 0) & (fl < V)).all(1)
    nf = cell_of[fl.clamp(0, V - 1)]                                               # [F, 3] int64: the corners' cells
    ends = lambda ids: torch.cat((ids.new_zeros(1), torch.bincount(ids, minlength=C).cumsum(0))).to(torch.int32)  # noqa: E731
    corner_cell = nf.reshape(-1)
    return dict(frame=frame, cell_key=cell_key, cell_of=cell_of, valid=valid, corner_cell_of=nf, corner_cell=corner_cell,
                corner_order=torch.sort(corner_cell, stable=True).indices.to(torch.int32), corner_start=ends(corner_cell),
                member_order=torch.sort(cell_of, stable=True).indices.to(torch.int32), member_start=ends(cell_of))


def _cluster_place(vertices, faces, runs, lanes):
    """[C, 3]: one launch of gip_mesh_cluster_place on the runs of _cluster_runs."""
    dev, C = vertices.device, int(runs["cell_key"].shape[0])
    placed = torch.empty((C, 3), dtype=torch.float32, device=dev)
    call_model(dev, "gip_mesh_cluster_place", ptr(vertices), int(vertices.shape[0]), ptr(faces), int(faces.shape[0]), ptr(runs["cell_key"]), C,
               ptr(runs["corner_order"]), ptr(runs["corner_start"]), ptr(runs["member_order"]), ptr(runs["member_start"]), *runs["frame"], lanes,
               ptr(placed))
    return placed


def cluster_decimate(vertices, faces, grid, lanes=None):
    """(vertices [C, 3], faces [F', 3] int32, vertex_map [V_in] int32): the mesh decimated by vertex clustering with quadric placement
    (Lindstrom 2000; DeCoro and Tatarchuk 2007), the GPU form of the error metric of the edge-collapse simplification the reference
    gets from a third party (gs_renderer.py:350).

    grid = n in 1 .. 2048 cells along the longest axis: lo = the per-axis minimum of the vertices, L the largest extent, h = L / n, cell
    index i = min((int) floor((p - lo) / h), n - 1) per axis in float32, key (iz n + iy) n + ix.  Every occupied cell becomes one vertex
    (ids = the ranks of the keys in ascending order), placed where the quadrics of the faces with a corner in the cell are smallest,
    regularised toward the mean of the cell's vertices and clamped to the cell (csrc/mesh_clean.hip states the arithmetic).  Faces are
    remapped; one with two equal corners is dropped; of faces with the same unordered corner set the lowest input index survives;
    survivors keep the input order.  A cell that no surviving face names is removed: the output vertices are exactly the referenced
    ones, in key order, and vertex_map is -1 for the vertices of removed cells.  At most 2^21 - 1 occupied cells (ValueError beyond;
    three ids share a 63-bit sort key).  No float atomics: two calls return bit-identical tensors.  `lanes` (16, 32 or 64; default %d)
    is the placement kernel's lanes per cell; it changes the last bits only.
    Clustering is not an edge collapse: it does not preserve manifoldness or orientation where the surface is thinner than a cell (two
    sheets in one cell merge; a sliver may flip), and it can join parts that were apart.  ValueError when the vertices have no extent."""
    vertices, faces = _mesh_args("cluster_decimate", vertices, faces)
    n = _grid_arg("cluster_decimate", grid)
    lanes = PLACE_LANES if lanes is None else int(lanes)
    if lanes not in (16, 32, 64):
        raise ValueError("cluster_decimate: lanes must be 16, 32 or 64")
    V, F = int(vertices.shape[0]), int(faces.shape[0])
    dev = vertices.device
    if V == 0:
        return vertices.new_empty((0, 3)), faces.new_empty((0, 3)), torch.empty(0, dtype=torch.int32, device=dev)
    runs = _cluster_runs(vertices, faces, n)
    cell_of, nf, corner_cell = runs["cell_of"], runs["corner_cell_of"], runs["corner_cell"]
    C = int(runs["cell_key"].shape[0])
    if C > MAX_CLUSTER_VERTICES:
        raise ValueError("cluster_decimate: %d occupied cells; at most %d" % (C, MAX_CLUSTER_VERTICES))
    placed = _cluster_place(vertices, faces, runs, lanes)
    valid = runs["valid"]
    # faces: drop the collapsed ones, then all but the first of every unordered corner set
    alive = valid & (nf[:, 0] != nf[:, 1]) & (nf[:, 1] != nf[:, 2]) & (nf[:, 0] != nf[:, 2])
    s = torch.sort(nf, dim=1).values
    packed = torch.where(alive, (s[:, 0] << 42) | (s[:, 1] << 21) | s[:, 2], torch.full_like(s[:, 0], 2 ** 63 - 1))
    ks, order = torch.sort(packed, stable=True)                                    # stable: a run starts with its lowest input index
    first = torch.ones_like(ks, dtype=torch.bool)
    first[1:] = ks[1:] != ks[:-1]
    keep = torch.zeros(F, dtype=torch.bool, device=dev)
    keep[order] = first & (ks != 2 ** 63 - 1)
    used = torch.zeros(C, dtype=torch.int32, device=dev).index_add_(0, corner_cell, keep.repeat_interleave(3).to(torch.int32)) > 0
    vrank, frank = torch.cumsum(used, 0) - 1, torch.cumsum(keep, 0) - 1
    if F:
        C_out, F_out = (int(x) for x in torch.stack((vrank[-1] + 1, frank[-1] + 1)).cpu())      # the host read that sizes the outputs
    else:
        C_out, F_out = 0, 0
    new_id = torch.where(used, vrank, torch.full_like(vrank, -1)).to(torch.int32)
    return _compact(used, vrank, C_out, placed), _compact(keep, frank, F_out, new_id[nf]), new_id[cell_of]


cluster_decimate.__doc__ %= PLACE_LANES


def decimate_mesh(vertices, faces, target_faces):
    """(vertices, faces, vertex_map, grid): cluster_decimate at the finest grid whose count of faces with three corners in three cells
    (cluster_face_count) is at most `target_faces`, in place of kiui's decimate_mesh (gs_renderer.py:350, decimate_target = 1e5).  The
    removal of duplicates can only lower the count, so the result has at most target_faces faces.  A bisection over n in [1, 2048] with
    the invariant count(lo) <= target < count(hi): one probe at 2048 (the answer when it fits), then at most 11, each one kernel and
    one host read.  F <= target_faces returns the inputs unchanged with vertex_map = 0 .. V - 1 and grid = 0.  cluster_decimate's
    limits hold: clustering does not preserve manifoldness or orientation in parts thinner than a cell."""
    given = (vertices, faces)
    vertices, faces = _mesh_args("decimate_mesh", vertices, faces)
    if not target_faces >= 1:
        raise ValueError("decimate_mesh: target_faces must be at least 1")
    target = int(target_faces)
    if int(faces.shape[0]) <= target:
        return given[0], given[1], torch.arange(int(vertices.shape[0]), dtype=torch.int32, device=vertices.device), 0
    frame = _grid_frame("decimate_mesh", vertices)
    lo, hi = 1, MAX_GRID                                   # count(1) == 0: every vertex shares the one cell
    if cluster_face_count(vertices, faces, hi, frame) <= target:
        lo = hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if cluster_face_count(vertices, faces, mid, frame) <= target:
            lo = mid
        else:
            hi = mid
    return cluster_decimate(vertices, faces, lo) + (lo,)


def _array(t, dtype):
    return np.asarray(t.detach().cpu() if isinstance(t, torch.Tensor) else t, dtype=dtype)


def write_obj(path, vertices, faces, colors=None, normals=None):
    """Wavefront OBJ: `v x y z` lines (9 significant digits: a float32 survives the round trip), `f a b c` lines, 1-based.  With
    `colors` ([V, 3] in [0, 1]) the vertex lines become `v x y z r g b` (the common vertex-colour extension); with `normals` ([V, 3])
    the file gains one `vn` line per vertex and the faces are written `f a//a b//b c//c`."""
    v = _array(vertices, np.float32)
    f = _array(faces, np.int64) + 1
    col = None if colors is None else _array(colors, np.float32).reshape(-1, 3)
    nrm = None if normals is None else _array(normals, np.float32).reshape(-1, 3)
    if (col is not None and col.shape[0] != v.shape[0]) or (nrm is not None and nrm.shape[0] != v.shape[0]):
        raise ValueError("write_obj: colors and normals need one row per vertex")
    with open(path, "w") as out:
        out.write("# %d vertices, %d faces\n" % (v.shape[0], f.shape[0]))
        if col is None:
            out.write("".join("v %.9g %.9g %.9g\n" % (float(a), float(b), float(c)) for a, b, c in v))
        else:
            out.write("".join("v %.9g %.9g %.9g %.9g %.9g %.9g\n" % tuple(float(x) for x in row) for row in np.concatenate((v, col), 1)))
        if nrm is None:
            out.write("".join("f %d %d %d\n" % (a, b, c) for a, b, c in f))
        else:
            out.write("".join("vn %.9g %.9g %.9g\n" % (float(a), float(b), float(c)) for a, b, c in nrm))
            out.write("".join("f %d//%d %d//%d %d//%d\n" % (a, a, b, b, c, c) for a, b, c in f))


def read_obj_full(path):
    """(vertices [V, 3] float32, faces [F, 3] int32 0-based, colors [V, 3] float32 or None, normals [V, 3] float32 or None) of an OBJ
    that write_obj wrote: colours are the fourth to sixth number of the `v` lines, normals the `vn` lines."""
    v, f, c, n = [], [], [], []
    with open(path) as src:
        for line in src:
            parts = line.split()
            if not parts:
                continue
            if parts[0] == "v":
                v.append([float(x) for x in parts[1:4]])
                if len(parts) >= 7:
                    c.append([float(x) for x in parts[4:7]])
            elif parts[0] == "vn":
                n.append([float(x) for x in parts[1:4]])
            elif parts[0] == "f":
                f.append([int(x.split("/")[0]) - 1 for x in parts[1:4]])
    if c and len(c) != len(v):
        raise ValueError("%s: some vertices carry a colour and some do not" % path)
    return (np.asarray(v, np.float32).reshape(-1, 3), np.asarray(f, np.int32).reshape(-1, 3),
            np.asarray(c, np.float32).reshape(-1, 3) if c else None, np.asarray(n, np.float32).reshape(-1, 3) if n else None)


def read_obj(path):
    """(vertices [V, 3] float32, faces [F, 3] int32, 0-based) of an OBJ that write_obj wrote; colours and normals, if the file has
    them, are left to read_obj_full."""
    return read_obj_full(path)[:2]


def write_ply_mesh(path, vertices, faces, colors=None, normals=None):
    """Binary little-endian PLY: vertex x y z float32, then nx ny nz float32 (with `normals`), then red green blue uchar (with
    `colors`, rounded from [0, 1]); face `list uchar int vertex_indices`.  The layout MeshLab and Blender read vertex colours from."""
    v = _array(vertices, np.float32).reshape(-1, 3)
    f = _array(faces, np.int32).reshape(-1, 3)
    fields, props = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")], ["property float x", "property float y", "property float z"]
    if normals is not None:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
        props += ["property float nx", "property float ny", "property float nz"]
    if colors is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        props += ["property uchar red", "property uchar green", "property uchar blue"]
    table = np.zeros(v.shape[0], dtype=fields)
    cols = [("x", "y", "z", v)]
    if normals is not None:
        cols.append(("nx", "ny", "nz", _array(normals, np.float32).reshape(-1, 3)))
    if colors is not None:
        cols.append(("red", "green", "blue", np.rint(np.clip(_array(colors, np.float64).reshape(-1, 3), 0, 1) * 255).astype(np.uint8)))
    for a, b, c, src in cols:
        if src.shape[0] != v.shape[0]:
            raise ValueError("write_ply_mesh: colors and normals need one row per vertex")
        table[a], table[b], table[c] = src[:, 0], src[:, 1], src[:, 2]
    tris = np.zeros(f.shape[0], dtype=[("n", "u1"), ("idx", "<i4", (3,))])
    tris["n"], tris["idx"] = 3, f
    header = ["ply", "format binary_little_endian 1.0", "element vertex %d" % v.shape[0]] + props + \
             ["element face %d" % f.shape[0], "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as out:
        out.write(("\n".join(header) + "\n").encode("ascii"))
        out.write(table.tobytes())
        out.write(tris.tobytes())


_PLY_TYPES = {"float": "<f4", "float32": "<f4", "uchar": "u1", "uint8": "u1", "int": "<i4", "int32": "<i4"}


def read_ply_mesh(path):
    """(vertices [V, 3] float32, faces [F, 3] int32, colors [V, 3] float32 in [0, 1] or None, normals [V, 3] float32 or None) of a
    PLY that write_ply_mesh wrote (binary little-endian, triangles only)."""
    with open(path, "rb") as src:
        if src.readline().strip() != b"ply":
            raise ValueError("%s is not a PLY file" % path)
        fmt, element, counts, vprops, fprop = None, None, {}, [], None
        while True:
            line = src.readline()
            if not line:
                raise ValueError("%s: no end_header" % path)
            parts = line.decode("ascii").split()
            if not parts or parts[0] == "comment":
                continue
            if parts[0] == "format":
                fmt = parts[1]
            elif parts[0] == "element":
                element = parts[1]
                counts[element] = int(parts[2])
            elif parts[0] == "property" and element == "vertex":
                vprops.append((parts[2], _PLY_TYPES[parts[1]]))
            elif parts[0] == "property" and element == "face":
                fprop = parts[1:]
            elif parts[0] == "end_header":
                break
        if fmt != "binary_little_endian":
            raise ValueError("unsupported PLY format %r" % fmt)
        if counts.get("face", 0) and (fprop is None or fprop[0] != "list" or _PLY_TYPES[fprop[1]] != "u1" or _PLY_TYPES[fprop[2]] != "<i4"):
            raise ValueError("%s: faces must be `list uchar int`" % path)
        nv, nf = counts.get("vertex", 0), counts.get("face", 0)
        vdt = np.dtype(vprops)
        table = np.frombuffer(src.read(nv * vdt.itemsize), dtype=vdt, count=nv)
        fdt = np.dtype([("n", "u1"), ("idx", "<i4", (3,))])
        tris = np.frombuffer(src.read(nf * fdt.itemsize), dtype=fdt, count=nf)
    if nf and (tris["n"] != 3).any():
        raise ValueError("%s: only triangles are supported" % path)
    names = set(vdt.names)
    pick = lambda keys: np.stack([table[k] for k in keys], 1)  # noqa: E731
    vertices = pick(("x", "y", "z")).astype(np.float32).reshape(-1, 3)
    normals = pick(("nx", "ny", "nz")).astype(np.float32).reshape(-1, 3) if {"nx", "ny", "nz"} <= names else None
    colors = (pick(("red", "green", "blue")).astype(np.float32) / 255).reshape(-1, 3) if {"red", "green", "blue"} <= names else None
    return vertices, tris["idx"].astype(np.int32).reshape(-1, 3), colors, normals


def write_obj_textured(path, vertices, faces, uv, texture, normals=None, uv_idx=None):
    """Wavefront OBJ with a material and a texture, the layout of the reference's exporter (threestudio/utils/saving.py:519-545):
    `path` = dir/name.obj gets `mtllib name.mtl`, `g object`, `usemtl default`, the `v` lines, `vn` lines (with `normals`, one per
    vertex) and `vt u v` lines (uv [F, 3, 2]: three per face, none shared; numbers with 9 significant digits as write_obj), then
    `f a/t/a b/t/b c/t/c` (`f a/t b/t c/t` without normals) with t = 3 f + 1 .. 3 f + 3.  dir/name.mtl holds the reference's
    statements in its order and names dir/name_kd.png, the texture ([H, W, 3] in [0, 1], row 0 on top) as an 8-bit PNG.  The
    reference calls every texture `texture_kd.*`; here the name follows the OBJ's, because two exports into one directory would
    otherwise overwrite each other's texture.
    uv_idx [F, 3] (a chart atlas' t_tex_idx): uv is then [Vt, 2], one `vt` line per texture vertex, and a face's corners name
    t = uv_idx + 1, so faces share their texture vertices."""
    import os

    from .texture import write_png_rgb
    v = _array(vertices, np.float32).reshape(-1, 3)
    f = _array(faces, np.int64).reshape(-1, 3) + 1
    vt = _array(uv, np.float32).reshape(-1, 2)
    nrm = None if normals is None else _array(normals, np.float32).reshape(-1, 3)
    if uv_idx is None:
        if vt.shape[0] != 3 * f.shape[0]:
            raise ValueError("write_obj_textured: uv needs three rows per face")
        ft = np.arange(1, 3 * f.shape[0] + 1, dtype=np.int64).reshape(-1, 3)
    else:
        ft = _array(uv_idx, np.int64).reshape(-1, 3) + 1
        if ft.shape[0] != f.shape[0] or (ft.size and (ft.min() < 1 or ft.max() > vt.shape[0])):
            raise ValueError("write_obj_textured: uv_idx needs one row per face with indices into uv")
    if nrm is not None and nrm.shape[0] != v.shape[0]:
        raise ValueError("write_obj_textured: normals need one row per vertex")
    stem = os.path.splitext(os.path.abspath(path))[0]
    name = os.path.basename(stem)
    with open(path, "w") as out:
        out.write("mtllib %s.mtl\ng object\nusemtl default\n" % name)
        out.write("".join("v %.9g %.9g %.9g\n" % (float(a), float(b), float(c)) for a, b, c in v))
        if nrm is not None:
            out.write("".join("vn %.9g %.9g %.9g\n" % (float(a), float(b), float(c)) for a, b, c in nrm))
        out.write("".join("vt %.9g %.9g\n" % (float(a), float(b)) for a, b in vt))
        if nrm is None:
            out.write("".join("f %d/%d %d/%d %d/%d\n" % (a, ta, b, tb, c, tc) for (a, b, c), (ta, tb, tc) in zip(f, ft)))
        else:
            out.write("".join("f %d/%d/%d %d/%d/%d %d/%d/%d\n" % (a, ta, a, b, tb, b, c, tc, c) for (a, b, c), (ta, tb, tc) in zip(f, ft)))
    with open(stem + ".mtl", "w") as out:
        out.write("newmtl default\nKa 0.0 0.0 0.0\nmap_Kd %s_kd.png\nKs 0.0 0.0 0.0\n" % name)
    write_png_rgb(stem + "_kd.png", texture)


def read_obj_textured(path, return_index=False):
    """(vertices [V, 3] float32, faces [F, 3] int32 0-based, normals [V, 3] float32 or None, uv [F, 3, 2] float32, texture [H, W, 3]
    float32 in [0, 1]) of what write_obj_textured wrote: the texture is the `map_Kd` of the file that `mtllib` names.
    return_index=True appends (v_tex [Vt, 2] float32, t_tex_idx [F, 3] int32): the `vt` lines and the faces' indices into them."""
    import os

    from .texture import read_png_rgb
    v, n, vt, f, ft, mtl = [], [], [], [], [], None
    with open(path) as src:
        for line in src:
            parts = line.split()
            if not parts:
                continue
            if parts[0] == "mtllib":
                mtl = parts[1]
            elif parts[0] == "v":
                v.append([float(x) for x in parts[1:4]])
            elif parts[0] == "vn":
                n.append([float(x) for x in parts[1:4]])
            elif parts[0] == "vt":
                vt.append([float(x) for x in parts[1:3]])
            elif parts[0] == "f":
                f.append([int(x.split("/")[0]) - 1 for x in parts[1:4]])
                ft.append([int(x.split("/")[1]) - 1 for x in parts[1:4]])
    if mtl is None:
        raise ValueError("%s names no material library" % path)
    folder, image = os.path.dirname(os.path.abspath(path)), None
    with open(os.path.join(folder, mtl)) as src:
        for line in src:
            parts = line.split()
            if parts and parts[0] == "map_Kd":
                image = parts[1]
    if image is None:
        raise ValueError("%s has no map_Kd" % mtl)
    uv = np.asarray(vt, np.float32).reshape(-1, 2)[np.asarray(ft, np.int64).reshape(-1, 3)]
    texture = read_png_rgb(os.path.join(folder, image)).astype(np.float32) / 255
    out = (np.asarray(v, np.float32).reshape(-1, 3), np.asarray(f, np.int32).reshape(-1, 3),
           np.asarray(n, np.float32).reshape(-1, 3) if n else None, uv.reshape(-1, 3, 2), texture)
    if return_index:
        out += (np.asarray(vt, np.float32).reshape(-1, 2), np.asarray(ft, np.int32).reshape(-1, 3))
    return out
