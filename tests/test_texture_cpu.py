"""Texture baking without a GPU: the C-ABI's declarations, bindings, exports and host-side argument checks (csrc/texture.hip,
include/gip_model.h), the atlas of gaussianip_amd/utils/texture.py against its restatement (tests/texture_reference.py), and the
PNG / textured OBJ writers and readers."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import sample_inputs
import texture_inputs
import texture_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = texture_inputs.layout_cases()


# ---------------------------------------------------------------------------------------------------------------- C-ABI
def test_symbols_declared_bound_and_exported():
    from gaussianip_amd import _lib
    header = open(os.path.join(ROOT, "include", "gip_model.h")).read()
    assert _lib.TEXTURE_SYMBOLS == ["gip_texture_bake_workspace_size", "gip_texture_bake"]
    lib = ctypes.CDLL(os.path.join(_lib.LIB_DIR, "libgip_model.so"))
    for sym in _lib.TEXTURE_SYMBOLS:
        assert re.search(r"\bint %s\(" % sym, header), sym
        getattr(lib, sym)
    bound = _lib.model_lib()
    for P, R, nb in ((1000, 128, 16), (0, 24, 4), (123457, 64, 8)):
        need, sample_need = ctypes.c_size_t(0), ctypes.c_size_t(1)
        assert bound.gip_texture_bake_workspace_size(P, R, nb, ctypes.byref(need)) == 0
        assert bound.gip_field_sample_workspace_size(P, R, nb, ctypes.byref(sample_need)) == 0 and need.value == sample_need.value
    need = ctypes.c_size_t(0)
    assert bound.gip_texture_bake_workspace_size(1000, 30, 16, ctypes.byref(need)) == 1     # num_blocks does not divide the resolution
    assert bound.gip_texture_bake_workspace_size(-1, 32, 8, ctypes.byref(need)) == 1
    assert bound.gip_texture_bake_workspace_size(10, 2048, 2048, ctypes.byref(need)) == 1   # more than 1024 blocks per axis
    assert bound.gip_texture_bake_workspace_size(10, 32, 8, None) == 1


def test_host_side_argument_checks_launch_nothing():
    from gaussianip_amd import _lib
    bound = _lib.model_lib()

    def call(P=5, R=32, nb=8, V=30, F=10, T=64, cell=8, slices=0, ws_bytes=0, ptr=None):
        """Every array NULL (or the non-NULL dummy `ptr`, which nothing may dereference)."""
        return bound.gip_texture_bake(ptr, ptr, ptr, ptr, ptr, P, ptr, 1.0, ptr, R, nb, 0.375, ptr, V, ptr, F, ptr, ptr, T, cell, slices,
                                      ptr, ws_bytes, ptr, ptr, None)
    assert call(F=0) == 0                                    # no faces: a successful no-op
    assert call(F=0, P=0, V=0) == 0
    assert call() == 1                                       # faces without their arrays
    assert call(R=30, nb=16, F=0) == 1                       # a shape outside the limits
    assert call(P=-1, F=0) == 1
    assert call(nb=2048, R=2048, F=0) == 1
    assert call(T=3, cell=3, F=0) == 1                       # T < 4
    assert call(T=16385, F=0) == 1                           # T > 16384
    assert call(cell=3, F=0) == 1                            # cell < 4
    assert call(T=64, cell=65, F=0) == 1                     # cell > T
    assert call(T=64, cell=8, F=129) == 1                    # 2 (T // cell)^2 = 128 < F
    assert call(T=64, cell=8, F=128) == 1                    # fits, but the arrays are NULL
    assert call(slices=-1, F=0) == 1
    assert call(F=2 ** 31) == 1 and call(V=2 ** 31, F=0) == 1 and call(F=-1) == 1 and call(V=-1, F=0) == 1
    dummy = ctypes.c_void_p(64)
    assert call(ptr=dummy, ws_bytes=5 * 48 - 1) == 1         # a short workspace, every pointer non-NULL: nothing is dereferenced
    assert call(ptr=dummy, V=0, ws_bytes=1 << 20) == 1       # faces without vertices


# ---------------------------------------------------------------------------------------------------------------- layout
@pytest.mark.parametrize("F,T", CASES)
def test_layout_ownership_and_uv(F, T):
    from gaussianip_amd.utils import texture as tex
    c, n, b = tex.atlas_layout(F, T)
    assert (c, n, b) == texture_reference.layout(F, T) and b == c - 3 and c >= 4 and 2 * n * n >= F
    assert c == T or 2 * (T // (c + 1)) ** 2 < F             # the largest such c
    own = tex.texel_owner(F, T)
    assert own.shape == (T, T) and np.array_equal(own, texture_reference.owner(F, T)[0])
    counts = np.bincount(own[own >= 0], minlength=F)         # a texel has one entry in `own`: no texel has two owners
    f = np.arange(F)
    assert np.array_equal(counts, np.where(f & 1, c * (c - 1) // 2, c * (c + 1) // 2))
    uv = tex.atlas_uv(F, T)
    assert uv.shape == (F, 3, 2) and uv.dtype == np.float32 and (uv > 0).all() and (uv < 1).all()
    assert np.array_equal(uv, texture_reference.uv(F, T))
    if F <= 1000:
        assert np.array_equal(texture_reference.corners(F, T), texture_reference.corners_fast(F, T))
    st = texture_reference.corners_fast(F, T)
    e1, e2 = st[:, 1] - st[:, 0], st[:, 2] - st[:, 0]
    area2 = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    assert (area2 == area2[0]).all() and abs(int(area2[0])) == b * b      # one orientation, the same for both halves
    # every texel under a bilinear footprint of a point of the face's UV triangle is the face's own: corners, edge midpoints and
    # 8 seeded interior points, as integer barycentric weights (w0, w1, w2) / D — exact integer arithmetic throughout
    rng = np.random.default_rng(F + T)
    D = 1 << 12
    w = [(D, 0, 0), (0, D, 0), (0, 0, D), (D // 2, D // 2, 0), (0, D // 2, D // 2), (D // 2, 0, D // 2)]
    for _ in range(8):
        a = int(rng.integers(1, D - 1))
        bb = int(rng.integers(1, D - a))
        w.append((D - a - bb, a, bb))
    w = np.array(w, np.int64)                                             # [14, 3], rows sum to D
    assert (w.sum(1) == D).all() and (w >= 0).all()
    num = np.einsum("pk,fkc->fpc", w, st)                                 # [F, 14, 2]: the point times D
    lo, frac = num // D, (num % D != 0).astype(np.int64)
    for dx in (0, 1):
        for dy in (0, 1):
            x = lo[..., 0] + dx * frac[..., 0]                            # with a zero fraction the second texel has weight 0
            y = lo[..., 1] + dy * frac[..., 1]
            assert (x >= 0).all() and (x < T).all() and (y >= 0).all() and (y < T).all()
            assert (own[y, x] == f[:, None]).all()


def test_layout_errors():
    from gaussianip_amd.utils import texture as tex
    assert tex.atlas_layout(131072, 1024) == (4, 256, 1)
    with pytest.raises(ValueError, match="1028"):            # the smallest size that works: 4 * 257
        tex.atlas_layout(131073, 1024)
    with pytest.raises(ValueError):
        tex.atlas_uv(33, 16)
    assert tex.atlas_layout(0, 64) == (64, 1, 61)
    # the sizes of the layout's table in DESIGN.md
    for F, T, c, share in ((180312, 2048, 6, 0.774), (180312, 4096, 13, 0.908), (736000, 4096, 6, 0.790)):
        assert tex.atlas_layout(F, T)[0] == c
        assert abs(float((tex.texel_owner(F, T) >= 0).mean()) - share) < 5e-4


def test_default_texture_size():
    from gaussianip_amd.scene import GaussianModel
    size = GaussianModel._default_texture_size
    assert size(0) == 64 and size(128) == 64 and size(129) == 128           # 2 * (64 // 8)^2 = 128
    assert size(180312) == 4096 and size(736000) == 8192                    # 8192: c = 13
    assert size(2 * (8192 // 4) ** 2) == 8192                               # c = 4: below 8, but the cap
    with pytest.raises(ValueError):
        size(2 * (8192 // 4) ** 2 + 1)


# ---------------------------------------------------------------------------------------------------------------- points
@pytest.mark.parametrize("F,T", [(1, 8), (7, 16), (50, 32), (1000, 128)])
def test_texel_points_match_the_restatement(F, T):
    from gaussianip_amd.utils import texture as tex
    v, f = texture_inputs.random_mesh(F, seed=F)
    want, wf, wx, wy = texture_reference.points(v, f, T, np.float32)
    got, gf, gx, gy = tex.texel_points(torch.from_numpy(v), torch.from_numpy(f), T)
    assert got.dtype == torch.float32 and np.array_equal(gf.numpy(), wf) and np.array_equal(gx.numpy(), wx) and np.array_equal(gy.numpy(), wy)
    assert np.array_equal(got.numpy().view(np.uint32), want.view(np.uint32))              # bit for bit
    own, li, lj = texture_reference.owner(F, T)
    li, lj = li[wy, wx], lj[wy, wx]
    _, _, b = texture_reference.layout(F, T)
    tri = v[f[wf]]                                                                         # [K, 3, 3]
    at0, at1, at2 = (li == 0) & (lj == 0), (li == b) & (lj == 0), (li == 0) & (lj == b)
    assert at0.sum() == F and at1.sum() == F and at2.sum() == F
    assert np.array_equal(got.numpy()[at0], tri[at0, 0])                                   # v0 exactly
    # v1 and v2: fl(v0 + fl(v - v0)) is off by at most half an ulp of the difference plus half an ulp of the sum; that is within
    # 1 ulp of v wherever the difference is no larger than v (where it is larger, its rounding alone can exceed an ulp of v)
    for at, k in ((at1, 1), (at2, 2)):
        v0, vk, p = tri[at, 0], tri[at, k], got.numpy()[at]
        err = np.abs(p.astype(np.float64) - vk.astype(np.float64))
        ulp = np.maximum(np.spacing(np.abs(vk)), np.spacing(np.abs(p))).astype(np.float64)
        assert (err <= 0.5 * np.spacing(np.abs(vk - v0)).astype(np.float64) + 0.5 * ulp).all()
        small = np.abs(vk - v0) <= np.abs(vk)
        assert small.sum() > small.size // 2 and (err[small] <= ulp[small]).all()


# ---------------------------------------------------------------------------------------------------------------- constant colour
def test_reference_bakes_a_constant_colour():
    cl, rgb = sample_inputs.sphere_cloud()
    world, faces = texture_inputs.sphere_mesh()
    vn = (world.astype(np.float64) * 1.8).astype(np.float32)                # sphere_cloud: center 0, scale 1.8
    T = 64
    density, color_sum, info = texture_reference.bake_sums(cl, rgb, 32, 4, vn, faces, T, np.float64)
    assert np.abs(info["center"]).max() <= 1e-7 and abs(info["scale"] - 1.8) <= 1e-6
    assert np.array_equal(info["owned"], texture_reference.owner(len(faces), T)[0] >= 0)
    assert (density[~info["owned"]] == 0).all() and (color_sum[~info["owned"]] == 0).all()
    lit = info["owned"] & (density > 0)
    assert lit.sum() > 0.9 * info["owned"].sum()
    color = color_sum[lit] / density[lit][:, None]
    assert np.abs(color - np.array(sample_inputs.SPHERE_COLOR, np.float32).astype(np.float64)).max() <= 1e-6


# ---------------------------------------------------------------------------------------------------------------- files
def test_png_round_trip(tmp_path):
    from gaussianip_amd.utils.texture import read_png_rgb, write_png_rgb
    img = np.random.default_rng(11).uniform(-0.1, 1.1, (37, 53, 3)).astype(np.float32)     # some values are clipped
    want = np.rint(np.clip(img.astype(np.float64), 0, 1) * 255).astype(np.uint8)
    path = str(tmp_path / "t.png")
    write_png_rgb(path, img)
    got = read_png_rgb(path)
    assert got.dtype == np.uint8 and got.shape == (37, 53, 3) and np.array_equal(got, want)
    write_png_rgb(path, torch.from_numpy(img))
    assert np.array_equal(read_png_rgb(path), want)
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        with Image.open(path) as im:
            assert im.mode == "RGB" and np.array_equal(np.asarray(im), want)
    with pytest.raises(ValueError):
        write_png_rgb(path, np.zeros((4, 4), np.float32))


V = np.array([[0, 0, 0], [1, 0.5, 0], [0, 1, 1 / 3], [-2.5e-7, 3, 1e10]], np.float32)
FACES = np.array([[0, 1, 2], [2, 1, 3]], np.int32)
N = np.array([[0, 0, 1], [0, -1, 0], [0.6, 0.8, 0], [0, 0, 0]], np.float32)


@pytest.mark.parametrize("with_normals", [True, False])
def test_textured_obj_round_trip(tmp_path, with_normals):
    from gaussianip_amd.utils import texture as tex
    from gaussianip_amd.utils.mesh import read_obj, read_obj_textured, write_obj_textured
    uv = tex.atlas_uv(2, 12)                                                # not a power of two: the numbers need their 9 digits
    image = np.random.default_rng(12).uniform(0, 1, (12, 12, 3)).astype(np.float32)
    path = str(tmp_path / "sub.dir" / "avatar.obj")
    os.makedirs(os.path.dirname(path))
    write_obj_textured(path, V, FACES, uv, image, normals=N if with_normals else None)
    assert sorted(os.listdir(os.path.dirname(path))) == ["avatar.mtl", "avatar.obj", "avatar_kd.png"]
    assert open(path[:-4] + ".mtl").read() == "newmtl default\nKa 0.0 0.0 0.0\nmap_Kd avatar_kd.png\nKs 0.0 0.0 0.0\n"
    lines = open(path).read().splitlines()
    assert lines[:3] == ["mtllib avatar.mtl", "g object", "usemtl default"]
    kinds = [ln.split()[0] for ln in lines[3:]]
    assert kinds == ["v"] * 4 + (["vn"] * 4 if with_normals else []) + ["vt"] * 6 + ["f"] * 2
    assert lines[-2:] == (["f 1/1/1 2/2/2 3/3/3", "f 3/4/3 2/5/2 4/6/4"] if with_normals else ["f 1/1 2/2 3/3", "f 3/4 2/5 4/6"])
    assert lines[3 + 3] == "v -2.49999999e-07 3 1e+10"
    rv, rf, rn, ruv, rtex = read_obj_textured(path)
    assert np.array_equal(rv, V) and np.array_equal(rf, FACES) and rf.dtype == np.int32
    assert np.array_equal(rn, N) if with_normals else rn is None
    assert ruv.shape == (2, 3, 2) and ruv.dtype == np.float32 and np.array_equal(ruv, uv)
    assert rtex.shape == (12, 12, 3) and rtex.dtype == np.float32 and np.abs(rtex - image).max() <= 0.5 / 255 + 1e-7
    pv, pf = read_obj(path)                                                 # the plain reader still reads such a file
    assert np.array_equal(pv, V) and np.array_equal(pf, FACES)
    with pytest.raises(ValueError):
        write_obj_textured(path, V, FACES, uv[:1], image)


def test_empty_textured_mesh_round_trips(tmp_path):
    from gaussianip_amd.utils.mesh import read_obj_textured, write_obj_textured
    e3, ei = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    path = str(tmp_path / "e.obj")
    write_obj_textured(path, e3, ei, np.zeros((0, 3, 2), np.float32), np.zeros((64, 64, 3), np.float32), normals=e3)
    rv, rf, rn, ruv, rtex = read_obj_textured(path)
    assert rv.shape == (0, 3) and rf.shape == (0, 3) and rn is None and ruv.shape == (0, 3, 2)
    assert rtex.shape == (64, 64, 3) and not rtex.any()


def test_bake_texture_argument_errors_without_a_gpu():
    from gaussianip_amd.scene import GaussianModel
    v, f = torch.zeros(4, 3), torch.zeros((2, 3), dtype=torch.int32)
    with pytest.raises(ValueError, match="divide"):
        GaussianModel(0, device="cpu").bake_texture(v, f, resolution=30, num_blocks=16)
    with pytest.raises(RuntimeError, match="GPU"):
        GaussianModel(0, device="cpu").bake_texture(v, f, resolution=32, num_blocks=8)
