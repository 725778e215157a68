"""Gaussian parameter store + Adam-state surgery + densify / prune, API-compatible with the reference.

Reference: gaussiansplatting/scene/gaussian_model.py — activations :15-30, fields :33-48, getters :84-107,
create_from_pcd :113-136, training_setup :138-159, lr schedule :161-181, PLY I/O :183-264, optimizer surgery
:266-355, densify_and_split :357-380, densify_and_clone :382-393, densify_and_prune :395-410, prune_only :413-418,
add_densification_stats :420-422.  Pinned by tests/golden/gaussian_model.npz (traces captured from the imported
reference class).

Differences that do not change results: tensors follow `device` (default "cuda") instead of a hard-coded "cuda";
the six parameter groups are handled through one table instead of six hand-written copies; PLY files are read and
written by a small built-in binary reader/writer (same header and column order as plyfile produces).
"""
import os

import numpy as np
import torch
from torch import nn

from ..utils.general import (build_rotation, build_scaling_rotation, get_expon_lr_func, inverse_sigmoid,
                             strip_symmetric)
from ..utils.graphics import BasicPointCloud
from ..utils.sh import RGB2SH

# optimizer group name -> attribute holding the parameter (order = the reference's param_groups order)
_GROUPS = (("xyz", "_xyz"), ("f_dc", "_features_dc"), ("f_rest", "_features_rest"), ("opacity", "_opacity"),
           ("scaling", "_scaling"), ("rotation", "_rotation"))


def _covariance_from_scaling_rotation(scaling, scaling_modifier, rotation):
    L = build_scaling_rotation(scaling_modifier * scaling, rotation)
    return strip_symmetric(L @ L.transpose(1, 2))


_FUSED_ACT = True     # False: the three getters' op chains (the same-box A/B of DESIGN §4d; tests flip the attribute)


class _Activate(torch.autograd.Function):
    """(sigmoid(opacity), exp(scaling), normalize(rotation)) in one launch, their backward in one (include/gip_model.h:
    gip_activate_gaussians*): the values of the getters :72-89, which stay what every other caller uses."""

    @staticmethod
    def forward(ctx, o, s, q):
        from .._lib import call_model, ptr
        oo, so, qo = torch.empty_like(o), torch.empty_like(s), torch.empty_like(q)
        call_model(o.device, "gip_activate_gaussians", ptr(o), ptr(s), ptr(q), o.shape[0], ptr(oo), ptr(so), ptr(qo))
        ctx.save_for_backward(oo, so, q)
        return oo, so, qo

    @staticmethod
    def backward(ctx, go, gs, gq):
        from .._lib import call_model, ptr
        oo, so, q = ctx.saved_tensors
        go, gs, gq = (None if g_ is None else g_.contiguous() for g_ in (go, gs, gq))
        need = ctx.needs_input_grad
        d_o = torch.empty_like(oo) if need[0] else None
        d_s = torch.empty_like(so) if need[1] else None
        d_q = torch.empty_like(q) if need[2] else None
        call_model(oo.device, "gip_activate_gaussians_backward", ptr(oo), ptr(so), ptr(q), ptr(go), ptr(gs), ptr(gq), oo.shape[0],
                   ptr(d_o), ptr(d_s), ptr(d_q))
        return d_o, d_s, d_q


class GaussianModel:
    def get_activated(self):
        """(get_opacity, get_scaling, get_rotation) of one step — on the GPU with the stock activations one launch forward and
        one backward instead of the three getters' op chains."""
        o, s, q = self._opacity, self._scaling, self._rotation
        if (_FUSED_ACT and o.is_cuda and self.opacity_activation is torch.sigmoid and self.scaling_activation is torch.exp and
                self.rotation_activation is torch.nn.functional.normalize and
                all(t.dtype == torch.float32 and t.is_contiguous() for t in (o, s, q)) and o.shape[0] > 0):
            return _Activate.apply(o, s, q)
        return self.get_opacity, self.get_scaling, self.get_rotation

    def setup_functions(self):
        self.scaling_activation = torch.exp
        self.scaling_inverse_activation = torch.log
        self.covariance_activation = _covariance_from_scaling_rotation
        self.opacity_activation = torch.sigmoid
        self.inverse_opacity_activation = inverse_sigmoid
        self.rotation_activation = torch.nn.functional.normalize

    def __init__(self, sh_degree: int, device="cuda"):
        self.device = torch.device(device)
        self.active_sh_degree = 0
        self.max_sh_degree = sh_degree
        for _, attr in _GROUPS:
            setattr(self, attr, torch.empty(0))
        self.max_radii2D = torch.empty(0)
        self.xyz_gradient_accum = torch.empty(0)
        self.denom = torch.empty(0)
        self.optimizer = None
        self.percent_dense = 0
        self.spatial_lr_scale = 0
        self.setup_functions()

    # ------------------------------------------------------------------ state hand-off
    def capture(self):
        return (self.active_sh_degree, self._xyz, self._features_dc, self._features_rest, self._scaling, self._rotation,
                self._opacity, self.max_radii2D, self.xyz_gradient_accum, self.denom, self.optimizer.state_dict(),
                self.spatial_lr_scale)

    def restore(self, model_args, training_args):
        (self.active_sh_degree, self._xyz, self._features_dc, self._features_rest, self._scaling, self._rotation,
         self._opacity, self.max_radii2D, grad_accum, denom, opt_dict, self.spatial_lr_scale) = model_args
        self.training_setup(training_args)
        self.xyz_gradient_accum, self.denom = grad_accum, denom
        self.optimizer.load_state_dict(opt_dict)

    # ------------------------------------------------------------------ activated views
    @property
    def get_scaling(self):
        return self.scaling_activation(self._scaling)

    @property
    def get_rotation(self):
        return self.rotation_activation(self._rotation)

    @property
    def get_xyz(self):
        return self._xyz

    @property
    def get_features(self):
        return torch.cat((self._features_dc, self._features_rest), dim=1)

    @property
    def get_opacity(self):
        return self.opacity_activation(self._opacity)

    def get_covariance(self, scaling_modifier=1):
        # raw (un-normalised) rotation: build_rotation normalises it (reference quirk kept, :106-107)
        return self.covariance_activation(self.get_scaling, scaling_modifier, self._rotation)

    def oneupSHdegree(self):
        if self.active_sh_degree < self.max_sh_degree:
            self.active_sh_degree += 1

    # ------------------------------------------------------------------ density field and mesh (gs_renderer.py:240-361)
    def _field_geometry(self, what, resolution, num_blocks):
        """The argument checks shared by extract_fields and sample_fields; (resolution, num_blocks) as ints."""
        resolution, num_blocks = int(resolution), int(num_blocks)
        if resolution < 1 or num_blocks < 1 or resolution % num_blocks != 0:
            raise ValueError("%s: num_blocks (%d) must divide resolution (%d)" % (what, num_blocks, resolution))
        if num_blocks > 1024:
            raise ValueError("%s: at most 1024 blocks per axis" % what)
        if not self._xyz.is_cuda:
            raise RuntimeError("%s runs on the GPU only (the model's tensors are on %s)" % (what, self._xyz.device))
        return resolution, num_blocks

    def _field_sources(self):
        """(mask, xyz, opacity [P], scaling, rotation) of the Gaussians the density field is made of — those with opacity > 0.005 —
        or None when there are none; sets self.center / self.scale, the normalisation to ~ [-1, 1] (gs_renderer.py:252-261)."""
        opacities = self.get_opacity.float()
        mask = (opacities > 0.005).squeeze(1)         # pre-filter, :252
        opacities = opacities[mask].reshape(-1).contiguous()
        if int(opacities.shape[0]) == 0:
            return None
        xyzs = self.get_xyz.float()[mask].contiguous()
        stds = self.get_scaling.float()[mask].contiguous()
        rots = self._rotation.float()[mask].contiguous()
        mn, mx = xyzs.amin(0), xyzs.amax(0)           # normalise to ~ [-1, 1], :259-261
        self.center = (mn + mx) / 2
        extent = (mx - mn).amax().item()
        self.scale = 1.8 / extent if extent > 0 else 1.0      # a single centre has no extent (the reference divides by zero there)
        return mask, xyzs, opacities, stds, rots

    def _field_call(self, entry, src, colors, resolution, num_blocks, relax_ratio, before, after):
        """One call of the C entry `entry` of the field family (gip_density_field, gip_field_sample, gip_texture_bake) on the sources
        `src` of _field_sources(): the sources (with `colors` [N, 3] of the whole model cut to them, unless None) and the geometry,
        then the entry's own arguments `before` and `after` the workspace; tensors go by address (_lib.ptr)."""
        import ctypes

        from .. import _lib
        mask, xyzs, opacities, stds, rots = src
        dev = xyzs.device
        P = int(opacities.shape[0])
        grid = torch.linspace(-1, 1, resolution, dtype=torch.float32).to(dev)      # the host's values: the cut below depends on their bits
        margin = (2 / num_blocks) * relax_ratio       # rounded to float32 on the way in, like `vmin -= block_size * relax_ratio`
        need = ctypes.c_size_t(0)
        _lib.query_model("gip_field_workspace_size", P, resolution, num_blocks, ctypes.byref(need))
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        rgb = () if colors is None else (colors.float()[mask].contiguous(),)
        args = ((xyzs, opacities, stds, rots) + rgb + (P, self.center.contiguous(), self.scale, grid, resolution, num_blocks, margin) +
                tuple(before) + (ws, need.value) + tuple(after))
        _lib.call_model(dev, entry, *(_lib.ptr(a) if isinstance(a, torch.Tensor) else a for a in args))

    @staticmethod
    def _point_blocks(u, resolution, num_blocks):
        """The block [V] (int64, (bx * nb + by) * nb + bz) each normalised point of u [V, 3] is evaluated in: per axis the block of the
        last grid value <= the coordinate (points outside the grid: the edge blocks)."""
        grid = torch.linspace(-1, 1, resolution, dtype=torch.float32).to(u.device)      # as in _field_call: exact for grid values
        cell = (torch.bucketize(u.contiguous(), grid, right=True) - 1).clamp(0, resolution - 1) // (resolution // num_blocks)
        return (cell[:, 0] * num_blocks + cell[:, 1]) * num_blocks + cell[:, 2]

    def _colors(self, what, colors):
        """`colors` checked: [N, 3] per Gaussian of the model (before the opacity prefilter); None = the base colour."""
        from ..utils.sh import C0
        if colors is None:
            colors = (0.5 + C0 * self._features_dc.float().reshape(-1, 3)).clamp(0, 1)
        if not (isinstance(colors, torch.Tensor) and colors.device == self._xyz.device and colors.dim() == 2 and
                tuple(colors.shape) == (self._xyz.shape[0], 3)):
            raise ValueError("%s: colors must be an [N, 3] tensor on the model's device, one row per Gaussian" % what)
        return colors

    @torch.no_grad()
    def extract_fields(self, resolution=128, num_blocks=16, relax_ratio=1.5):
        """The density of the Gaussians on a resolution^3 grid over the normalised cloud ([R, R, R] float32, `ij` order), the
        reference's GaussianModel.extract_fields (gs_renderer.py:240-331) in two launches (csrc/field.hip) instead of a Python loop
        over num_blocks^3 blocks: Gaussians with opacity > 0.005, normalised by self.center / self.scale (set here, as there), each
        contributing to the blocks whose box, relaxed by relax_ratio block sizes, strictly contains its centre.
        ValueError when num_blocks does not divide resolution (the reference's behaviour there is an accident of Tensor.split)."""
        resolution, num_blocks = self._field_geometry("extract_fields", resolution, num_blocks)
        occ = torch.zeros((resolution,) * 3, dtype=torch.float32, device=self._xyz.device)
        src = self._field_sources()
        if src is not None:
            self._field_call("gip_density_field", src, None, resolution, num_blocks, relax_ratio, (), (occ,))
        return occ

    @torch.no_grad()
    def extract_mesh(self, path=None, density_thresh=1.0, resolution=128, num_blocks=16, relax_ratio=1.5, *, clean=False, min_faces=8,
                     min_diameter=0.05, decimate_target=0):
        """(vertices [V, 3] float32 in world coordinates, faces [F, 3] int32) of the surface density == density_thresh, written as a
        Wavefront OBJ when `path` is given.  gs_renderer.py:333-350; the surface is extracted by marching tetrahedra on the GPU
        (utils/mesh.py) instead of mcubes, so it is closed by construction.  clean=True drops the floaters (utils.mesh.clean_mesh with
        min_faces and min_diameter, the reference's clean_mesh without its remeshing); decimate_target > 0 then reduces the mesh to at
        most that many faces (utils.mesh.decimate_mesh: vertex clustering, which does not preserve manifoldness in parts thinner than
        a cell; the reference's decimate_target is 1e5).  With the defaults neither runs and the result is the plain surface."""
        from ..utils import mesh
        occ = self.extract_fields(resolution, num_blocks, relax_ratio)
        vertices, faces = mesh.extract_surface(occ, density_thresh)
        if vertices.shape[0]:
            vertices = vertices / (resolution - 1.0) * 2 - 1
            vertices = vertices / self.scale + self.center       # back to the original space, :344
        if clean or decimate_target:
            vertices, faces, _, _ = self._clean_decimate(vertices, faces, clean, min_faces, min_diameter, decimate_target)
        if path is not None:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            mesh.write_obj(path, vertices, faces)
        return vertices, faces

    @staticmethod
    def _clean_decimate(vertices, faces, clean, min_faces, min_diameter, decimate_target):
        """The reference's order (gs_renderer.py:346-350): clean, then decimate.  (vertices, faces, vertex_map or None, moved):
        vertex_map [V_in] int32 of the cleaning alone (None without it); moved: the decimation replaced the vertices."""
        from ..utils import mesh
        if not decimate_target >= 0:
            raise ValueError("decimate_target must not be negative (0: no decimation)")
        vertex_map, moved = None, False
        if clean and faces.shape[0]:
            vertices, faces, info = mesh.clean_mesh(vertices, faces, min_faces, min_diameter, validate=False)      # the extraction's own faces
            vertex_map = info["vertex_map"]
        if decimate_target and faces.shape[0] > int(decimate_target):
            vertices, faces, _, grid = mesh.decimate_mesh(vertices, faces, int(decimate_target))
            moved = grid != 0
        return vertices, faces, vertex_map, moved

    def _sample(self, what, u, block, colors, resolution, num_blocks, relax_ratio):
        """density [V], gradient [V, 3] (normalised space) and colour sum [V, 3] at the normalised points u [V, 3], each evaluated in
        the block `block` [V] (int64, (bx * nb + by) * nb + bz) — one call of gip_field_sample (csrc/field_sample.hip).  Outputs in
        the caller's order.  `colors`: [N, 3] per Gaussian of the model (before the opacity prefilter), None = the base colour."""
        dev = self._xyz.device
        V = int(u.shape[0])
        out = {"density": torch.zeros(V, dtype=torch.float32, device=dev), "gradient": torch.zeros((V, 3), dtype=torch.float32, device=dev),
               "color_sum": torch.zeros((V, 3), dtype=torch.float32, device=dev)}
        colors = self._colors(what, colors)
        src = self._field_sources()
        if src is None or V == 0:
            return out
        order = torch.sort(block, stable=True).indices            # grouped by block, the caller's order kept inside a block
        counts = torch.bincount(block, minlength=num_blocks ** 3)
        block_start = torch.cat((counts.new_zeros(1), counts.cumsum(0))).to(torch.int32)
        pts = u[order].contiguous()
        dens, grad, csum = (torch.empty_like(out[k]) for k in ("density", "gradient", "color_sum"))
        self._field_call("gip_field_sample", src, colors, resolution, num_blocks, relax_ratio, (pts, block_start, V), (dens, grad, csum))
        out["density"][order], out["gradient"][order], out["color_sum"][order] = dens, grad, csum
        return out

    @staticmethod
    def _blend(color_sum, density):
        """color_sum / density where density > 0, else 0."""
        d = density.unsqueeze(1)
        return torch.where(d > 0, color_sum / d.clamp_min(torch.finfo(torch.float32).tiny), torch.zeros_like(color_sum))

    @torch.no_grad()
    def sample_fields(self, points, colors=None, resolution=128, num_blocks=16, relax_ratio=1.5, normalized=False):
        """{"density": [V], "gradient": [V, 3], "color": [V, 3]} of the density field at `points` ([V, 3] float32 GPU tensor, world
        coordinates, or normalised ones with normalized=True), in the caller's order.  The field is extract_fields': the same
        sources, normalisation, blocks and membership for the same (resolution, num_blocks, relax_ratio); a point is evaluated
        in the block of the last grid value <= its coordinate per axis (points outside the grid: the edge blocks), so a grid point
        gives its voxel of extract_fields.  gradient is d density / d point in world units; color is the weight-blended `colors`
        ([N, 3] per Gaussian; default the view-independent base colour 0.5 + C0 * features_dc, clamped to [0, 1]), 0 where the
        density is 0.  Raises like extract_fields, and ValueError for points that are not a [V, 3] float32 GPU tensor."""
        resolution, num_blocks = self._field_geometry("sample_fields", resolution, num_blocks)
        if not (isinstance(points, torch.Tensor) and points.is_cuda and points.dtype == torch.float32 and points.dim() == 2 and
                points.shape[1] == 3):
            raise ValueError("sample_fields needs a [V, 3] float32 GPU tensor of points")
        dev = self._xyz.device
        points = points.detach().to(dev)
        src = self._field_sources()                   # sets center / scale; None: nothing passes the prefilter, every sum is empty
        if normalized or src is None:
            u = points
        else:
            u = (points - self.center) * self.scale
        block = self._point_blocks(u, resolution, num_blocks)
        out = self._sample("sample_fields", u, block, colors, resolution, num_blocks, relax_ratio)
        scale = self.scale if src is not None else 1.0
        return {"density": out["density"], "gradient": out["gradient"] * scale, "color": self._blend(out["color_sum"], out["density"])}

    @torch.no_grad()
    def to_tetrahedra_sdf_grid(self, resolution=64, density_thresh=1.0, tets_path=None, feature_steps=0, feature_lr=0.01,
                               pos_encoding_config=None, mlp_network_config=None, **field_kwargs):
        """A utils.isosurface.TetrahedraSDFGrid that starts from this model's surface density == density_thresh: the bridge from the
        representation the project trains to a mesh whose vertices AND connectivity can be optimised further.  isosurface_bbox is the
        box of the normalised cloud, center -/+ 1 / scale; sdf = clamp(density_thresh - density, -1, 1) with the density of
        sample_fields(**field_kwargs) at the grid's vertices (the clamp is the reference's TetrahedraSDFGrid.create_from of an
        implicit volume); inside is negative, as in the reference.  resolution and tets_path choose the tetrahedral grid
        (utils.isosurface.MarchingTetrahedraHelper); the deformation starts at zero.  field_kwargs are sample_fields' num_blocks and
        relax_ratio, and field_resolution for its resolution (the name `resolution` is the tetrahedral grid's here).
        feature_steps > 0 gives the grid a feature network (n_feature_dims=3; pos_encoding_config and mlp_network_config as
        TetrahedraSDFGrid's, the reference's by default) and fits it with that many Adam steps at feature_lr to sample_fields'
        blended colour at the vertices of the extracted surface: the loss is the MSE of sigmoid(features).  The default 0 returns
        the geometry alone, as before."""
        from ..utils.isosurface import TetrahedraSDFGrid, scale_tensor
        if "field_resolution" in field_kwargs:
            field_kwargs["resolution"] = field_kwargs.pop("field_resolution")
        if set(field_kwargs) - {"resolution", "num_blocks", "relax_ratio"}:
            raise TypeError("to_tetrahedra_sdf_grid: unknown arguments %s" % sorted(set(field_kwargs) - {"resolution", "num_blocks", "relax_ratio"}))
        dev = self._xyz.device
        feature_steps = int(feature_steps)
        if feature_steps < 0:
            raise ValueError("to_tetrahedra_sdf_grid: feature_steps must not be negative")
        grid = TetrahedraSDFGrid(isosurface_resolution=resolution, tets_path=tets_path, n_feature_dims=3 if feature_steps else 0,
                                 pos_encoding_config=pos_encoding_config, mlp_network_config=mlp_network_config).to(dev)
        if self._field_sources() is not None:                # sets center / scale; without sources the box stays the unit one
            half = 1.0 / self.scale
            grid.isosurface_bbox.copy_(torch.stack((self.center - half, self.center + half)))
        helper = grid.isosurface_helper
        points = scale_tensor(helper.grid_vertices, helper.points_range, grid.isosurface_bbox).contiguous()
        density = self.sample_fields(points, **field_kwargs)["density"]
        grid.sdf.data = (float(density_thresh) - density).clamp(-1, 1).reshape(-1, 1)
        if feature_steps:
            vertices = grid.isosurface().v_pos.detach().contiguous()
            grid.mesh = None
            if vertices.shape[0]:
                target = self.sample_fields(vertices, **field_kwargs)["color"]
                with torch.enable_grad():
                    optimizer = torch.optim.Adam(list(grid.encoding.parameters()) + list(grid.feature_network.parameters()), lr=feature_lr)
                    for _ in range(feature_steps):
                        optimizer.zero_grad()
                        loss = ((torch.sigmoid(grid(vertices)["features"]) - target) ** 2).mean()
                        loss.backward()
                        optimizer.step()
        return grid

    @torch.no_grad()
    def extract_mesh_with_attributes(self, path=None, density_thresh=1.0, resolution=128, num_blocks=16, relax_ratio=1.5, colors=None, *,
                                     clean=False, min_faces=8, min_diameter=0.05, decimate_target=0):
        """(vertices [V, 3] float32, faces [F, 3] int32, normals [V, 3] float32, colors [V, 3] float32 in [0, 1]): extract_mesh's
        vertices and faces, bit for bit, with the Gaussians sampled at the vertices (sample_fields' sums; a vertex is evaluated in the
        block of the grid point that owns its edge).  normals = -gradient / |gradient|: analytic, toward decreasing density like the
        faces' winding, zero where the gradient is zero.  colors: the blend of `colors` (default: the base colour), which must lie
        in [0, 1] for the result to.  `path` ending in .ply writes a binary PLY, any other path a Wavefront OBJ.
        clean, min_faces, min_diameter, decimate_target: extract_mesh's.  After cleaning alone the normals and colours are the kept
        vertices' rows of the uncleaned result, bit for bit; a decimation moves the vertices, so normals and colours are then
        sample_fields' at the new vertices (evaluated in the block that holds each).  The written file follows the final mesh."""
        from ..utils import mesh
        resolution, num_blocks = self._field_geometry("extract_mesh_with_attributes", resolution, num_blocks)
        occ = self.extract_fields(resolution, num_blocks, relax_ratio)
        v, faces = mesh.extract_surface(occ, density_thresh)
        vertices = v
        if v.shape[0]:
            vertices = v / (resolution - 1.0) * 2 - 1
            u = vertices
            vertices = vertices / self.scale + self.center       # back to the original space, as extract_mesh
            cell = v.floor().long().clamp(0, resolution - 1) // (resolution // num_blocks)
            block = (cell[:, 0] * num_blocks + cell[:, 1]) * num_blocks + cell[:, 2]
            out = self._sample("extract_mesh_with_attributes", u, block, colors, resolution, num_blocks, relax_ratio)
            g = out["gradient"].double()
            n = g.norm(dim=1, keepdim=True)
            normals = torch.where(n > 0, -g / n.clamp_min(1e-300), torch.zeros_like(g)).float()
            vcolors = self._blend(out["color_sum"], out["density"])
        else:
            normals, vcolors = torch.zeros_like(v), torch.zeros_like(v)
        if clean or decimate_target:
            vertices, faces, vertex_map, moved = self._clean_decimate(vertices, faces, clean, min_faces, min_diameter, decimate_target)
            if moved:
                out = self.sample_fields(vertices, colors, resolution, num_blocks, relax_ratio)
                g = out["gradient"].double()
                n = g.norm(dim=1, keepdim=True)
                normals = torch.where(n > 0, -g / n.clamp_min(1e-300), torch.zeros_like(g)).float()
                vcolors = out["color"]
            elif vertex_map is not None:
                rows = torch.nonzero(vertex_map >= 0).reshape(-1)      # ascending: the kept vertices keep their order
                normals, vcolors = normals[rows], vcolors[rows]
        if path is not None:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            if str(path).lower().endswith(".ply"):
                mesh.write_ply_mesh(path, vertices, faces, colors=vcolors, normals=normals)
            else:
                mesh.write_obj(path, vertices, faces, colors=vcolors, normals=normals)
        return vertices, faces, normals, vcolors

    @staticmethod
    def _default_texture_size(F):
        """The smallest power of two >= 64 whose atlas has cells of side >= 8, at most 8192 (ValueError if F faces do not fit that)."""
        from ..utils import texture as tex
        size = 64
        while size < 8192:
            try:
                if tex.atlas_layout(F, size)[0] >= 8:
                    break
            except ValueError:
                pass
            size *= 2
        tex.atlas_layout(F, size)
        return size

    @torch.no_grad()
    def bake_texture(self, vertices, faces, texture_size=None, colors=None, resolution=128, num_blocks=16, relax_ratio=1.5, slices=None,
                     normalized=False):
        """{"texture": [T, T, 3] float32, "density": [T, T], "uv": [F, 3, 2] float32, "cell": c}: the weight-blended `colors` of the
        Gaussians baked into a T x T texture of the mesh (vertices [V, 3] float32 in world coordinates, faces [F, 3] int32, both on
        the GPU, as extract_mesh returns them; normalized=True: vertices in the field's normalised coordinates, as in
        sample_fields).  The atlas is utils/texture.py's: every face owns a right-isosceles triangle of texels in a cell of side c,
        `uv` are its corners' OBJ texture coordinates; row 0 of the texture is the top image row.  A texel is the field of
        sample_fields (same sources, normalisation, blocks and membership for the same resolution, num_blocks, relax_ratio) at its
        point on the face's plane, evaluated in the block of the face's centroid; texture = color_sum / density, 0 where the density
        is 0 or no face owns the texel, in [0, 1] when `colors` are.  One call of csrc/texture.hip, no point array.
        texture_size=None: the smallest power of two >= 64 with c >= 8, at most 8192.  colors: [N, 3] per Gaussian, default the base
        colour (a view-dependent colour from one direction is baked by passing it here).  slices: workgroups a block's texels are
        spread over (None: from the fullest block); the result does not depend on it.  Raises like sample_fields, and ValueError
        for faces that do not fit the texture or index outside [0, V)."""
        out = self._bake_sums(vertices, faces, texture_size, colors, resolution, num_blocks, relax_ratio, slices, normalized)
        T = out["density"].shape[0]
        texture = self._blend(out["color_sum"].reshape(-1, 3), out["density"].reshape(-1)).reshape(T, T, 3)
        return {"texture": texture, "density": out["density"], "uv": out["uv"], "cell": out["cell"]}

    @torch.no_grad()
    def _bake_sums(self, vertices, faces, texture_size=None, colors=None, resolution=128, num_blocks=16, relax_ratio=1.5, slices=None,
                   normalized=False):
        """bake_texture's checks and its one call of gip_texture_bake: {"density": [T, T], "color_sum": [T, T, 3], "uv", "cell"}, the
        raw sums (0 at unowned texels)."""
        from ..utils import texture as tex
        from ..utils.mesh import _mesh_args
        resolution, num_blocks = self._field_geometry("bake_texture", resolution, num_blocks)
        dev = self._xyz.device
        vertices, faces = _mesh_args("bake_texture", vertices, faces)
        if slices is not None and not 1 <= int(slices) <= 65535:
            raise ValueError("bake_texture: slices must lie in 1 .. 65535")
        V, F = int(vertices.shape[0]), int(faces.shape[0])
        T = self._default_texture_size(F) if texture_size is None else int(texture_size)
        if T < 4 or T > 16384:
            raise ValueError("bake_texture: texture_size must lie in 4 .. 16384")
        c, _, _ = tex.atlas_layout(F, T)
        colors = self._colors("bake_texture", colors)
        density = torch.zeros((T, T), dtype=torch.float32, device=dev)
        color_sum = torch.zeros((T, T, 3), dtype=torch.float32, device=dev)
        out = {"density": density, "color_sum": color_sum, "uv": torch.from_numpy(tex.atlas_uv(F, T)).to(dev), "cell": c}
        if F == 0:
            return out
        vertices, faces = vertices.to(dev), faces.to(dev)
        src = self._field_sources()
        fl = faces.long()
        if src is not None and V > 0:
            u = vertices if normalized else ((vertices - self.center) * self.scale).contiguous()
            tri = u[fl.clamp(0, V - 1)]
            block = self._point_blocks((tri[:, 0] + tri[:, 1] + tri[:, 2]) / 3, resolution, num_blocks)
            counts = torch.bincount(block, minlength=num_blocks ** 3)
            lo, hi, fullest = (int(x) for x in torch.stack((fl.min(), fl.max(), counts.max())).cpu())      # the one host read
        else:
            lo, hi = (int(x) for x in torch.stack((fl.min(), fl.max())).cpu())
        if lo < 0 or hi >= V:
            raise ValueError("bake_texture: face indices must lie in [0, %d)" % V)
        if src is None:
            return out
        if slices is None:      # one pass (256 lanes * 4 texels) per workgroup of the fullest block, within reason
            slices = min(max((fullest * (c * (c + 1) // 2) + 1023) // 1024, 1), 1024)
        face_order = torch.sort(block, stable=True).indices.to(torch.int32)
        block_start = torch.cat((counts.new_zeros(1), counts.cumsum(0))).to(torch.int32)
        self._field_call("gip_texture_bake", src, colors, resolution, num_blocks, relax_ratio,
                         (u, V, faces, F, face_order, block_start, T, c, int(slices)), (density, color_sum))
        return out

    @torch.no_grad()
    def bake_chart_texture(self, vertices, faces, atlas, colors=None, resolution=128, num_blocks=16, relax_ratio=1.5):
        """{"texture": [T, T, 3] float32, "covered": [T, T] bool, "filled": [T, T] bool, "uv": [F, 3, 2], "atlas": atlas}: the
        weight-blended `colors` of the Gaussians baked into the chart atlas `atlas` (utils.uv_atlas.unwrap_charts of this mesh: vertices
        [V, 3] float32 world coordinates, faces [F, 3] int32, on the GPU) — the reference's exporter (threestudio/models/exporters/
        mesh_exporter.py:53-137) with the project's own unwrapping, rasteriser and seam padding.  atlas.texel_points gives the covered
        texels and their points on the surface, sample_fields the colour there (`colors`, resolution, num_blocks, relax_ratio are
        that method's), and utils.uv_atlas.dilate_texture pads the seams by atlas.pad rounds; `filled` marks what holds a colour
        after that, every other texel is 0.  Raises like sample_fields, and ValueError for an atlas of another face list."""
        from ..utils.mesh import _mesh_args
        from ..utils.uv_atlas import ChartAtlas, dilate_texture
        vertices, faces = _mesh_args("bake_chart_texture", vertices, faces)
        if not isinstance(atlas, ChartAtlas) or tuple(atlas.t_tex_idx.shape) != tuple(faces.shape):
            raise ValueError("bake_chart_texture: atlas must be the ChartAtlas of these faces")
        T = int(atlas.texture_size)
        dev = vertices.device
        covered, points, _ = atlas.texel_points(vertices)
        texture = torch.zeros((T, T, 3), dtype=torch.float32, device=dev)
        at = points[covered].contiguous()
        if at.shape[0]:
            texture[covered] = self.sample_fields(at, colors, resolution, num_blocks, relax_ratio)["color"].to(dev)
        texture, filled = dilate_texture(texture, covered, atlas.pad)
        return {"texture": texture, "covered": covered, "filled": filled, "uv": atlas.uv, "atlas": atlas}

    @torch.no_grad()
    def bake_texture_from_views(self, vertices, faces, cameras, pipe=None, texture_size=None, images=None, alphas=None, depth_tolerance=None,
                                *, min_cos=0.2, min_alpha=0.5, two_sided=True, unpremultiply=None, colors=None, resolution=128,
                                num_blocks=16, relax_ratio=1.5):
        """{"texture": [T, T, 3] float32, "count": [T, T] int32, "weight_sum": [T, T], "uv": [F, 3, 2], "cell": c}: the texture of the
        mesh (vertices [V, 3] float32 world coordinates, faces [F, 3] int32, on the GPU) baked from what `cameras` see — the way
        the reference's exporter textures its mesh, gathered per texel instead of scattered and inpainted.  The views are projected
        onto the atlas of bake_texture by utils.texture.project_views behind the visibility of utils.texture.visible_depth; a texel
        that at least one view passes (count > 0) is color_sum / weight_sum, the views blended by cos^2 of the viewing angle; every
        other texel is bake_texture's value, bit for bit (`colors`, resolution, num_blocks, relax_ratio are that method's).
        images=None: the Gaussians are rendered here with render_views over a black background (camera by camera when
        pipe.convert_SHs_python forbids the batched call), the looked-up colour is divided by the looked-up alpha
        (unpremultiply=None reads as True) and a view counts where that alpha is >= min_alpha.  images [K, 3, H, W] with optional
        alphas [K, 1, H, W] (for example refined views with their cameras) skip the render; `pipe` may then be None and
        unpremultiply=None reads as False.  depth_tolerance=None: one grid spacing of the extraction in world units.  min_cos,
        min_alpha, two_sided: project_views'.  Raises like bake_texture and project_views."""
        from ..utils import texture as tex
        cams = list(cameras) if isinstance(cameras, (list, tuple)) else [cameras]
        tex._view_size("bake_texture_from_views", cams)
        if unpremultiply is None:
            unpremultiply = images is None
        if unpremultiply and not float(min_alpha) > 0:
            raise ValueError("bake_texture_from_views: unpremultiply needs min_alpha > 0")
        field = self.bake_texture(vertices, faces, texture_size, colors, resolution, num_blocks, relax_ratio)
        T = int(field["texture"].shape[0])
        dev = field["texture"].device
        if images is None:
            from ..renderer import render, render_views
            if pipe is None:
                raise ValueError("bake_texture_from_views needs `pipe` to render the views (or images=)")
            bg = torch.zeros(3, dtype=torch.float32, device=dev)
            if getattr(pipe, "convert_SHs_python", False):
                pkgs = [render(c, self, pipe, bg) for c in cams]
                images = torch.stack([p["render"] for p in pkgs])
                alphas = torch.stack([p["alpha_3dgs"] for p in pkgs])
            else:
                from .._lib import GIP_MAX_VIEWS as step      # render_views' limit per call
                pkgs = [render_views(cams[i:i + step], self, pipe, bg) for i in range(0, len(cams), step)]
                images = torch.cat([p["render"] for p in pkgs])
                alphas = torch.cat([p["alpha_3dgs"] for p in pkgs])
            images, alphas = images.detach().float().contiguous(), alphas.detach().float().contiguous()
        if depth_tolerance is None:
            scale = float(self.scale) if self._field_sources() is not None else 1.0
            depth_tolerance = 2.0 / max(int(resolution) - 1, 1) / scale
        vertices, faces = vertices.detach().to(dev).contiguous(), faces.detach().to(dev).contiguous()
        vis = tex.visible_depth(cams, vertices, faces, validate=False)       # bake_texture has checked the indices
        out = tex.project_views(vertices, faces, T, cams, images, vis, depth_tolerance=depth_tolerance, alphas=alphas, min_cos=min_cos,
                                min_alpha=min_alpha, two_sided=two_sided, unpremultiply=unpremultiply)
        seen = (out["count"] > 0).unsqueeze(2)
        texture = torch.where(seen, out["color_sum"] / out["weight_sum"].clamp_min(torch.finfo(torch.float32).tiny).unsqueeze(2),
                              field["texture"])
        return {"texture": texture, "count": out["count"], "weight_sum": out["weight_sum"], "uv": out["uv"], "cell": out["cell"]}

    @torch.no_grad()
    def extract_textured_mesh(self, path=None, density_thresh=1.0, resolution=128, num_blocks=16, relax_ratio=1.5, texture_size=None,
                              colors=None, *, clean=False, min_faces=8, min_diameter=0.05, decimate_target=0, bake="field", cameras=None,
                              pipe=None, atlas="faces", **view_kwargs):
        """(vertices [V, 3], faces [F, 3] int32, normals [V, 3], uv [F, 3, 2], texture [T, T, 3]): the mesh and normals of
        extract_mesh_with_attributes, bit for bit, with bake_texture's atlas and texture in place of vertex colours — the reference's
        export_obj_with_mtl (threestudio/models/exporters/mesh_exporter.py:53-137) without its third-party unwrapping, rasterising
        and inpainting.  With path = dir/name.obj it writes name.obj, name.mtl and name_kd.png (utils.mesh.write_obj_textured).
        clean, min_faces, min_diameter, decimate_target: extract_mesh_with_attributes'; the texture is baked on the cleaned and
        decimated mesh (fewer faces: larger atlas cells at the same texture size), and the files follow it.
        bake="views": the texture is bake_texture_from_views' from `cameras` (ValueError without any) with `pipe` and the further
        keywords of that method (images, alphas, depth_tolerance, min_cos, min_alpha, two_sided, unpremultiply); the default
        bake="field" takes none of them.
        atlas="charts": the mesh is unwrapped into a chart atlas (utils.uv_atlas.unwrap_charts at texture_size) and the texture is
        bake_chart_texture's: continuous UVs that neighbouring faces share, which the mipmapped lookup and an image editor can use;
        uv is still [F, 3, 2] (the atlas' v_tex[t_tex_idx]) and the OBJ shares its `vt` lines between faces.  The default
        atlas="faces" is the fixed per-face atlas.  bake="views" with atlas="charts" raises NotImplementedError."""
        from ..utils import mesh
        if bake not in ("field", "views"):
            raise ValueError("extract_textured_mesh: bake must be 'field' or 'views', not %r" % (bake,))
        if atlas not in ("faces", "charts"):
            raise ValueError("extract_textured_mesh: atlas must be 'faces' or 'charts', not %r" % (atlas,))
        if atlas == "charts" and bake == "views":
            raise NotImplementedError("extract_textured_mesh: bake='views' is not available with atlas='charts': project_views is built on "
                                      "the per-face atlas; use bake='field' or atlas='faces'")
        if bake == "views" and (cameras is None or (isinstance(cameras, (list, tuple)) and len(cameras) == 0)):
            raise ValueError("extract_textured_mesh: bake='views' needs cameras")
        if bake == "field" and (cameras is not None or pipe is not None or view_kwargs):
            raise ValueError("extract_textured_mesh: cameras, pipe and %s belong to bake='views'" % (sorted(view_kwargs) or "its keywords"))
        vertices, faces, normals, _ = self.extract_mesh_with_attributes(None, density_thresh, resolution, num_blocks, relax_ratio, colors,
                                                                        clean=clean, min_faces=min_faces, min_diameter=min_diameter,
                                                                        decimate_target=decimate_target)
        if atlas == "charts":
            from ..utils.uv_atlas import unwrap_charts
            size = self._default_texture_size(int(faces.shape[0])) if texture_size is None else int(texture_size)
            charts = unwrap_charts(vertices, faces, size)
            baked = self.bake_chart_texture(vertices, faces, charts, colors, resolution, num_blocks, relax_ratio)
            if path is not None:
                os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
                mesh.write_obj_textured(path, vertices, faces, charts.v_tex, baked["texture"], normals=normals, uv_idx=charts.t_tex_idx)
            return vertices, faces, normals, baked["uv"], baked["texture"]
        if bake == "views":
            baked = self.bake_texture_from_views(vertices, faces, cameras, pipe, texture_size, colors=colors, resolution=resolution,
                                                 num_blocks=num_blocks, relax_ratio=relax_ratio, **view_kwargs)
        else:
            baked = self.bake_texture(vertices, faces, texture_size, colors, resolution, num_blocks, relax_ratio)
        if path is not None:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            mesh.write_obj_textured(path, vertices, faces, baked["uv"], baked["texture"], normals=normals)
        return vertices, faces, normals, baked["uv"], baked["texture"]

    @torch.no_grad()
    def render_textured_mesh(self, camera, bg_color=None, position_gradients=False, antialias=False, *, clean=False, min_faces=8,
                             min_diameter=0.05, decimate_target=0, **extract_kwargs):
        """utils.rasterize.render_mesh of extract_textured_mesh(**extract_kwargs) from `camera` (or a list of cameras): the exported
        mesh on the pixel grid of the Gaussian render of the same camera.  The dict of render_mesh plus "mesh": the tuple that
        extract_textured_mesh returned.  position_gradients and antialias are render_mesh's keywords; clean, min_faces, min_diameter and
        decimate_target are extract_textured_mesh's."""
        from ..utils.rasterize import render_mesh
        if clean or decimate_target:
            extract_kwargs.update(clean=clean, min_faces=min_faces, min_diameter=min_diameter, decimate_target=decimate_target)
        mesh = self.extract_textured_mesh(**extract_kwargs)
        vertices, faces, _, uv, texture = mesh
        out = render_mesh(camera, vertices, faces, uv, texture, bg_color=bg_color, validate=False,      # the extraction's own faces
                          position_gradients=position_gradients, antialias=antialias)
        out["mesh"] = mesh
        return out

    @torch.no_grad()
    def render_field_volume(self, camera, num_samples_per_ray=256, density_scale=1.0, grid_resolution=32, bg_color=None, **field_kwargs):
        """The density-and-colour field that extract_mesh meshes, seen from `camera` by volume rendering (utils/volume.py):
        {"comp_rgb" [3, H, W], "opacity" [1, H, W], "depth" [1, H, W]} in the layout of render(...).  One ray per pixel centre from
        the camera's centre; the box is the normalised cloud's, center -/+ 1 / scale, as in to_tetrahedra_sdf_grid; its
        grid_resolution^3 occupancy grid is extract_fields(**field_kwargs) max-pooled, > 0; steps of 1.732 * 2 / scale /
        num_samples_per_ray; sigma = density_scale * density and the colour of sample_fields(**field_kwargs) at the samples'
        midpoints.  depth is the weighted sum of the midpoints' distances (not divided by the opacity).  bg_color: three numbers,
        black when absent; a pixel whose ray misses the box is exactly bg_color.  field_kwargs: resolution, num_blocks, relax_ratio."""
        import math

        from ..utils import volume
        if set(field_kwargs) - {"resolution", "num_blocks", "relax_ratio"}:
            raise TypeError("render_field_volume: unknown arguments %s" % sorted(set(field_kwargs) - {"resolution", "num_blocks", "relax_ratio"}))
        num_samples_per_ray, G = int(num_samples_per_ray), int(grid_resolution)
        if num_samples_per_ray < 1 or not 1 <= G <= volume.MAX_GRID:
            raise ValueError("render_field_volume: num_samples_per_ray must be at least 1 and grid_resolution lie in 1 .. %d" % volume.MAX_GRID)
        dev = self._xyz.device
        H, W = int(camera.image_height), int(camera.image_width)
        bg = torch.zeros(3, device=dev) if bg_color is None else torch.as_tensor(bg_color, dtype=torch.float32, device=dev).reshape(3)
        out = {"comp_rgb": bg[:, None, None].expand(3, H, W).clone(), "opacity": torch.zeros((1, H, W), device=dev),
               "depth": torch.zeros((1, H, W), device=dev)}
        field = self.extract_fields(**field_kwargs)                   # sets center / scale
        if self._field_sources() is None:
            return out
        occ = torch.nn.functional.adaptive_max_pool3d(field[None, None], G)[0, 0] > 0
        half = 1.0 / self.scale
        aabb = torch.cat((self.center - half, self.center + half))
        # the camera looks along +z with x to the right and y down; its matrices are stored transposed
        c2w = torch.linalg.inv(camera.world_view_transform.to(dev).float().t())
        fx, fy = W / (2.0 * math.tan(camera.FoVx / 2.0)), H / (2.0 * math.tan(camera.FoVy / 2.0))
        j, i = torch.meshgrid(torch.arange(H, dtype=torch.float32, device=dev) + 0.5, torch.arange(W, dtype=torch.float32, device=dev) + 0.5,
                              indexing="ij")
        directions = torch.stack(((i - W / 2.0) / fx, (j - H / 2.0) / fy, torch.ones_like(i)), dim=-1).reshape(-1, 3)
        rays_d = torch.nn.functional.normalize(directions @ c2w[:3, :3].t(), dim=-1).contiguous()
        rays_o = c2w[:3, 3].expand(rays_d.shape).contiguous()
        step = 1.732 * 2 * half / num_samples_per_ray
        ray_indices, t_starts, t_ends, _ = volume.march_rays(rays_o, rays_d, occ, aabb, step, max_samples_per_ray=num_samples_per_ray + 1)
        if ray_indices.shape[0] == 0:
            return out
        index = ray_indices.long()
        t_mid = ((t_starts + t_ends) / 2.0)[:, None]
        sampled = self.sample_fields((rays_o[index] + rays_d[index] * t_mid).contiguous(), **field_kwargs)
        sigmas = (float(density_scale) * sampled["density"]).contiguous()
        weights, _, _ = volume.render_weight_from_density(t_starts, t_ends, sigmas, ray_indices, H * W)
        opacity = volume.accumulate_along_rays(weights, None, ray_indices, H * W)
        depth = volume.accumulate_along_rays(weights, t_mid, ray_indices, H * W)
        rgb = volume.accumulate_along_rays(weights, sampled["color"].contiguous(), ray_indices, H * W)
        comp = rgb + bg * (1.0 - opacity)
        return {"comp_rgb": comp.t().reshape(3, H, W).contiguous(), "opacity": opacity.t().reshape(1, H, W).contiguous(),
                "depth": depth.t().reshape(1, H, W).contiguous()}

    # ------------------------------------------------------------------ initialisation
    def create_from_pcd(self, pcd: BasicPointCloud, spatial_lr_scale: float, dist2=None):
        """`dist2` (mean squared 3-NN distance per point) defaults to the HIP distCUDA2 replacement."""
        dev = self.device
        self.spatial_lr_scale = spatial_lr_scale
        pts = torch.tensor(np.asarray(pcd.points)).float().to(dev)
        n = pts.shape[0]
        n_coef = (self.max_sh_degree + 1) ** 2
        feats = torch.zeros((n, 3, n_coef), dtype=torch.float32, device=dev)
        feats[:, :3, 0] = RGB2SH(torch.tensor(np.asarray(pcd.colors)).float().to(dev))
        print("Number of points at initialisation : ", n)
        if dist2 is None:
            from ..knn import distCUDA2
            dist2 = distCUDA2(pts)
        dist2 = torch.clamp_min(torch.as_tensor(dist2, dtype=torch.float32, device=dev), 0.0000001)
        scales = torch.log(torch.sqrt(dist2))[..., None].repeat(1, 3)
        rots = torch.zeros((n, 4), device=dev)
        rots[:, 0] = 1
        opac = inverse_sigmoid(0.1 * torch.ones((n, 1), dtype=torch.float32, device=dev))
        self._xyz = nn.Parameter(pts.contiguous().requires_grad_(True))      # (a point array that arrives transposed keeps its strides otherwise)
        self._features_dc = nn.Parameter(feats[:, :, 0:1].transpose(1, 2).contiguous().requires_grad_(True))
        self._features_rest = nn.Parameter(feats[:, :, 1:].transpose(1, 2).contiguous().requires_grad_(True))
        self._scaling = nn.Parameter(scales.requires_grad_(True))
        self._rotation = nn.Parameter(rots.requires_grad_(True))
        self._opacity = nn.Parameter(opac.requires_grad_(True))
        self.max_radii2D = torch.zeros((n,), device=dev)

    def training_setup(self, training_args, fused: bool = False):
        """`fused=True` (GPU only): the same update rule as torch.optim.Adam with all six groups in ONE launch
        (scene/adam.py -> gip_adam_step; GIP_ADAM=torch selects torch's fused Adam, 18 launches), and the form that lets a
        GradScaler skip on the device: `scaler.step()` then issues no host synchronisation (the reference's plain Adam
        under `precision: 16-mixed` pays one `.item()` per step)."""
        n, dev = self.get_xyz.shape[0], self.get_xyz.device
        self.percent_dense = training_args.percent_dense
        self.xyz_gradient_accum = torch.zeros((n, 1), device=dev)
        self.denom = torch.zeros((n, 1), device=dev)
        lrs = {"xyz": training_args.position_lr_init * self.spatial_lr_scale, "f_dc": training_args.feature_lr,
               "f_rest": training_args.feature_lr / 20.0, "opacity": training_args.opacity_lr,
               "scaling": training_args.scaling_lr, "rotation": training_args.rotation_lr}
        self.params_list = [{"params": [getattr(self, attr)], "lr": lrs[name], "name": name} for name, attr in _GROUPS]
        if fused and dev.type == "cuda":
            from .adam import GipAdam          # the same update as torch's fused Adam, all six groups in ONE launch
            self.optimizer = GipAdam(self.params_list, lr=0.0, eps=1e-15)
        else:
            self.optimizer = torch.optim.Adam(self.params_list, lr=0.0, eps=1e-15, **({"fused": True} if fused else {}))
        self.xyz_scheduler_args = get_expon_lr_func(
            lr_init=training_args.position_lr_init * self.spatial_lr_scale,
            lr_final=training_args.position_lr_final * self.spatial_lr_scale,
            lr_delay_mult=training_args.position_lr_delay_mult, max_steps=training_args.position_lr_max_steps)

    def update_learning_rate(self, iteration):
        for group in self.optimizer.param_groups:
            if group["name"] == "xyz":
                group["lr"] = self.xyz_scheduler_args(iteration)

    def set_refine_learning_rate(self, iteration):
        self.update_learning_rate(iteration)

    # ------------------------------------------------------------------ PLY (float32 columns, plyfile-compatible)
    def construct_list_of_attributes(self):
        names = ["x", "y", "z", "nx", "ny", "nz"]
        names += ["f_dc_%d" % i for i in range(self._features_dc.shape[1] * self._features_dc.shape[2])]
        names += ["f_rest_%d" % i for i in range(self._features_rest.shape[1] * self._features_rest.shape[2])]
        names.append("opacity")
        names += ["scale_%d" % i for i in range(self._scaling.shape[1])]
        names += ["rot_%d" % i for i in range(self._rotation.shape[1])]
        return names

    def save_ply(self, path):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        xyz = self._xyz.detach().cpu().numpy()
        cols = [xyz, np.zeros_like(xyz),
                self._features_dc.detach().transpose(1, 2).flatten(start_dim=1).contiguous().cpu().numpy(),
                self._features_rest.detach().transpose(1, 2).flatten(start_dim=1).contiguous().cpu().numpy(),
                self._opacity.detach().cpu().numpy(), self._scaling.detach().cpu().numpy(),
                self._rotation.detach().cpu().numpy()]
        table = np.concatenate(cols, axis=1).astype("<f4")
        names = self.construct_list_of_attributes()
        assert table.shape[1] == len(names)
        header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % table.shape[0]
        header += "".join("property float %s\n" % n for n in names) + "end_header\n"
        with open(path, "wb") as f:
            f.write(header.encode("ascii"))
            f.write(np.ascontiguousarray(table).tobytes())

    @staticmethod
    def _read_ply(path):
        with open(path, "rb") as f:
            names, n, fmt = [], 0, None
            while True:
                line = f.readline().decode("ascii").strip()
                if line.startswith("format"):
                    fmt = line.split()[1]
                elif line.startswith("element vertex"):
                    n = int(line.split()[-1])
                elif line.startswith("property"):
                    parts = line.split()
                    if parts[1] not in ("float", "float32"):
                        raise ValueError("only float32 vertex properties are supported: %s" % line)
                    names.append(parts[2])
                elif line == "end_header":
                    break
            if fmt != "binary_little_endian":
                raise ValueError("unsupported PLY format %r" % fmt)
            data = np.frombuffer(f.read(n * len(names) * 4), dtype="<f4").reshape(n, len(names))
        return {name: data[:, i] for i, name in enumerate(names)}

    def load_ply(self, path):
        col = self._read_ply(path)
        dev = self.device
        xyz = np.stack((col["x"], col["y"], col["z"]), axis=1)
        n = xyz.shape[0]

        def numbered(prefix):
            keys = sorted((k for k in col if k.startswith(prefix)), key=lambda k: int(k.split("_")[-1]))
            return np.stack([col[k] for k in keys], axis=1) if keys else np.zeros((n, 0), np.float32)

        f_dc = np.stack((col["f_dc_0"], col["f_dc_1"], col["f_dc_2"]), axis=1).reshape(n, 3, 1)
        f_rest = numbered("f_rest_")
        assert f_rest.shape[1] == 3 * (self.max_sh_degree + 1) ** 2 - 3
        f_rest = f_rest.reshape(n, 3, (self.max_sh_degree + 1) ** 2 - 1)

        def param(a):
            return nn.Parameter(torch.tensor(np.ascontiguousarray(a), dtype=torch.float, device=dev).requires_grad_(True))

        self._xyz = param(xyz)
        self._features_dc = nn.Parameter(torch.tensor(f_dc, dtype=torch.float, device=dev).transpose(1, 2).contiguous().requires_grad_(True))
        self._features_rest = nn.Parameter(torch.tensor(f_rest, dtype=torch.float, device=dev).transpose(1, 2).contiguous().requires_grad_(True))
        self._opacity = param(col["opacity"][..., None])
        self._scaling = param(numbered("scale_"))
        self._rotation = param(numbered("rot"))
        self.active_sh_degree = self.max_sh_degree

    # ------------------------------------------------------------------ optimizer surgery
    def _rebuild(self, transform, state_transform):
        """Replace every group's parameter by transform(name, old) and its Adam moments by state_transform(name, m);
        returns {name: new parameter}."""
        out = {}
        for group in self.optimizer.param_groups:
            assert len(group["params"]) == 1
            old = group["params"][0]
            state = self.optimizer.state.pop(old, None)
            new = nn.Parameter(transform(group["name"], old).requires_grad_(True))
            if state is not None:
                state["exp_avg"] = state_transform(group["name"], state["exp_avg"])
                state["exp_avg_sq"] = state_transform(group["name"], state["exp_avg_sq"])
                self.optimizer.state[new] = state
            group["params"][0] = new
            out[group["name"]] = new
        return out

    def _adopt(self, tensors):
        for name, attr in _GROUPS:
            if name in tensors:
                setattr(self, attr, tensors[name])

    def replace_tensor_to_optimizer(self, tensor, name):
        out = {}
        for group in self.optimizer.param_groups:
            if group["name"] != name:
                continue
            state = self.optimizer.state.pop(group["params"][0], None)
            state["exp_avg"] = torch.zeros_like(tensor)
            state["exp_avg_sq"] = torch.zeros_like(tensor)
            group["params"][0] = nn.Parameter(tensor.requires_grad_(True))
            self.optimizer.state[group["params"][0]] = state
            out[name] = group["params"][0]
        return out

    def reset_opacity(self):
        new = inverse_sigmoid(torch.min(self.get_opacity, torch.ones_like(self.get_opacity) * 0.01))
        self._opacity = self.replace_tensor_to_optimizer(new, "opacity")["opacity"]

    def _prune_optimizer(self, mask):
        return self._rebuild(lambda _n, p: p[mask], lambda _n, m: m[mask])

    def prune_points(self, mask):
        keep = ~mask
        self._adopt(self._prune_optimizer(keep))
        self.xyz_gradient_accum = self.xyz_gradient_accum[keep]
        self.denom = self.denom[keep]
        self.max_radii2D = self.max_radii2D[keep]

    def cat_tensors_to_optimizer(self, tensors_dict):
        return self._rebuild(lambda n, p: torch.cat((p, tensors_dict[n]), dim=0),
                             lambda n, m: torch.cat((m, torch.zeros_like(tensors_dict[n])), dim=0))

    def densification_postfix(self, new_xyz, new_features_dc, new_features_rest, new_opacities, new_scaling, new_rotation):
        self._adopt(self.cat_tensors_to_optimizer({"xyz": new_xyz, "f_dc": new_features_dc, "f_rest": new_features_rest,
                                                   "opacity": new_opacities, "scaling": new_scaling,
                                                   "rotation": new_rotation}))
        n, dev = self.get_xyz.shape[0], self.get_xyz.device
        self.xyz_gradient_accum = torch.zeros((n, 1), device=dev)
        self.denom = torch.zeros((n, 1), device=dev)
        self.max_radii2D = torch.zeros((n,), device=dev)

    # ------------------------------------------------------------------ densification
    def densify_and_split(self, grads, grad_threshold, scene_extent, N=2):
        n, dev = self.get_xyz.shape[0], self.get_xyz.device
        padded = torch.zeros((n,), device=dev)
        padded[:grads.shape[0]] = grads.squeeze()
        sel = (padded >= grad_threshold) & (self.get_scaling.max(dim=1).values > self.percent_dense * scene_extent)
        stds = self.get_scaling[sel].repeat(N, 1)
        samples = torch.normal(mean=torch.zeros((stds.size(0), 3), device=dev), std=stds)
        rots = build_rotation(self._rotation[sel]).repeat(N, 1, 1)
        new_xyz = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + self.get_xyz[sel].repeat(N, 1)
        new_scaling = self.scaling_inverse_activation(self.get_scaling[sel].repeat(N, 1) / (0.8 * N))
        self.densification_postfix(new_xyz, self._features_dc[sel].repeat(N, 1, 1), self._features_rest[sel].repeat(N, 1, 1),
                                   self._opacity[sel].repeat(N, 1), new_scaling, self._rotation[sel].repeat(N, 1))
        self.prune_points(torch.cat((sel, torch.zeros(N * int(sel.sum()), device=dev, dtype=torch.bool))))

    def densify_and_clone(self, grads, grad_threshold, scene_extent):
        sel = (torch.norm(grads, dim=-1) >= grad_threshold) & \
              (self.get_scaling.max(dim=1).values <= self.percent_dense * scene_extent)
        self.densification_postfix(self._xyz[sel], self._features_dc[sel], self._features_rest[sel], self._opacity[sel],
                                   self._scaling[sel], self._rotation[sel])

    def densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size, max_world_size):
        if self._xyz.is_cuda:
            return self._densify_and_prune_fused(max_grad, min_opacity, extent, max_screen_size, max_world_size)
        return self._densify_and_prune_stepwise(max_grad, min_opacity, extent, max_screen_size, max_world_size)

    def _gather_all(self, index, n_old, new_rows):
        """One launch (include/gip_model.h) rebuilds the six parameters and their Adam moments:
        row j <- old[index[j]] if index[j] < n_old else new_rows[name][index[j] - n_old] (moments of new rows: zeros)."""
        from .. import _lib
        n_out = int(index.numel())
        descs, outs, keep_alive = [], {}, []
        for group in self.optimizer.param_groups:
            name, old = group["name"], group["params"][0]
            new = new_rows[name].contiguous()
            dst = torch.empty((n_out,) + tuple(old.shape[1:]), dtype=old.dtype, device=old.device)
            rb = dst[0:1].numel() * dst.element_size() if n_out else 0     # zero for SH degree 0's empty f_rest rows
            if rb:
                descs.append((old.data.contiguous(), new, dst, rb))
            state = self.optimizer.state.get(old, None)
            moments = {}
            if state is not None and "exp_avg" in state:
                for key in ("exp_avg", "exp_avg_sq"):
                    mdst = torch.empty_like(dst)
                    if rb:
                        descs.append((state[key].contiguous(), None, mdst, rb))
                    moments[key] = mdst
            outs[name] = (dst, moments)
        arr = (_lib.GipGatherTensor * len(descs))()
        for i, (o, nw, d, rb) in enumerate(descs):
            arr[i].old_rows = o.data_ptr() if o.numel() else None
            arr[i].new_rows = nw.data_ptr() if (nw is not None and nw.numel()) else None
            arr[i].dst, arr[i].row_bytes = d.data_ptr(), rb
            keep_alive.append((o, nw, d))
        if descs:
            _lib.call_model(index.device, "gip_gather_rows", arr, len(descs), _lib.ptr(index), n_out, n_old)
        rebuilt = {}
        for group in self.optimizer.param_groups:
            old = group["params"][0]
            dst, moments = outs[group["name"]]
            state = self.optimizer.state.pop(old, None)
            new = nn.Parameter(dst.requires_grad_(True))
            if state is not None:
                state.update(moments)
                self.optimizer.state[new] = state
            group["params"][0] = new
            rebuilt[group["name"]] = new
        return rebuilt

    # ------------------------------------------------------------------ spatial order (not in the reference)
    @staticmethod
    def morton_order(xyz, bits=10):
        """Permutation that sorts points along a 3-D Morton (Z-order) curve.  Rendering is invariant under a permutation
        of the Gaussians (up to float summation order); a spatially coherent order lets the 256 Gaussians of a
        preprocess workgroup share tile-histogram atomics and keeps a tile's records close in memory."""
        lo, hi = xyz.min(dim=0).values, xyz.max(dim=0).values
        q = ((xyz - lo) / (hi - lo).clamp_min(1e-12) * (2 ** bits - 1)).long().clamp_(0, 2 ** bits - 1)
        code = torch.zeros(xyz.shape[0], dtype=torch.long, device=xyz.device)
        for b in range(bits):
            for a in range(3):
                code |= ((q[:, a] >> b) & 1) << (3 * b + a)
        return torch.argsort(code)

    def sort_spatially(self):
        """Re-order the Gaussians (parameters, Adam moments, densification statistics) along a Morton curve.  Call after
        create_from_pcd / densify_and_prune.  render() is unchanged up to float summation order and the order of entries
        with identical depth bits (ties are broken by Gaussian index, as in the reference)."""
        perm = self.morton_order(self._xyz.detach())
        if self.optimizer is not None and self._xyz.is_cuda:
            P = self._xyz.shape[0]
            empty = {g["name"]: g["params"][0].detach()[:0] for g in self.optimizer.param_groups}
            self._adopt(self._gather_all(perm.contiguous(), P, empty))
        else:
            for _, attr in _GROUPS:
                setattr(self, attr, nn.Parameter(getattr(self, attr).detach()[perm].requires_grad_(True)))
            if self.optimizer is not None:
                raise ValueError("sort_spatially on CPU must run before training_setup")
        for name in ("xyz_gradient_accum", "denom", "max_radii2D"):
            t = getattr(self, name)
            if t.numel() and t.shape[0] == perm.shape[0]:
                setattr(self, name, t[perm])
        return perm

    def _densify_and_prune_fused(self, max_grad, min_opacity, extent, max_screen_size, max_world_size, N=2):
        """densify_and_clone -> densify_and_split -> prune_points x2 of the reference (gaussian_model.py:357-411) with
        the same selections, the same torch.normal draw and the same final row order, but every tensor rebuilt ONCE:
        the survivors of [old | clones | split children] are described by one index list and moved by gip_gather_rows."""
        P, dev = self.get_xyz.shape[0], self.get_xyz.device
        grads = self.xyz_gradient_accum / self.denom
        grads[grads.isnan()] = 0.0
        scaling = self.get_scaling
        big = scaling.max(dim=1).values > self.percent_dense * extent
        clone_sel = (torch.norm(grads, dim=-1) >= max_grad) & ~big
        split_sel = (grads.squeeze(-1) >= max_grad) & big
        stds = scaling[split_sel].repeat(N, 1)
        samples = torch.normal(mean=torch.zeros((stds.size(0), 3), device=dev), std=stds)
        rots = build_rotation(self._rotation[split_sel]).repeat(N, 1, 1)
        child_xyz = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + self.get_xyz[split_sel].repeat(N, 1)
        child_scaling = self.scaling_inverse_activation(scaling[split_sel].repeat(N, 1) / (0.8 * N))
        new_rows = {
            "xyz": torch.cat((self._xyz[clone_sel], child_xyz)),
            "f_dc": torch.cat((self._features_dc[clone_sel], self._features_dc[split_sel].repeat(N, 1, 1))),
            "f_rest": torch.cat((self._features_rest[clone_sel], self._features_rest[split_sel].repeat(N, 1, 1))),
            "opacity": torch.cat((self._opacity[clone_sel], self._opacity[split_sel].repeat(N, 1))),
            "scaling": torch.cat((self._scaling[clone_sel], child_scaling)),
            "rotation": torch.cat((self._rotation[clone_sel], self._rotation[split_sel].repeat(N, 1))),
        }

        def pruned(opacity_raw, scaling_raw):
            m = (self.opacity_activation(opacity_raw) < min_opacity).squeeze(-1)
            if max_screen_size:     # max_radii2D was reset to zeros by the densification: only the world-size test can fire
                m = m | (torch.zeros_like(m, dtype=torch.float32) > max_screen_size) | \
                    (self.scaling_activation(scaling_raw).max(dim=1).values > max_world_size)
            return m
        keep_old = ~split_sel & ~pruned(self._opacity, self._scaling)
        keep_new = ~pruned(new_rows["opacity"], new_rows["scaling"])
        index = torch.cat((torch.nonzero(keep_old).squeeze(-1), P + torch.nonzero(keep_new).squeeze(-1))).contiguous()
        self._adopt(self._gather_all(index, P, new_rows))
        n = int(index.numel())
        self.xyz_gradient_accum = torch.zeros((n, 1), device=dev)
        self.denom = torch.zeros((n, 1), device=dev)
        self.max_radii2D = torch.zeros((n,), device=dev)
        torch.cuda.empty_cache()

    def _densify_and_prune_stepwise(self, max_grad, min_opacity, extent, max_screen_size, max_world_size):
        grads = self.xyz_gradient_accum / self.denom
        grads[grads.isnan()] = 0.0
        self.densify_and_clone(grads, max_grad, extent)
        self.densify_and_split(grads, max_grad, extent)
        prune = (self.get_opacity < min_opacity).squeeze()
        if max_screen_size:
            prune = prune | (self.max_radii2D > max_screen_size) | (self.get_scaling.max(dim=1).values > max_world_size)
        self.prune_points(prune)
        if self.get_xyz.is_cuda:
            torch.cuda.empty_cache()

    def prune_only(self, min_opacity=0.05, max_world_size=0.01):
        prune = (self.get_opacity < min_opacity).squeeze() | (self.get_scaling.max(dim=1).values > max_world_size)
        self.prune_points(prune)
        if self.get_xyz.is_cuda:
            torch.cuda.empty_cache()

    def add_densification_stats(self, viewspace_point_tensor, update_filter):
        """gaussian_model.py:420-422.  Written with a multiplicative mask instead of boolean-mask indexing: the same
        values (x + 0 == x), but no nonzero() and therefore no host synchronisation inside the training step."""
        m = update_filter.to(self.xyz_gradient_accum.dtype).unsqueeze(-1)
        self.xyz_gradient_accum += torch.norm(viewspace_point_tensor[:, :2], dim=-1, keepdim=True) * m
        self.denom += m
