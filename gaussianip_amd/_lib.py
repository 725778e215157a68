"""ctypes binding of the four HIP libraries: libgip_raster.so (include/gip_raster.h), libgip_knn.so (include/gip_knn.h),
libgip_model.so (include/gip_model.h: scene, loss, mesh, field, tet, hash-grid, volume and SDF-volume kernels) and libgip_nn.so (include/gip_nn.h: the
denoiser / VAE kernels and the guidance glue).

Host code launches through `call_model`, `call_nn` and `call_knn` (pointers from `ptr`, the device's current stream appended, a
RuntimeError naming the entry point on a non-zero status) and asks stream-less questions through `query_model`; the rasterizer has
its own plan-based path in rasterizer.py.  Entry points that return a size or a count, not a status, are called directly on
`model_lib()` / `nn_lib()` / `knn_lib()`.

The product path has NO CPU fallback: if the HIP library is missing, loading raises ImportError with build
instructions (`python -c "import __graft_entry__ as g; g.build()"`).
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(_HERE, "lib")

GIP_MAX_VIEWS = 16
GIP_RECORD_BYTES = 64
GIP_PARTIAL_FLOATS = 12
GIP_OK = 0

_vp = ctypes.c_void_p


class GipRasterConfig(ctypes.Structure):
    _fields_ = [("P", ctypes.c_int32), ("V", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32),
                ("sh_degree", ctypes.c_int32), ("sh_coeffs", ctypes.c_int32), ("prefiltered", ctypes.c_int32),
                ("debug", ctypes.c_int32), ("scale_modifier", ctypes.c_float),
                ("tanfovx", ctypes.c_float * GIP_MAX_VIEWS), ("tanfovy", ctypes.c_float * GIP_MAX_VIEWS),
                ("capacity", ctypes.c_uint64), ("exact_lists", ctypes.c_int32), ("forward_only", ctypes.c_int32),
                ("sh_scalar", ctypes.c_int32), ("antialiasing", ctypes.c_int32)]


class GipRasterInputs(ctypes.Structure):
    _fields_ = [(n, _vp) for n in ("means3D", "shs", "colors_precomp", "opacities", "scales", "rotations",
                                   "cov3D_precomp", "viewmatrix", "projmatrix", "campos", "bg")]


class GipRasterOutputs(ctypes.Structure):
    _fields_ = [(n, _vp) for n in ("color", "radii", "depth", "alpha", "host_header")]


class GipRasterGradsIn(ctypes.Structure):
    _fields_ = [(n, _vp) for n in ("dL_dcolor", "dL_ddepth", "dL_dalpha", "alpha", "color", "depth")]


class GipRasterGradsOut(ctypes.Structure):
    _fields_ = [(n, _vp) for n in ("dL_dmeans3D", "dL_dmeans2D", "dL_dshs", "dL_dcolors_precomp", "dL_dopacities",
                                   "dL_dscales", "dL_drotations", "dL_dcov3D_precomp")]


class GipRasterStateLayout(ctypes.Structure):
    _fields_ = [(n, ctypes.c_size_t) for n in ("header", "records", "inst_offset", "tile_count", "tile_start",
                                                "tile_cursor", "tile_count_b", "inst_slot", "block_sums", "block_offset", "keys", "n_contrib",
                                                "final_T", "tile_order", "seg_start", "ckpt_start", "seg_tile", "checkpoints", "sh_colors", "total")] + \
               [(n, ctypes.c_uint32) for n in ("tiles_x", "tiles_y", "num_blocks", "reserved")]


_raster = None
_knn = None


def _missing(name):
    return ImportError(
        "gaussianip_amd: %s not found in %s. The HIP extension must be built for gfx950 first "
        "(`python -c 'import __graft_entry__ as g; g.build()'` or `make -C gaussianip_amd/csrc`). "
        "There is no CPU fallback for the product path." % (name, LIB_DIR))


call_counts = {}       # C-ABI entry point -> number of calls through this module (tests assert that the HIP path ran)


class _Counted:
    """The loaded library with a per-symbol call counter in front of every entry point.  A `*_buckets` entry point of the
    rasterizer is the launch set of the entry point it extends with another key layout: it counts under that name as well."""

    def __init__(self, lib):
        self._lib = lib
        self._wrapped = {}

    def __getattr__(self, name):
        w = self._wrapped.get(name)
        if w is None:
            fn = getattr(self._lib, name)

            names = (name, name.replace("_buckets", "")) if name.startswith("gip_raster_") and "_buckets" in name else (name,)

            def w(*args, _fn=fn, _names=names):
                for n in _names:
                    call_counts[n] = call_counts.get(n, 0) + 1
                return _fn(*args)
            self._wrapped[name] = w
        return w


def raster_lib():
    global _raster
    if _raster is None:
        path = os.path.join(LIB_DIR, os.environ.get("GIP_RASTER_LIB", "libgip_raster.so"))
        if not os.path.exists(path):
            raise _missing("libgip_raster.so")
        lib = ctypes.CDLL(path)
        lib.gip_abi_version.restype = ctypes.c_int
        lib.gip_status_string.restype = ctypes.c_char_p
        lib.gip_status_string.argtypes = [ctypes.c_int]
        lib.gip_raster_state_bytes.restype = ctypes.c_size_t
        lib.gip_raster_state_bytes.argtypes = [ctypes.POINTER(GipRasterConfig)]
        lib.gip_raster_scratch_bytes.restype = ctypes.c_size_t
        lib.gip_raster_scratch_bytes.argtypes = [ctypes.POINTER(GipRasterConfig)]
        lib.gip_raster_state_layout.restype = ctypes.c_int
        lib.gip_raster_state_layout.argtypes = [ctypes.POINTER(GipRasterConfig), ctypes.POINTER(GipRasterStateLayout)]
        lib.gip_raster_forward.restype = ctypes.c_int
        lib.gip_raster_forward.argtypes = [ctypes.POINTER(GipRasterConfig), ctypes.POINTER(GipRasterInputs),
                                           ctypes.POINTER(GipRasterOutputs), _vp, ctypes.c_size_t, _vp]
        lib.gip_raster_backward.restype = ctypes.c_int
        lib.gip_raster_backward.argtypes = [ctypes.POINTER(GipRasterConfig), ctypes.POINTER(GipRasterInputs),
                                            ctypes.POINTER(GipRasterGradsIn), _vp, ctypes.c_size_t, _vp,
                                            ctypes.c_size_t, ctypes.POINTER(GipRasterGradsOut), _vp]
        lib.gip_raster_forward_profiled.restype = ctypes.c_int
        lib.gip_raster_forward_profiled.argtypes = lib.gip_raster_forward.argtypes + [ctypes.POINTER(ctypes.c_float)]
        lib.gip_raster_backward_profiled.restype = ctypes.c_int
        lib.gip_raster_backward_profiled.argtypes = lib.gip_raster_backward.argtypes + [ctypes.POINTER(ctypes.c_float)]
        # bucket mode (a per-tile key bucket of `bucket_stride` entries behind the dense layout; 0 = dense): additive entry points
        _u32 = ctypes.c_uint32
        lib.gip_raster_state_bytes_buckets.restype = ctypes.c_size_t
        lib.gip_raster_state_bytes_buckets.argtypes = [ctypes.POINTER(GipRasterConfig), _u32]
        lib.gip_raster_state_layout_buckets.restype = ctypes.c_int
        lib.gip_raster_state_layout_buckets.argtypes = [ctypes.POINTER(GipRasterConfig), _u32, ctypes.POINTER(GipRasterStateLayout),
                                                        ctypes.POINTER(ctypes.c_size_t)]
        lib.gip_raster_forward_buckets.restype = ctypes.c_int
        lib.gip_raster_forward_buckets.argtypes = lib.gip_raster_forward.argtypes + [_u32]
        lib.gip_raster_backward_buckets.restype = ctypes.c_int
        lib.gip_raster_backward_buckets.argtypes = lib.gip_raster_backward.argtypes + [_u32]
        lib.gip_raster_forward_buckets_profiled.restype = ctypes.c_int
        lib.gip_raster_forward_buckets_profiled.argtypes = lib.gip_raster_forward.argtypes + [_u32, ctypes.POINTER(ctypes.c_float)]
        lib.gip_raster_backward_buckets_profiled.restype = ctypes.c_int
        lib.gip_raster_backward_buckets_profiled.argtypes = lib.gip_raster_backward.argtypes + [_u32, ctypes.POINTER(ctypes.c_float)]
        lib.gip_raster_read_header.restype = ctypes.c_int
        lib.gip_raster_read_header.argtypes = [_vp, _vp, _vp]
        lib.gip_raster_mark_visible.restype = ctypes.c_int
        lib.gip_raster_mark_visible.argtypes = [ctypes.c_int32, _vp, _vp, _vp, _vp, _vp]
        _raster = _Counted(lib)
    return _raster


def knn_lib():
    global _knn
    if _knn is None:
        path = os.path.join(LIB_DIR, "libgip_knn.so")
        if not os.path.exists(path):
            raise _missing("libgip_knn.so")
        lib = ctypes.CDLL(path)
        lib.gip_knn_workspace_bytes.restype = ctypes.c_size_t
        lib.gip_knn_workspace_bytes.argtypes = [ctypes.c_int32]
        lib.gip_knn_mean_dist2.restype = ctypes.c_int
        lib.gip_knn_mean_dist2.argtypes = [ctypes.c_int32, _vp, _vp, _vp, ctypes.c_size_t, _vp]
        lib.gip_knn_workspace_bytes_mode.restype = ctypes.c_size_t
        lib.gip_knn_workspace_bytes_mode.argtypes = [ctypes.c_int32, ctypes.c_int32]
        lib.gip_knn_mean_dist2_mode.restype = ctypes.c_int
        lib.gip_knn_mean_dist2_mode.argtypes = [ctypes.c_int32, _vp, _vp, _vp, ctypes.c_size_t, ctypes.c_int32, _vp]
        _knn = _Counted(lib)
    return _knn


_model = None


class GipAdamGroup(ctypes.Structure):
    _fields_ = [("param", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p), ("exp_avg_sq", ctypes.c_void_p),
                ("step", ctypes.c_void_p), ("n", ctypes.c_int64), ("lr", ctypes.c_float), ("reserved", ctypes.c_int32)]


class GipGatherTensor(ctypes.Structure):
    _fields_ = [("old_rows", ctypes.c_void_p), ("new_rows", ctypes.c_void_p), ("dst", ctypes.c_void_p),
                ("row_bytes", ctypes.c_int32), ("reserved", ctypes.c_int32)]


def model_lib():
    global _model
    if _model is None:
        path = os.path.join(LIB_DIR, "libgip_model.so")
        if not os.path.exists(path):
            raise _missing("libgip_model.so")
        lib = ctypes.CDLL(path)
        lib.gip_gather_rows.restype = ctypes.c_int
        lib.gip_gather_rows.argtypes = [ctypes.POINTER(GipGatherTensor), ctypes.c_int32, _vp, ctypes.c_int64, ctypes.c_int64, _vp]
        lib.gip_adam_step.restype = ctypes.c_int
        lib.gip_adam_step.argtypes = [ctypes.POINTER(GipAdamGroup), ctypes.c_int32, ctypes.c_double, ctypes.c_double, ctypes.c_double, _vp, _vp]
        lib.gip_openpose_draw.restype = ctypes.c_int
        lib.gip_openpose_draw.argtypes = [_vp, _vp, _vp, _vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _vp, ctypes.c_size_t, _vp]
        lib.gip_openpose_workspace_bytes.restype = ctypes.c_size_t
        lib.gip_openpose_workspace_bytes.argtypes = [ctypes.c_int32, ctypes.c_int32]
        lib.gip_pack_bucket.restype = ctypes.c_int
        lib.gip_pack_bucket.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int64), ctypes.c_int32, _vp,
                                        ctypes.c_int32, ctypes.c_int64, _vp, _vp]
        lib.gip_max_bucket.restype = ctypes.c_int
        lib.gip_max_bucket.argtypes = [_vp, ctypes.c_int32, ctypes.c_int64, _vp, ctypes.c_int64, _vp, _vp]
        lib.gip_unpack_bucket.restype = ctypes.c_int
        lib.gip_unpack_bucket.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int64), ctypes.c_int32, _vp,
                                          ctypes.c_int64, _vp, ctypes.c_float, _vp]
        lib.gip_sparsity_workspace_bytes.restype = ctypes.c_size_t
        lib.gip_sparsity_workspace_bytes.argtypes = []
        lib.gip_sparsity_loss_forward.restype = ctypes.c_int
        lib.gip_sparsity_loss_forward.argtypes = [_vp, ctypes.c_int64, _vp, _vp]
        lib.gip_sparsity_loss_backward.restype = ctypes.c_int
        lib.gip_sparsity_loss_backward.argtypes = [_vp, ctypes.c_int64, _vp, ctypes.c_float, _vp, _vp, _vp]
        lib.gip_activate_gaussians.restype = ctypes.c_int
        lib.gip_activate_gaussians.argtypes = [_vp, _vp, _vp, ctypes.c_int64, _vp, _vp, _vp, _vp]
        lib.gip_activate_gaussians_backward.restype = ctypes.c_int
        lib.gip_activate_gaussians_backward.argtypes = [_vp] * 6 + [ctypes.c_int64, _vp, _vp, _vp, _vp]
        lib.gip_densify_stats.restype = ctypes.c_int
        lib.gip_densify_stats.argtypes = [_vp, ctypes.c_int32, ctypes.c_int64, _vp, _vp, _vp, _vp, _vp, _vp]
        lib.gip_ssim_workspace_bytes.restype = ctypes.c_size_t
        lib.gip_ssim_workspace_bytes.argtypes = [ctypes.c_int32] * 4
        lib.gip_ssim_forward.restype = ctypes.c_int
        lib.gip_ssim_forward.argtypes = [_vp, _vp] + [ctypes.c_int32] * 4 + [_vp, _vp, _vp, _vp, _vp]
        lib.gip_ssim_backward.restype = ctypes.c_int
        lib.gip_ssim_backward.argtypes = [_vp, _vp, _vp, _vp] + [ctypes.c_int32] * 4 + [_vp, _vp]
        lib.gip_field_workspace_size.restype = ctypes.c_int
        lib.gip_field_workspace_size.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_size_t)]
        lib.gip_density_field.restype = ctypes.c_int
        lib.gip_density_field.argtypes = [_vp, _vp, _vp, _vp, ctypes.c_int64, _vp, ctypes.c_float, _vp, ctypes.c_int32, ctypes.c_int32,
                                          ctypes.c_float, _vp, ctypes.c_size_t, _vp, _vp]
        lib.gip_surface_count.restype = ctypes.c_int
        lib.gip_surface_count.argtypes = [_vp, ctypes.c_int32, ctypes.c_float, _vp, _vp, _vp]
        lib.gip_surface_emit.restype = ctypes.c_int
        lib.gip_surface_emit.argtypes = [_vp, ctypes.c_int32, ctypes.c_float, _vp, _vp, _vp, _vp, _vp, _vp]
        lib.gip_field_sample_workspace_size.restype = ctypes.c_int
        lib.gip_field_sample_workspace_size.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_size_t)]
        lib.gip_field_sample.restype = ctypes.c_int
        lib.gip_field_sample.argtypes = [_vp, _vp, _vp, _vp, _vp, ctypes.c_int64, _vp, ctypes.c_float, _vp, ctypes.c_int32, ctypes.c_int32,
                                         ctypes.c_float, _vp, _vp, ctypes.c_int64, _vp, ctypes.c_size_t, _vp, _vp, _vp, _vp]
        lib.gip_texture_bake_workspace_size.restype = ctypes.c_int
        lib.gip_texture_bake_workspace_size.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_size_t)]
        lib.gip_texture_bake.restype = ctypes.c_int
        lib.gip_texture_bake.argtypes = [_vp, _vp, _vp, _vp, _vp, ctypes.c_int64, _vp, ctypes.c_float, _vp, ctypes.c_int32, ctypes.c_int32,
                                         ctypes.c_float, _vp, ctypes.c_int64, _vp, ctypes.c_int64, _vp, _vp, ctypes.c_int32, ctypes.c_int32,
                                         ctypes.c_int32, _vp, ctypes.c_size_t, _vp, _vp, _vp]
        lib.gip_texture_project.restype = ctypes.c_int
        lib.gip_texture_project.argtypes = [_vp, ctypes.c_int64, _vp, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _vp, _vp, _vp,
                                            ctypes.c_int32, ctypes.c_int32, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_int32,
                                            ctypes.c_int32, _vp, _vp, _vp, _vp]
        _i32, _i64 = ctypes.c_int32, ctypes.c_int64
        lib.gip_mesh_raster_workspace_size.restype = ctypes.c_int
        lib.gip_mesh_raster_workspace_size.argtypes = [_i32, _i32, _i32, _i64, ctypes.POINTER(ctypes.c_size_t)]
        lib.gip_mesh_rasterize.restype = ctypes.c_int
        lib.gip_mesh_rasterize.argtypes = [_vp, _vp, _i32, _i64, _i64, _i32, _i32, _i32, _vp, ctypes.c_size_t, _vp, _vp]
        lib.gip_mesh_interpolate.restype = ctypes.c_int
        lib.gip_mesh_interpolate.argtypes = [_vp, _i32, _i64, _i32, _vp, _i64, _vp, _i32, _i32, _i32, _vp, _vp]
        lib.gip_mesh_interpolate_backward.restype = ctypes.c_int
        lib.gip_mesh_interpolate_backward.argtypes = [_vp, _i32, _i64, _i32, _vp, _i64, _vp, _i32, _i32, _i32, _vp, _vp]
        lib.gip_mesh_texture.restype = ctypes.c_int
        lib.gip_mesh_texture.argtypes = [_vp, _i32, _i32, _i32, _i32, _vp, _i32, _i32, _i32, _vp, _vp]
        lib.gip_mesh_texture_backward.restype = ctypes.c_int
        lib.gip_mesh_texture_backward.argtypes = [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp]
        lib.gip_mesh_shade.restype = ctypes.c_int
        lib.gip_mesh_shade.argtypes = [_vp, _vp, _i64, _i32, _vp, _i32, _i32, _vp, _i32, _i32, _i32, _vp, _vp]
        lib.gip_mesh_shade_backward.restype = ctypes.c_int
        lib.gip_mesh_shade_backward.argtypes = [_vp, _vp, _i64, _i32, _vp, _i32, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _vp]
        lib.gip_mesh_rasterize_backward.restype = ctypes.c_int
        lib.gip_mesh_rasterize_backward.argtypes = [_vp, _vp, _i32, _i64, _i64, _i32, _i32, _vp, _vp, _vp, _vp]
        lib.gip_mesh_interpolate_backward_rast.restype = ctypes.c_int
        lib.gip_mesh_interpolate_backward_rast.argtypes = [_vp, _vp, _i32, _i64, _i32, _vp, _i64, _vp, _i32, _i32, _i32, _vp, _vp]
        lib.gip_mesh_shade_backward_rast.restype = ctypes.c_int
        lib.gip_mesh_shade_backward_rast.argtypes = [_vp, _vp, _i64, _i32, _vp, _i32, _i32, _vp, _i32, _i32, _i32, _vp, _vp]
        lib.gip_mesh_antialias.restype = ctypes.c_int
        lib.gip_mesh_antialias.argtypes = [_vp, _i32, _vp, _vp, _vp, _vp, _i32, _i64, _i64, _i32, _i32, _vp, _vp]
        lib.gip_mesh_antialias_backward.restype = ctypes.c_int
        lib.gip_mesh_antialias_backward.argtypes = [_vp, _i32, _vp, _vp, _vp, _vp, _i32, _i64, _i64, _i32, _i32, _vp, _vp, _vp, _vp]
        lib.gip_mesh_rast_db.restype = ctypes.c_int
        lib.gip_mesh_rast_db.argtypes = [_vp, _vp, _i32, _i64, _i64, _i32, _i32, _vp, _vp, _vp]
        lib.gip_mesh_interpolate_da.restype = ctypes.c_int
        lib.gip_mesh_interpolate_da.argtypes = [_vp, _i32, _i64, _i32, _vp, _i64, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp]
        lib.gip_mesh_interpolate_da_backward.restype = ctypes.c_int
        lib.gip_mesh_interpolate_da_backward.argtypes = [_vp, _i32, _i64, _i32, _vp, _i64, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp]
        lib.gip_mesh_mip_levels.restype = ctypes.c_int
        lib.gip_mesh_mip_levels.argtypes = [_i32, _i32, _i32, ctypes.POINTER(_i32), ctypes.POINTER(_i64)]
        lib.gip_mesh_mip_build.restype = ctypes.c_int
        lib.gip_mesh_mip_build.argtypes = [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _i64, _vp]
        lib.gip_mesh_mip_fold.restype = ctypes.c_int
        lib.gip_mesh_mip_fold.argtypes = [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _i64, _vp]
        lib.gip_mesh_texture_mip.restype = ctypes.c_int
        lib.gip_mesh_texture_mip.argtypes = [_vp, _i32, _i32, _i32, _i32, _vp, _i64, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp]
        lib.gip_mesh_texture_mip_backward.restype = ctypes.c_int
        lib.gip_mesh_texture_mip_backward.argtypes = [_vp, _i32, _i32, _i32, _i32, _vp, _i64, _i32, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _i32,
                                                      _vp, _vp, _vp, _vp, _vp, _vp]
        _f32 = ctypes.c_float
        lib.gip_mesh_components_rounds.restype = ctypes.c_int
        lib.gip_mesh_components_rounds.argtypes = [_vp, _i64, _i64, _vp, _vp, _i32, _vp]
        lib.gip_mesh_component_stats.restype = ctypes.c_int
        lib.gip_mesh_component_stats.argtypes = [_vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp]
        lib.gip_mesh_cluster_keys.restype = ctypes.c_int
        lib.gip_mesh_cluster_keys.argtypes = [_vp, _i64, _f32, _f32, _f32, _f32, _i32, _vp, _vp]
        lib.gip_mesh_cluster_count.restype = ctypes.c_int
        lib.gip_mesh_cluster_count.argtypes = [_vp, _i64, _vp, _i64, _f32, _f32, _f32, _f32, _i32, _vp, _vp]
        lib.gip_mesh_cluster_place.restype = ctypes.c_int
        lib.gip_mesh_cluster_place.argtypes = [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _f32, _f32, _f32, _f32, _i32, _i32, _vp, _vp]
        _sz = ctypes.c_size_t
        lib.gip_mesh_geometry_workspace_size.restype = ctypes.c_int
        lib.gip_mesh_geometry_workspace_size.argtypes = [_i64, ctypes.POINTER(_sz)]
        lib.gip_mesh_vertex_normals.restype = ctypes.c_int
        lib.gip_mesh_vertex_normals.argtypes = [_vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp]
        lib.gip_mesh_vertex_normals_backward.restype = ctypes.c_int
        lib.gip_mesh_vertex_normals_backward.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp]
        lib.gip_mesh_laplacian_loss.restype = ctypes.c_int
        lib.gip_mesh_laplacian_loss.argtypes = [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _sz, _vp]
        lib.gip_mesh_laplacian_loss_backward.restype = ctypes.c_int
        lib.gip_mesh_laplacian_loss_backward.argtypes = [_vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp]
        lib.gip_mesh_normal_consistency.restype = ctypes.c_int
        lib.gip_mesh_normal_consistency.argtypes = [_vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _sz, _vp]
        lib.gip_mesh_normal_consistency_backward.restype = ctypes.c_int
        lib.gip_mesh_normal_consistency_backward.argtypes = [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp]
        lib.gip_uv_face_classes.restype = ctypes.c_int
        lib.gip_uv_face_classes.argtypes = [_vp, _vp, _vp, _i64, _i64, _i32, _f32, _vp, _vp, _vp, _vp, _vp]
        lib.gip_uv_chart_rounds.restype = ctypes.c_int
        lib.gip_uv_chart_rounds.argtypes = [_vp, _vp, _i64, _vp, _vp, _i32, _vp]
        lib.gip_uv_chart_boxes.restype = ctypes.c_int
        lib.gip_uv_chart_boxes.argtypes = [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp]
        lib.gip_uv_place.restype = ctypes.c_int
        lib.gip_uv_place.argtypes = [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _f32, _i32, _vp, _vp]
        lib.gip_uv_vertex_tangents.restype = ctypes.c_int
        lib.gip_uv_vertex_tangents.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _vp]
        lib.gip_uv_vertex_tangents_backward.restype = ctypes.c_int
        lib.gip_uv_vertex_tangents_backward.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp]
        lib.gip_texture_dilate.restype = ctypes.c_int
        lib.gip_texture_dilate.argtypes = [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp]
        lib.gip_tet_workspace_size.restype = ctypes.c_int
        lib.gip_tet_workspace_size.argtypes = [_i64, ctypes.POINTER(_sz)]
        lib.gip_tet_mark.restype = ctypes.c_int
        lib.gip_tet_mark.argtypes = [_vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp]
        lib.gip_tet_emit.restype = ctypes.c_int
        lib.gip_tet_emit.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp]
        lib.gip_tet_backward.restype = ctypes.c_int
        lib.gip_tet_backward.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _vp]
        lib.gip_tet_sdf_diff.restype = ctypes.c_int
        lib.gip_tet_sdf_diff.argtypes = [_vp, _vp, _i64, _i64, _vp, _vp, _vp, _sz, _vp]
        lib.gip_tet_sdf_diff_backward.restype = ctypes.c_int
        lib.gip_tet_sdf_diff_backward.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp]
        _levels = [_vp] * 5 + [_i64, _i32, _i32, _i64]        # the level table's five host arrays, then N, L, F, P
        lib.gip_hashgrid_forward.restype = ctypes.c_int
        lib.gip_hashgrid_forward.argtypes = [_vp, _vp] + _levels + [_vp, _vp]
        lib.gip_hashgrid_backward_input.restype = ctypes.c_int
        lib.gip_hashgrid_backward_input.argtypes = [_vp, _vp, _vp] + _levels + [_vp, _vp]
        lib.gip_hashgrid_backward_table.restype = ctypes.c_int
        lib.gip_hashgrid_backward_table.argtypes = [_vp, _vp] + _levels + [_vp, _vp]
        _box = [_f32] * 9 + [_f32, _f32, _f32, _i32]          # lo, hi and scale per axis, then dt, near, far, K_cap
        lib.gip_volume_march_count.restype = ctypes.c_int
        lib.gip_volume_march_count.argtypes = [_vp, _vp, _vp, _vp, _i64, _i32] + _box + [_vp, _vp]
        lib.gip_volume_march_emit.restype = ctypes.c_int
        lib.gip_volume_march_emit.argtypes = [_vp, _vp, _vp, _vp, _i64, _i32] + _box + [_vp, _i64, _vp, _vp, _vp, _vp]
        lib.gip_volume_weights_forward.restype = ctypes.c_int
        lib.gip_volume_weights_forward.argtypes = [_vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp]
        lib.gip_volume_weights_backward.restype = ctypes.c_int
        lib.gip_volume_weights_backward.argtypes = [_vp] * 7 + [_i64, _i64, _vp, _vp]
        lib.gip_volume_accumulate_forward.restype = ctypes.c_int
        lib.gip_volume_accumulate_forward.argtypes = [_vp, _vp, _vp, _i64, _i64, _i32, _vp, _vp]
        lib.gip_volume_accumulate_backward.restype = ctypes.c_int
        lib.gip_volume_accumulate_backward.argtypes = [_vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _vp, _vp]
        lib.gip_volume_alpha_weights_forward.restype = ctypes.c_int
        lib.gip_volume_alpha_weights_forward.argtypes = [_vp, _vp, _i64, _i64, _vp, _vp, _vp]
        lib.gip_volume_alpha_weights_backward.restype = ctypes.c_int
        lib.gip_volume_alpha_weights_backward.argtypes = [_vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp]
        _sdf = [_vp] * 8 + [_f32]                             # sdf, normals, rays_d, t_starts, t_ends, values, offsets, inv_std, then rho
        lib.gip_volume_sdf_render_forward.restype = ctypes.c_int
        lib.gip_volume_sdf_render_forward.argtypes = _sdf + [_i64, _i64, _i32, _vp, _vp, _vp, _vp, _vp]
        lib.gip_volume_sdf_render_backward.restype = ctypes.c_int
        lib.gip_volume_sdf_render_backward.argtypes = _sdf + [_vp] * 5 + [_i64, _i64, _i32, _vp, _vp, _vp, _vp, _vp]
        _model = _Counted(lib)
    return _model


def ptr(t):
    """The address of tensor t for a C-ABI call; null for None or an empty tensor."""
    return ctypes.c_void_p(t.data_ptr() if t is not None and t.numel() else None)


def _call(lib, name, args, dev=None, accept=()):
    """The one place the C-ABI protocol is spelled: entry point `name` of `lib` with args and, when dev is given, dev's current
    stream as its last argument; RuntimeError naming the entry point unless it returns 0 or a status in `accept`.  Returns the status."""
    if dev is not None:
        import torch
        args += (ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream),)
    rc = getattr(lib, name)(*args)
    if rc != 0 and rc not in accept:
        raise RuntimeError("%s failed with status %d" % (name, rc))
    return rc


def call_model(dev, name, *args):
    """libgip_model.so's entry point `name` with args and, as its last argument, dev's current stream; RuntimeError unless it returns 0."""
    import torch
    with torch.cuda.device(dev):
        _call(model_lib(), name, args, dev)


def call_knn(dev, name, *args):
    """libgip_knn.so's entry point `name`, same contract as call_model (dev selected, its current stream last)."""
    import torch
    with torch.cuda.device(dev):
        _call(knn_lib(), name, args, dev)


def query_model(name, *args):
    """An entry point of libgip_model.so that takes no stream and launches nothing (the *_workspace_size queries,
    gip_mesh_mip_levels): RuntimeError unless it returns 0."""
    _call(model_lib(), name, args)


def call_nn(dev, name, *args, accept=()):
    """libgip_nn.so's entry point `name` with args and, as its last argument, dev's current stream; RuntimeError unless it returns 0
    or a status in `accept` (one the caller handles itself); returns the status.
    Unlike call_model it does NOT select dev (no torch.cuda.device guard): the denoiser makes several hundred of these calls per
    eager step, also on side streams and under graph capture, its callers never switched devices around them, and what the guard
    would cost on that path has not been measured.  The caller runs with the tensors' device current."""
    return _call(nn_lib(), name, args, dev, accept)


_nn = None


def nn_lib():
    global _nn
    if _nn is None:
        path = os.path.join(LIB_DIR, os.environ.get("GIP_NN_LIB", "libgip_nn.so"))
        if not os.path.exists(path):
            raise _missing("libgip_nn.so")
        lib = ctypes.CDLL(path)
        lib.gip_gn_workspace_bytes.restype = ctypes.c_size_t
        lib.gip_gn_workspace_bytes.argtypes = [ctypes.c_int32, ctypes.c_int32]
        lib.gip_gn_silu_forward.restype = ctypes.c_int
        lib.gip_gn_silu_forward.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32,
                                            ctypes.c_int32, ctypes.c_float, ctypes.c_int32, _vp, ctypes.c_int32, _vp,
                                            ctypes.c_size_t, _vp]
        lib.gip_gn_silu_backward.restype = ctypes.c_int
        lib.gip_gn_silu_backward.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_int32, ctypes.c_int64,
                                             ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _vp, ctypes.c_int32, _vp,
                                             ctypes.c_size_t, _vp]
        lib.gip_gn_silu_backward_accum.restype = ctypes.c_int
        lib.gip_gn_silu_backward_accum.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_int32, ctypes.c_int64,
                                                   ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _vp, ctypes.c_int32, _vp, _vp,
                                                   ctypes.c_size_t, _vp]
        lib.gip_conv3x3s2_dgrad_nhwc_f16.restype = ctypes.c_int
        lib.gip_conv3x3s2_dgrad_nhwc_f16.argtypes = [_vp, _vp, _vp] + [ctypes.c_int32] * 5 + [_vp]
        lib.gip_upsample2x_conv3x3_nhwc_f16.restype = ctypes.c_int
        lib.gip_upsample2x_conv3x3_nhwc_f16.argtypes = [_vp, _vp, _vp, _vp] + [ctypes.c_int32] * 5 + [_vp]
        lib.gip_winograd_input_f16.restype = ctypes.c_int
        lib.gip_winograd_input_f16.argtypes = [_vp, _vp] + [ctypes.c_int32] * 4 + [_vp]
        lib.gip_winograd_output_f16.restype = ctypes.c_int
        lib.gip_winograd_output_f16.argtypes = [_vp, _vp, _vp, _vp] + [ctypes.c_int32] * 4 + [_vp]
        lib.gip_winograd_output_stats_f16.restype = ctypes.c_int
        lib.gip_winograd_output_stats_f16.argtypes = [_vp, _vp, _vp, _vp, _vp] + [ctypes.c_int32] * 4 + [_vp]
        lib.gip_conv3x3_fewch_nhwc_f16.restype = ctypes.c_int
        lib.gip_conv3x3_fewch_nhwc_f16.argtypes = [_vp, _vp, _vp, _vp] + [ctypes.c_int32] * 7 + [_vp]
        lib.gip_conv3x3_c3_fwd_stats_nhwc_f16.restype = ctypes.c_int
        lib.gip_conv3x3_c3_fwd_stats_nhwc_f16.argtypes = [_vp, _vp, _vp, _vp] + [ctypes.c_int32] * 4 + [_vp, _vp]
        lib.gip_conv3x3_c3_fwd_nhwc_f16.restype = ctypes.c_int
        lib.gip_conv3x3_c3_fwd_nhwc_f16.argtypes = [_vp, _vp, _vp, _vp] + [ctypes.c_int32] * 4 + [_vp]
        lib.gip_conv3x3_c3_dgrad_nhwc_f16.restype = ctypes.c_int
        lib.gip_conv3x3_c3_dgrad_nhwc_f16.argtypes = [_vp, _vp, _vp] + [ctypes.c_int32] * 4 + [_vp]
        lib.gip_gn_silu_backward_sums.restype = ctypes.c_int
        lib.gip_gn_silu_backward_sums.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_int32, ctypes.c_int64,
                                                  ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _vp, ctypes.c_int32, _vp, _vp,
                                                  ctypes.c_int32, _vp, ctypes.c_size_t, _vp]
        lib.gip_conv3x3_gnbwd_nhwc_f16.restype = ctypes.c_int
        lib.gip_conv3x3_gnbwd_nhwc_f16.argtypes = [_vp, _vp, _vp] + [ctypes.c_int32] * 5 + [_vp, _vp, _vp, _vp, _vp, ctypes.c_int32,
                                                   ctypes.c_int32, _vp, ctypes.c_int32, _vp, _vp]
        lib.gip_gn_silu_forward_stats.restype = ctypes.c_int
        lib.gip_gn_silu_forward_stats.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32,
                                                  ctypes.c_int32, ctypes.c_float, ctypes.c_int32, _vp, ctypes.c_int32, _vp,
                                                  ctypes.c_int32, _vp]
        lib.gip_conv3x3_stats_nhwc_f16.restype = ctypes.c_int
        lib.gip_conv3x3_stats_nhwc_f16.argtypes = [_vp, _vp, _vp, _vp, _vp] + [ctypes.c_int32] * 5 + [_vp, _vp]
        lib.gip_conv3x3_stats_ws_nhwc_f16.restype = ctypes.c_int
        lib.gip_conv3x3_stats_ws_nhwc_f16.argtypes = [_vp, _vp, _vp, _vp, _vp] + [ctypes.c_int32] * 5 + [_vp, ctypes.c_int32, _vp, ctypes.c_size_t, _vp]
        lib.gip_linear_stats_f16.restype = ctypes.c_int
        lib.gip_linear_stats_f16.argtypes = [_vp, _vp, _vp, _vp, _vp, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, _vp, _vp]
        lib.gip_add_bias_residual.restype = ctypes.c_int
        lib.gip_add_bias_residual.argtypes = [_vp, _vp, _vp, _vp, ctypes.c_int64, ctypes.c_int32, _vp]
        lib.gip_geglu.restype = ctypes.c_int
        lib.gip_geglu.argtypes = [_vp, _vp, ctypes.c_int64, ctypes.c_int32, _vp]
        lib.gip_cat2_stats_f16.restype = ctypes.c_int
        lib.gip_cat2_stats_f16.argtypes = [_vp, _vp, _vp, _vp, _vp, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, _vp]
        lib.gip_layernorm_f16.restype = ctypes.c_int
        lib.gip_layernorm_f16.argtypes = [_vp, _vp, _vp, _vp, ctypes.c_int64, ctypes.c_int32, ctypes.c_float, _vp]
        lib.gip_lpips_layer_blocks.restype = ctypes.c_int32
        lib.gip_lpips_layer_blocks.argtypes = [ctypes.c_int32, ctypes.c_int64]
        lib.gip_lpips_layer_forward.restype = ctypes.c_int
        lib.gip_lpips_layer_forward.argtypes = [_vp, _vp, _vp, _vp, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, _vp]
        lib.gip_lpips_layer_backward.restype = ctypes.c_int
        lib.gip_lpips_layer_backward.argtypes = [_vp, _vp, _vp, _vp, _vp, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, _vp]
        lib.gip_attention_fwd_strided2_f16.restype = ctypes.c_int
        lib.gip_attention_fwd_strided2_f16.argtypes = [_vp, _vp, _vp, _vp] + [ctypes.c_int32] * 5 + [ctypes.c_float, _vp, _vp, ctypes.c_int32,
                                                       ctypes.c_float, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _vp]
        lib.gip_attention_variant.restype = ctypes.c_int
        lib.gip_attention_variant.argtypes = [ctypes.c_int32] * 6
        lib.gip_attention_fwd_f16.restype = ctypes.c_int
        lib.gip_attention_fwd_f16.argtypes = [_vp, _vp, _vp, _vp] + [ctypes.c_int32] * 5 + [ctypes.c_float, _vp, _vp, ctypes.c_int32, ctypes.c_float, _vp]
        lib.gip_attention_fwd_strided_f16.restype = ctypes.c_int
        lib.gip_attention_fwd_strided_f16.argtypes = [_vp, _vp, _vp, _vp] + [ctypes.c_int32] * 5 + [ctypes.c_float, _vp, _vp, ctypes.c_int32, ctypes.c_float, ctypes.c_int32, ctypes.c_int32, _vp]
        lib.gip_conv3x3s2_stats_nhwc_f16.restype = ctypes.c_int
        lib.gip_conv3x3s2_stats_nhwc_f16.argtypes = [_vp, _vp, _vp, _vp] + [ctypes.c_int32] * 7 + [_vp, _vp]
        lib.gip_conv3x3s2_nhwc_f16.restype = ctypes.c_int
        lib.gip_conv3x3s2_nhwc_f16.argtypes = [_vp, _vp, _vp, _vp] + [ctypes.c_int32] * 7 + [_vp, ctypes.c_size_t, _vp]
        lib.gip_linear_row_parts.restype = ctypes.c_int32
        lib.gip_linear_row_parts.argtypes = [ctypes.c_int64, ctypes.c_int32]
        lib.gip_linear_rows_f16.restype = ctypes.c_int
        lib.gip_linear_rows_f16.argtypes = [_vp, _vp, _vp, _vp, _vp, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, _vp, _vp]
        lib.gip_linear_ln_f16.restype = ctypes.c_int
        lib.gip_linear_ln_f16.argtypes = [_vp, _vp, _vp, _vp, _vp, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _vp,
                                          ctypes.c_int32, ctypes.c_float, _vp]
        lib.gip_linear_f16.restype = ctypes.c_int
        lib.gip_linear_f16.argtypes = [_vp, _vp, _vp, _vp, _vp, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _vp]
        lib.gip_conv3x3_nhwc_f16.restype = ctypes.c_int
        lib.gip_conv3x3_nhwc_f16.argtypes = [_vp, _vp, _vp, _vp, _vp] + [ctypes.c_int32] * 5 + [_vp, ctypes.c_size_t, _vp]
        _i64p = ctypes.POINTER(ctypes.c_int64)
        lib.gip_image_prep_f16.restype = ctypes.c_int
        lib.gip_image_prep_f16.argtypes = [_vp] + [ctypes.c_int32] * 4 + [_vp, _vp]
        lib.gip_image_prep_backward_f16.restype = ctypes.c_int
        lib.gip_image_prep_backward_f16.argtypes = [_vp] + [ctypes.c_int32] * 4 + [_vp, _vp]
        lib.gip_latent_sample_f16.restype = ctypes.c_int
        lib.gip_latent_sample_f16.argtypes = [_vp, _i64p, _vp, _vp, _vp, _vp, ctypes.c_float] + [ctypes.c_int32] * 5 + [_vp, _vp, _vp]
        lib.gip_latent_sample_backward_f16.restype = ctypes.c_int
        lib.gip_latent_sample_backward_f16.argtypes = [_vp, _i64p, _vp, _vp, ctypes.c_float] + [ctypes.c_int32] * 4 + [_vp, _vp]
        lib.gip_anpg_loss_f16.restype = ctypes.c_int
        lib.gip_anpg_loss_f16.argtypes = [_vp, _i64p, _vp, _i64p, _vp, _vp] + [ctypes.c_int32] * 4 + [ctypes.c_float, ctypes.c_int32,
                                          ctypes.c_int32, ctypes.c_float, _vp, _vp, _vp, _vp, _vp]
        lib.gip_timestep_embedding_f16.restype = ctypes.c_int
        lib.gip_timestep_embedding_f16.argtypes = [_vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_float, _vp, _vp]
        lib.gip_winograd_input_gn_f16.restype = ctypes.c_int
        lib.gip_winograd_input_gn_f16.argtypes = [_vp, _vp] + [ctypes.c_int32] * 4 + [_vp, _vp, _vp, _vp, ctypes.c_int32, ctypes.c_int32, _vp,
                                                  ctypes.c_int32, _vp]
        lib.gip_gn_stats_from_partials.restype = ctypes.c_int
        lib.gip_gn_stats_from_partials.argtypes = [_vp, _vp, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_float,
                                                   _vp, ctypes.c_int32, _vp, ctypes.c_int32, _vp]
        lib.gip_conv3x3_gnin_nhwc_f16.restype = ctypes.c_int
        lib.gip_conv3x3_gnin_nhwc_f16.argtypes = [_vp, _vp, _vp, _vp, _vp] + [ctypes.c_int32] * 5 + [_vp, _vp, _vp, _vp, ctypes.c_int32,
                                                  ctypes.c_int32, _vp, ctypes.c_int32, _vp, _vp]
        lib.gip_linear_batched_f16.restype = ctypes.c_int
        lib.gip_linear_batched_f16.argtypes = [_vp, _vp, _vp, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32,
                                               ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, _vp]
        lib.gip_softmax_rows_f16.restype = ctypes.c_int
        lib.gip_softmax_rows_f16.argtypes = [_vp, ctypes.c_int64, ctypes.c_int32, ctypes.c_float, _vp]
        lib.gip_softmax_rows_backward_f16.restype = ctypes.c_int
        lib.gip_softmax_rows_backward_f16.argtypes = [_vp, _vp, ctypes.c_int64, ctypes.c_int32, ctypes.c_float, _vp]
        lib.gip_scale_cast_f16.restype = ctypes.c_int
        lib.gip_scale_cast_f16.argtypes = [_vp, _vp, ctypes.c_float, _vp, ctypes.c_int64, _vp]
        _nn = _Counted(lib)
    return _nn


def status_string(rc):
    return raster_lib().gip_status_string(int(rc)).decode()


RASTER_SYMBOLS = ["gip_abi_version", "gip_status_string", "gip_raster_state_bytes", "gip_raster_scratch_bytes",
                  "gip_raster_state_layout", "gip_raster_forward", "gip_raster_backward", "gip_raster_read_header",
                  "gip_raster_mark_visible", "gip_raster_forward_profiled", "gip_raster_backward_profiled",
                  "gip_raster_state_bytes_buckets", "gip_raster_state_layout_buckets", "gip_raster_forward_buckets",
                  "gip_raster_backward_buckets", "gip_raster_forward_buckets_profiled", "gip_raster_backward_buckets_profiled"]
FIELD_SYMBOLS = ["gip_field_workspace_size", "gip_density_field", "gip_surface_count", "gip_surface_emit"]
SAMPLE_SYMBOLS = ["gip_field_sample_workspace_size", "gip_field_sample"]
TEXTURE_SYMBOLS = ["gip_texture_bake_workspace_size", "gip_texture_bake"]
TEXTURE_PROJECT_SYMBOLS = ["gip_texture_project"]
MESH_SYMBOLS = ["gip_mesh_raster_workspace_size", "gip_mesh_rasterize", "gip_mesh_interpolate", "gip_mesh_interpolate_backward",
                "gip_mesh_texture", "gip_mesh_texture_backward", "gip_mesh_shade", "gip_mesh_shade_backward"]
MESH_GRAD_SYMBOLS = ["gip_mesh_rasterize_backward", "gip_mesh_interpolate_backward_rast", "gip_mesh_shade_backward_rast", "gip_mesh_antialias",
                     "gip_mesh_antialias_backward"]
MESH_MIP_SYMBOLS = ["gip_mesh_rast_db", "gip_mesh_interpolate_da", "gip_mesh_interpolate_da_backward", "gip_mesh_mip_levels",
                    "gip_mesh_mip_build", "gip_mesh_mip_fold", "gip_mesh_texture_mip", "gip_mesh_texture_mip_backward"]
MESH_CLEAN_SYMBOLS = ["gip_mesh_components_rounds", "gip_mesh_component_stats", "gip_mesh_cluster_keys", "gip_mesh_cluster_count",
                      "gip_mesh_cluster_place"]
MESH_GEOM_SYMBOLS = ["gip_mesh_geometry_workspace_size", "gip_mesh_vertex_normals", "gip_mesh_vertex_normals_backward",
                     "gip_mesh_laplacian_loss", "gip_mesh_laplacian_loss_backward", "gip_mesh_normal_consistency",
                     "gip_mesh_normal_consistency_backward"]
MESH_UV_SYMBOLS = ["gip_uv_face_classes", "gip_uv_chart_rounds", "gip_uv_chart_boxes", "gip_uv_place", "gip_uv_vertex_tangents",
                   "gip_uv_vertex_tangents_backward", "gip_texture_dilate"]
MESH_TET_SYMBOLS = ["gip_tet_workspace_size", "gip_tet_mark", "gip_tet_emit", "gip_tet_backward", "gip_tet_sdf_diff",
                    "gip_tet_sdf_diff_backward"]
HASHGRID_SYMBOLS = ["gip_hashgrid_forward", "gip_hashgrid_backward_input", "gip_hashgrid_backward_table"]
VOLUME_SYMBOLS = ["gip_volume_march_count", "gip_volume_march_emit", "gip_volume_weights_forward", "gip_volume_weights_backward",
                  "gip_volume_accumulate_forward", "gip_volume_accumulate_backward"]
VOLUME_SDF_SYMBOLS = ["gip_volume_alpha_weights_forward", "gip_volume_alpha_weights_backward", "gip_volume_sdf_render_forward",
                      "gip_volume_sdf_render_backward"]
