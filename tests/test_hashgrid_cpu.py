"""The hash-grid encoding without a GPU (csrc/hashgrid.hip, gaussianip_amd/utils/encoding.py): the level table, the float64 restatement's
analytic gradients against central differences, the float32 op chain against the restatement, the progressive mask, the factories'
argument handling, the exported symbols, the entry points' argument checks (which launch nothing) and the compiler's resource report of
every kernel of the file."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import hashgrid_inputs as inputs
import hashgrid_reference as reference
from test_model_no_spills_cpu import HIPCC, resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = tuple("%s_kernelILi%dE" % (k, F) for k in ("hashgrid_forward", "hashgrid_backward_input", "hashgrid_backward_table")
                for F in (1, 2, 4, 8))


def test_symbols_exported():
    from gaussianip_amd import _lib
    from gaussianip_amd.utils import encoding, isosurface, rasterize
    so = os.path.join(ROOT, "gaussianip_amd", "lib", "libgip_model.so")
    assert os.path.exists(so), "libgip_model.so is not built"
    names = {ln.split()[-1] for ln in subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout.splitlines()
             if ln.strip()}
    lib = _lib.model_lib()
    with open(os.path.join(ROOT, "include", "gip_model.h")) as fh:
        header = fh.read()
    assert _lib.HASHGRID_SYMBOLS == ["gip_hashgrid_forward", "gip_hashgrid_backward_input", "gip_hashgrid_backward_table"]
    for sym in _lib.HASHGRID_SYMBOLS:
        assert sym in names and getattr(lib, sym) is not None and "int %s(" % sym in header, sym
    with open(os.path.join(ROOT, "gaussianip_amd", "csrc", "Makefile")) as fh:
        assert fh.read().count("hashgrid.hip") == 2                  # a prerequisite of libgip_model.so and a source of its command
    assert encoding.__all__ == ["HashGridLayout", "hash_grid_encode", "HashGridEncoding", "ProgressiveBandHashGrid",
                                "ProgressiveBandFrequency", "CompositeEncoding", "VanillaMLP", "get_encoding", "get_mlp", "get_activation"]
    assert "render_field_mesh" in rasterize.__all__ and callable(rasterize.render_field_mesh)
    assert callable(isosurface.TetrahedraSDFGrid.forward)


def test_layout_tables():
    from gaussianip_amd.utils.encoding import HashGridLayout
    a = inputs.layout("a")
    # exp2f(l * log2f(1.5)) is not exactly 1.5^l: a few units in the last place of float32
    assert a.scales.dtype == np.float32 and np.abs(a.scales / np.array([3.0, 5.0, 8.0, 12.5, 19.25, 29.375]) - 1).max() < 4 * 2.0 ** -23
    assert a.resolutions == [4, 6, 9, 14, 21, 31]
    assert a.sizes == [64, 216, 736, 1024, 1024, 1024] and a.offsets == [0, 64, 280, 1016, 2040, 3064]
    assert a.hashed == [False, False, False, True, True, True]
    assert a.n_rows == 4088 and a.n_params == 8176 and a.n_output_dims == 12
    c = inputs.layout("c")
    # the definition, restated with Python integers and numpy float32
    scale = np.float32(16)
    ratio = np.log2(np.float32(1.447269237440378))
    total = 0
    for l in range(16):
        s = np.exp2(np.float32(l) * ratio) * np.float32(16) - np.float32(1)
        assert s.dtype == np.float32 and c.scales[l] == s
        res = int(np.ceil(s)) + 1
        size = min((res ** 3 + 7) // 8 * 8, 2 ** 19)
        assert (c.resolutions[l], c.sizes[l], c.offsets[l], c.hashed[l]) == (res, size, total, res ** 3 > size), l
        total += size
    assert scale == 16 and c.resolutions[0] == 16 and c.sizes[0] == 4096 and not c.hashed[0]
    assert abs(float(c.scales[15]) - 4095.0) < 0.5 and c.resolutions[15] in (4096, 4097)
    assert c.hashed == [False] * 5 + [True] * 11                    # 16, 24, 34, 49, 70 nodes a side fit 2^19 rows; 101 do not
    assert c.n_rows == total and c.n_params == 2 * total and c.n_output_dims == 32
    assert all(s % 8 == 0 for s in c.sizes)
    # a cube far above 2^64 is simply too large; the limits
    big = HashGridLayout(dict(inputs.CONFIG_A, n_levels=32, per_level_scale=1.5, base_resolution=16))
    assert big.hashed[-1] and big.sizes[-1] == 1024 and big.resolutions[-1] ** 3 > 2 ** 64
    for wrong in (dict(n_levels=0), dict(n_levels=33), dict(n_features_per_level=3), dict(log2_hashmap_size=25), dict(base_resolution=0),
                  dict(per_level_scale=0.0), dict(per_level_scale=3.0, n_levels=32, base_resolution=64), dict(interpolation="Nearest")):
        with pytest.raises(ValueError):
            HashGridLayout(dict(inputs.CONFIG_A, **wrong))
    with pytest.raises(ValueError, match="n_levels"):
        HashGridLayout({"n_features_per_level": 2})


def test_inputs():
    for name in inputs.CASES:
        cfg, x, table, g = inputs.case(name)
        lay = inputs.layout(name)
        assert x.dtype == table.dtype == g.dtype == np.float32 and x.shape[1] == 3
        assert table.shape == (lay.n_rows, lay.n_features_per_level) and g.shape == (x.shape[0], lay.n_output_dims)
        assert inputs.case(name)[1] is x and not x.flags.writeable
    _, x, _, g = inputs.case("d")
    lay = inputs.layout("d")
    assert (x[inputs.D_ZERO] == 0).any(1).all() and (x[inputs.D_ONE] == 1).any(1).all()
    on_node = 0
    for l in range(lay.n_levels):
        _, frac, valid = reference.level_cells(x[inputs.D_NODES], lay.scales[l])
        on_node += int(((frac == 0) & valid[:, None]).all(1).sum())
        _, _, valid = reference.level_cells(x[inputs.D_NONFINITE], lay.scales[l])
        assert not valid.any()
        cell, _, valid = reference.level_cells(x[inputs.D_OUTSIDE], lay.scales[l])
        assert valid.all() and (cell < 0).any() and (cell >= lay.resolutions[l]).any()
    assert on_node >= 8                                               # points with frac == 0 on all three axes of some level
    assert (x[inputs.D_COPIES] == x[inputs.D_COPIES.start]).all() and (g[inputs.D_COPIES] == g[inputs.D_COPIES.start]).all()
    assert x[inputs.D_COPIES].shape[0] == 64


def test_analytic_gradients_against_central_differences():
    """Inside a cell the encoding is linear in every coordinate and in every table entry, so a central difference is exact up to
    rounding.  Per level: the points are moved to the middle of their cells on that level (pos = cell + 0.5), the upstream gradient is
    kept on that level's columns, and the step is a quarter of a cell.  The position's own float32 rounding (an ulp of pos, at most
    2^-19 below 32) over the step of 0.5 cells bounds the difference by 4e-6 of the gradient's scale; 1e-4 is asked."""
    cfg, x, table, g = inputs.case("a")
    lay = inputs.layout("a")
    x, g = x[:200], g[:200].astype(np.float64)
    F = lay.n_features_per_level
    for l in range(lay.n_levels):
        s = float(lay.scales[l])
        cell, _, _ = reference.level_cells(x, lay.scales[l])
        xm = (cell / s).astype(np.float32)                            # pos = cell + 0.5
        _, frac, valid = reference.level_cells(xm, lay.scales[l])
        assert valid.all() and np.abs(frac - 0.5).max() < 1e-3
        gl = np.zeros_like(g)
        gl[:, l * F:(l + 1) * F] = g[:, l * F:(l + 1) * F]
        g_x, g_table = reference.backward_f64(xm, table, gl, lay)
        h = np.float32(0.25 / s)
        for axis in range(3):
            step = np.zeros(3, np.float32)
            step[axis] = h
            hi, lo = (xm + step).astype(np.float32), (xm - step).astype(np.float32)
            fd = ((reference.encode_f64(hi, table, lay) - reference.encode_f64(lo, table, lay)) * gl).sum(1) / (
                hi[:, axis].astype(np.float64) - lo[:, axis].astype(np.float64))
            assert np.abs(fd - g_x[:, axis]).max() <= 1e-4 * np.abs(g_x).max(), (l, axis)
        # the table: a handful of touched entries and one untouched level
        rng = np.random.default_rng(l)
        touched = np.argwhere(g_table != 0)
        assert touched.shape[0] > 0 and (touched[:, 0] >= lay.offsets[l]).all() and (touched[:, 0] < lay.offsets[l] + lay.sizes[l]).all()
        base = (reference.encode_f64(xm, table, lay) * gl).sum()
        for r, f in touched[rng.integers(0, touched.shape[0], 6)]:
            bumped = table.astype(np.float64)
            bumped[r, f] += 0.5
            fd = ((reference.encode_f64(xm, bumped, lay) * gl).sum() - base) / 0.5
            assert abs(fd - g_table[r, f]) <= 1e-9 * max(1.0, abs(g_table[r, f])), (l, r, f)


@pytest.mark.parametrize("name", ["a", "b_f1_n65", "b_f4_n63", "b_f8_n65", "d", "e_n1", "e_n0"])
def test_op_chain_against_the_restatement(name):
    cfg, x, table, g = inputs.case(name)
    lay = inputs.layout(name)
    ref = reference.encode_f64(x, table, lay)
    ref_gx, ref_gt = reference.backward_f64(x, table, g, lay)
    assert np.isfinite(ref).all() and np.isfinite(ref_gx).all() and np.isfinite(ref_gt).all()
    # in float64 the chain is the restatement up to the order of its sums, with g_x rounded once to x's float32; in float32 a row sums up
    # to 8 corners x 1000 points and a gradient to x 12 columns x 8 corners, each term rounded to 2^-24
    for dtype, bar in ((torch.float64, 1e-13), (torch.float32, 2e-5)):
        xt = torch.from_numpy(x.copy()).requires_grad_(True)
        tt = torch.from_numpy(table.copy()).to(dtype).requires_grad_(True)
        enc = reference.op_chain(xt, tt, lay)
        assert enc.dtype == dtype and tuple(enc.shape) == ref.shape
        if x.shape[0] == 0:
            continue
        gx, gt = torch.autograd.grad((enc * torch.from_numpy(g.copy()).to(dtype)).sum(), (xt, tt))
        for got, want, what in ((enc.detach(), ref, "enc"), (gx, ref_gx, "g_x"), (gt, ref_gt, "g_table")):
            got = got.double().numpy()
            assert np.isfinite(got).all(), (name, what)
            limit = 2.0 ** -24 if (what, dtype) == ("g_x", torch.float64) else bar
            assert np.abs(got - want).max() <= limit * np.abs(want).max(), (name, what, dtype)
    if name == "d":
        assert not ref[inputs.D_NONFINITE].any() and not ref_gx[inputs.D_NONFINITE].any() and ref[inputs.D_OUTSIDE].all(1).all()


def test_progressive_band_masks():
    from gaussianip_amd.utils.encoding import ProgressiveBandFrequency, ProgressiveBandHashGrid
    cfg = dict(inputs.CONFIG_A, otype="ProgressiveBandHashGrid", start_level=2, start_step=100, update_steps=50)
    enc = ProgressiveBandHashGrid(3, cfg)
    assert enc.n_input_dims == 3 and enc.n_output_dims == 12 and not enc.mask.any() and enc.current_level == 2
    assert [n for n, _ in enc.named_parameters()] == ["encoding.params"] and "mask" not in enc.state_dict()
    for step in (0, 100, 149, 150, 275, 10 ** 6):
        enc.update_step(0, step)
        level = min(2 + max(step - 100, 0) // 50, 6)
        assert enc.current_level == level
        assert enc.mask.tolist() == [1.0] * (2 * level) + [0.0] * (12 - 2 * level), step
    with pytest.raises(ValueError, match="start_level"):
        ProgressiveBandHashGrid(3, dict(inputs.CONFIG_A))
    freq = ProgressiveBandFrequency(3, {"n_frequencies": 4, "n_masking_step": 100})
    assert freq.n_output_dims == 24 and freq.mask.tolist() == [1.0] * 4
    freq.update_step(0, 30)
    want = (1.0 - torch.cos(np.pi * (30 / 100 * 4 - torch.arange(0, 4)).clamp(0, 1))) / 2.0
    assert torch.equal(freq.mask, want) and want[0] == 1 and 0 < want[1] < 1 and want[3] == 0
    x = torch.rand(5, 3)
    out = freq(x)
    assert out.shape == (5, 24) and torch.allclose(out[:, :3], torch.sin(x)) and torch.allclose(out[:, 9:12], torch.cos(2 * x) * want[1])
    assert not out[:, 18:].any()


def test_factories_and_arguments():
    from gaussianip_amd.utils import encoding as E
    from gaussianip_amd.utils.isosurface import TetrahedraSDFGrid
    enc = E.get_encoding(3, dict(inputs.CONFIG_A))
    assert isinstance(enc, E.CompositeEncoding) and isinstance(enc.encoding, E.HashGridEncoding) and enc.n_output_dims == 12
    assert enc.encoding.n_input_dims == 3 and enc.encoding.params.shape == (8176,) and enc.encoding.params.dtype == torch.float32
    assert float(enc.encoding.params.detach().abs().max()) <= 1e-4 and float(enc.encoding.params.detach().std()) > 3e-5
    assert E.get_encoding(3, dict(inputs.CONFIG_A, include_xyz=True)).n_output_dims == 15
    assert isinstance(E.get_encoding(3, dict(inputs.CONFIG_A, otype="Grid", type="Hash")).encoding, E.HashGridEncoding)
    assert isinstance(E.get_encoding(3, {"otype": "ProgressiveBandFrequency", "n_frequencies": 6}).encoding, E.ProgressiveBandFrequency)
    with pytest.raises(ValueError, match="HashGrid, ProgressiveBandHashGrid, ProgressiveBandFrequency"):
        E.get_encoding(3, {"otype": "SphericalHarmonics"})
    with pytest.raises(ValueError, match="three input dimensions"):
        E.get_encoding(2, dict(inputs.CONFIG_A))
    with pytest.raises(ValueError, match="dict"):
        E.get_encoding(3, "HashGrid")
    mlp = E.get_mlp(12, 3, {"otype": "VanillaMLP", "activation": "ReLU", "output_activation": "none", "n_neurons": 64, "n_hidden_layers": 1})
    assert [tuple(p.shape) for p in mlp.parameters()] == [(64, 12), (3, 64)]
    deep = E.get_mlp(12, 3, {"otype": "VanillaMLP", "output_activation": "sigmoid", "n_neurons": 16, "n_hidden_layers": 3})
    assert [tuple(p.shape) for p in deep.parameters()] == [(16, 12), (16, 16), (16, 16), (3, 16)]
    x = torch.randn(7, 12)
    y = x
    for layer in list(deep.layers)[::2]:
        y = torch.relu(y @ layer.weight.t()) if layer is not deep.layers[-1] else y @ layer.weight.t()
    assert torch.allclose(deep(x), torch.sigmoid(y), atol=1e-6)
    with pytest.raises(ValueError, match="VanillaMLP"):
        E.get_mlp(12, 3, {"otype": "FullyFusedMLP", "n_neurons": 64, "n_hidden_layers": 1})
    with pytest.raises(ValueError, match="activation"):
        E.get_mlp(12, 3, {"otype": "VanillaMLP", "output_activation": "gelu6", "n_neurons": 64, "n_hidden_layers": 1})
    # the kernels have no CPU path
    lay = inputs.layout("a")
    with pytest.raises(ValueError, match="float32 GPU tensor"):
        E.hash_grid_encode(torch.rand(4, 3), torch.zeros(lay.n_rows, 2), lay)
    with pytest.raises(ValueError, match="HashGridLayout"):
        E.hash_grid_encode(torch.rand(4, 3), torch.zeros(lay.n_rows, 2), inputs.CONFIG_A)
    # the geometry: nothing by default, the reference's networks on request
    plain = TetrahedraSDFGrid(isosurface_resolution=4)
    assert sorted(n for n, _ in plain.named_parameters()) == ["deformation", "sdf"] and plain(torch.rand(3, 3)) == {}
    small = TetrahedraSDFGrid(isosurface_resolution=4, n_feature_dims=3, pos_encoding_config=dict(inputs.CONFIG_SMALL))
    assert sorted(n for n, _ in small.named_parameters()) == ["deformation", "encoding.encoding.params", "feature_network.layers.0.weight",
                                                              "feature_network.layers.2.weight", "sdf"]
    assert small.encoding.n_output_dims == 16 and tuple(small.feature_network.layers[0].weight.shape) == (64, 16)
    assert TetrahedraSDFGrid.POS_ENCODING_CONFIG == inputs.CONFIG_DEFAULT
    assert TetrahedraSDFGrid.MLP_NETWORK_CONFIG["n_neurons"] == 64 and TetrahedraSDFGrid.MLP_NETWORK_CONFIG["n_hidden_layers"] == 1


def test_argument_checks_launch_nothing():
    """Every check comes before the first launch, so these calls are safe on a machine without a GPU; `one` is a host address that a
    kernel would fault on."""
    from gaussianip_amd import _lib
    lib = _lib.model_lib()
    lay = inputs.layout("a")
    null = ctypes.c_void_p(None)
    buf = ctypes.create_string_buffer(64)
    one = ctypes.c_void_p(ctypes.addressof(buf))
    odd = ctypes.c_void_p(ctypes.addressof(buf) + 4)
    good = lay.level_args(5)
    assert len(good) == 9 and good[5:] == (5, 6, 2, 4088)

    def levels(N=5, L=6, F=2, P=4088, **arrays):
        """The level arguments with one of the five arrays, or a size, replaced; the arrays must outlive the call."""
        out = list(lay.level_args(N))
        for i, key in enumerate(("scale", "res", "size", "offset", "hashed")):
            if key in arrays:
                keep.append(arrays[key])
                out[i] = null if arrays[key] is None else ctypes.c_void_p(arrays[key].ctypes.data)
        out[5:] = [N, L, F, P]
        return out

    keep = []

    def all_three(lv):
        return (lib.gip_hashgrid_forward(one, one, *lv, one, null), lib.gip_hashgrid_backward_input(one, one, one, *lv, one, null),
                lib.gip_hashgrid_backward_table(one, one, *lv, one, null))

    scales, res, sizes = (np.array(a) for a in lay._arrays[:3])
    offsets = np.array(lay._arrays[3])
    bad_sizes, bad_sizes2, bad_res, bad_scale, bad_off = sizes.copy(), sizes.copy(), res.copy(), scales.copy(), offsets.copy()
    bad_sizes[2], bad_sizes2[5], bad_res[0], bad_scale[1], bad_off[3] = 0, 2 ** 24 + 8, 0, np.inf, 1000
    for lv in (levels(L=0), levels(L=33), levels(F=3), levels(F=16), levels(N=-1), levels(P=0), levels(P=4087), levels(P=4089),
               levels(N=2 ** 30), levels(N=2 ** 32 // (4 * 12) + 1), levels(scale=None), levels(res=None), levels(size=None),
               levels(offset=None), levels(hashed=None), levels(size=bad_sizes), levels(size=bad_sizes2), levels(res=bad_res),
               levels(scale=bad_scale), levels(offset=bad_off)):
        assert all_three(lv) == (1, 1, 1), lv[5:]
    # NULL and misaligned tensors
    lv = levels()
    assert lib.gip_hashgrid_forward(null, one, *lv, one, null) == 1 and lib.gip_hashgrid_forward(one, null, *lv, one, null) == 1
    assert lib.gip_hashgrid_forward(one, one, *lv, null, null) == 1 and lib.gip_hashgrid_forward(one, odd, *lv, one, null) == 1
    assert lib.gip_hashgrid_forward(one, one, *lv, odd, null) == 1
    assert lib.gip_hashgrid_backward_input(one, one, null, *lv, one, null) == 1
    assert lib.gip_hashgrid_backward_input(one, one, one, *lv, null, null) == 1
    assert lib.gip_hashgrid_backward_input(one, one, odd, *lv, one, null) == 1
    assert lib.gip_hashgrid_backward_table(one, null, *lv, one, null) == 1 and lib.gip_hashgrid_backward_table(one, one, *lv, null, null) == 1
    assert lib.gip_hashgrid_backward_table(null, one, *lv, one, null) == 1
    # no point: success, nothing launched or written, but the level table is still checked
    assert all_three(levels(N=0)) == (0, 0, 0)
    assert lib.gip_hashgrid_forward(null, null, *levels(N=0), null, null) == 0
    assert all_three(levels(N=0, F=3)) == (1, 1, 1)
    assert buf.raw == bytes(64)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_hashgrid_kernels_do_not_spill(tmp_path):
    scratch, spilled, log = resource_usage("hashgrid.hip", tmp_path / "o.o")
    for kernel in KERNELS:
        assert any(kernel in n for n in scratch), "no kernel-resource-usage remark for %s: %s" % (kernel, log[-500:])
    assert len(scratch) == len(KERNELS) == 12, sorted(scratch)
    bad = [(n, scratch[n], spilled.get(n, 0)) for n in scratch if scratch[n] or spilled.get(n, 0)]
    assert not bad, "kernels spilling: %s" % bad
