"""The hash-grid encoding on the GPU (csrc/hashgrid.hip, gaussianip_amd/utils/encoding.py), the feature network of TetrahedraSDFGrid,
render_field_mesh and GaussianModel.to_tetrahedra_sdf_grid(feature_steps=...).

Parity is against the float64 restatement of tests/hashgrid_reference.py on the cases of tests/hashgrid_inputs.py.  The rule, with the
constants of tests/test_gpu_isosurface.py: the kernel's error over the quantity's maximum is at most 4 x the float32 op chain's own
error on the same case (run on the CPU inside the test, normalised the same way) + 1e-6.  Every element of enc, g_x and g_table is
compared: cells are float32 by definition, so there is no knife edge to exclude.
With GIP_HASHGRID_PARITY_OUT=<file> the figures are written there as JSON (profiles/hashgrid_parity.json is such a run)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import field_inputs
import hashgrid_inputs as inputs
import hashgrid_reference as reference

pytestmark = pytest.mark.gpu
FACTOR, FLOOR = 4.0, 1e-6
_figures = {}


@pytest.fixture(scope="module", autouse=True)
def _write_figures():
    yield
    out = os.environ.get("GIP_HASHGRID_PARITY_OUT")
    if out and _figures:
        with open(out, "w") as f:
            f.write(json.dumps(_figures, indent=1, sort_keys=True) + "\n")


def _cu(a):
    return torch.from_numpy(np.array(a)).cuda()                 # a copy: the cases' arrays are read-only


def _np(t):
    return t.detach().cpu().numpy()


def _counts():
    from gaussianip_amd import _lib
    return dict(_lib.call_counts)


def _launches(before):
    after = _counts()
    return {k: after[k] - before.get(k, 0) for k in after if after[k] != before.get(k, 0)}


def _rule(name, got, f64, chain):
    """The module's rule for one quantity: got (the kernels), f64 (the truth) and chain (the float32 op chain) as arrays."""
    got, f64, chain = (np.asarray(a, np.float64) for a in (got, f64, chain))
    assert got.shape == f64.shape == chain.shape and np.isfinite(got).all(), name
    mx = np.abs(f64).max()
    assert mx > 0, name
    err, ref_err = float(np.abs(got - f64).max() / mx), float(np.abs(chain - f64).max() / mx)
    bar = FACTOR * ref_err + FLOOR
    print("%s: kernel %.3e op chain %.3e bar %.3e (maximum %.3e)" % (name, err, ref_err, bar, mx))
    _figures[name] = dict(kernel_err=err, op_chain_err=ref_err, bar=bar, maximum=float(mx))
    assert err <= bar, (name, err, ref_err, bar)


@functools.lru_cache(maxsize=None)
def _truth(name):
    """(enc, g_x, g_table) of a case twice: the float64 restatement, and the float32 op chain on the CPU.  Computed once and shared."""
    cfg, x, table, g = inputs.case(name)
    lay = inputs.layout(name)
    f64 = (reference.encode_f64(x, table, lay),) + reference.backward_f64(x, table, g, lay)
    xt, tt = torch.from_numpy(x.copy()).requires_grad_(True), torch.from_numpy(table.copy()).requires_grad_(True)
    enc = reference.op_chain(xt, tt, lay)
    gx, gt = torch.autograd.grad((enc * torch.from_numpy(g.copy())).sum(), (xt, tt))
    return f64, (enc.detach().numpy(), gx.numpy(), gt.numpy())


def _run(name, x=None, g=None):
    """(enc, g_x, g_table) of the kernels on a case (or on other points and upstream rows with the case's table)."""
    from gaussianip_amd.utils.encoding import hash_grid_encode
    cfg, cx, table, cg = inputs.case(name)
    xt = _cu(cx if x is None else x).requires_grad_(True)
    tt = _cu(table).requires_grad_(True)
    enc = hash_grid_encode(xt, tt, inputs.layout(name))
    gx, gt = torch.autograd.grad((enc * _cu(cg if g is None else g)).sum(), (xt, tt))
    return enc.detach(), gx, gt


# ---------------------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("name", [n for n in inputs.CASES if n != "e_n0"])
def test_parity_with_the_restatement(name):
    lay = inputs.layout(name)
    f64, chain = _truth(name)
    before = _counts()
    got = _run(name)
    assert _launches(before) == {"gip_hashgrid_forward": 1, "gip_hashgrid_backward_input": 1, "gip_hashgrid_backward_table": 1}
    N = inputs.case(name)[1].shape[0]
    assert got[0].dtype == torch.float32 and tuple(got[0].shape) == (N, lay.n_output_dims)
    assert tuple(got[1].shape) == (N, 3) and tuple(got[2].shape) == (lay.n_rows, lay.n_features_per_level)
    for what, a, b, c in zip(("enc", "g_x", "g_table"), got, f64, chain):
        _rule("%s_%s" % (name, what), _np(a), b, c)


def test_no_points_launch_nothing():
    from gaussianip_amd.utils.encoding import HashGridEncoding, hash_grid_encode
    lay = inputs.layout("e_n0")
    cfg, x, table, g = inputs.case("e_n0")
    before = _counts()
    enc, gx, gt = _run("e_n0")
    assert _launches(before) == {}
    assert tuple(enc.shape) == (0, 12) and tuple(gx.shape) == (0, 3) and tuple(gt.shape) == table.shape and not gt.any()
    # the module takes any leading shape; wrong devices, dtypes and shapes raise
    module = HashGridEncoding(3, inputs.config("a")).cuda()
    assert module(torch.rand(2, 5, 3, device="cuda")).shape == (10, 12) and module.n_output_dims == 12
    tt = _cu(table)
    for bad_x in (torch.rand(4, 3), torch.rand(4, 3, device="cuda").double(), torch.rand(4, 2, device="cuda"), torch.rand(3, device="cuda")):
        with pytest.raises(ValueError, match="float32 GPU tensor"):
            hash_grid_encode(bad_x, tt, lay)
    for bad_t in (tt.cpu(), tt.double(), tt[:-1], tt.reshape(-1)):
        with pytest.raises(ValueError, match="table"):
            hash_grid_encode(torch.rand(4, 3, device="cuda"), bad_t, lay)
    # a table that is a view at an address of no particular alignment is the same table
    wide = torch.zeros(tt.numel() + 1, device="cuda")
    wide[1:] = tt.reshape(-1)
    xs = _cu(inputs.case("a")[1])
    assert torch.equal(hash_grid_encode(xs, wide[1:].view_as(tt), lay), hash_grid_encode(xs, tt, lay))


# ---------------------------------------------------------------------------------------------------------------- 2. reproducible
@pytest.mark.parametrize("name", ["a", "b_f8_n65", "c"])
def test_bit_reproducible(name):
    first, second = _run(name), _run(name)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    # the table's gradient is summed by float atomics in the order they arrive: it is the one output that may differ in its last bits
    print("%s: g_table differs between two runs in %d of %d entries" % (name, int((first[2] != second[2]).sum()), first[2].numel()))


# ---------------------------------------------------------------------------------------------------------------- 3. edge points
def test_edge_points():
    cfg, x, table, g = inputs.case("d")
    enc, gx, gt = _run("d")
    bad = inputs.D_NONFINITE
    assert not enc[bad].any() and not gx[bad].any()                   # exact zeros, not small numbers
    assert torch.isfinite(enc).all() and torch.isfinite(gx).all() and torch.isfinite(gt).all()
    assert enc[inputs.D_OUTSIDE].all() and enc[inputs.D_ZERO].all() and enc[inputs.D_ONE].all()
    # the non-finite rows add nothing to the table's gradient: without them it is the same up to the order of the atomic adds
    keep = np.ones(x.shape[0], bool)
    keep[bad] = False
    _, _, gt_without = _run("d", x[keep], g[keep])
    f64 = _truth("d")[0][2]
    _rule("d_g_table_without_nonfinite", _np(gt_without), f64, _truth("d")[1][2])
    enc_bad, gx_bad, gt_bad = _run("d", x[bad], g[bad])
    assert not enc_bad.any() and not gx_bad.any() and not gt_bad.any()
    # 64 copies of a point give 64 x one copy's gradient
    one = inputs.D_COPIES.start
    _, gx_one, gt_one = _run("d", x[one:one + 1], g[one:one + 1])
    _, gx_many, gt_many = _run("d", x[inputs.D_COPIES], g[inputs.D_COPIES])
    assert torch.equal(gx_many, gx_one.expand(64, 3)) and torch.equal(gx[inputs.D_COPIES], gx_many)
    lay = inputs.layout("d")
    ref_one = reference.backward_f64(x[one:one + 1], table, g[one:one + 1], lay)[1]
    assert np.count_nonzero(ref_one) <= 8 * lay.n_output_dims
    xt, tt = torch.from_numpy(x[inputs.D_COPIES].copy()), torch.from_numpy(table.copy()).requires_grad_(True)
    (chain_many,) = torch.autograd.grad((reference.op_chain(xt, tt, lay) * torch.from_numpy(g[inputs.D_COPIES].copy())).sum(), tt)
    _rule("d_g_table_64_copies", _np(gt_many), 64.0 * ref_one, chain_many.numpy())
    assert torch.equal(gt_many != 0, gt_one != 0)                     # the same rows and no others


# ---------------------------------------------------------------------------------------------------------------- 4. autograd
def _mlp_weights(seed, n_in):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.rand((64, n_in), generator=gen) - 0.5) * 0.5, (torch.rand((3, 64), generator=gen) - 0.5) * 0.5]


def test_autograd_through_encoding_and_mlp():
    """HashGridEncoding + VanillaMLP on the GPU against the op chain + the same MLP on the CPU, in float32 and, as the truth, in
    float64: the features and the gradients to the table and to both weight matrices, under the module's rule."""
    from gaussianip_amd.utils.encoding import get_encoding, get_mlp
    cfg, x, table, _ = inputs.case("a")
    lay = inputs.layout("a")
    weights = _mlp_weights(5, lay.n_output_dims)
    target = torch.from_numpy(np.random.default_rng(6).random((x.shape[0], 3), dtype=np.float32))

    def loss_and_grads(features, leaves, tgt):
        loss = ((torch.sigmoid(features) - tgt) ** 2).mean()
        return [features.detach()] + list(torch.autograd.grad(loss, leaves))

    def on_cpu(dtype):
        enc = reference.ChainEncoding(lay, torch.from_numpy(table.copy()).reshape(-1), dtype)
        w = [a.clone().to(dtype).requires_grad_(True) for a in weights]
        feats = torch.relu(enc(torch.from_numpy(x.copy())) @ w[0].t()) @ w[1].t()
        return [_np(t).astype(np.float64) for t in loss_and_grads(feats, [enc.params] + w, target.to(dtype))]

    encoding = get_encoding(3, cfg).cuda()
    mlp = get_mlp(encoding.n_output_dims, 3, {"otype": "VanillaMLP", "output_activation": "none", "n_neurons": 64, "n_hidden_layers": 1}).cuda()
    with torch.no_grad():
        encoding.encoding.params.copy_(_cu(table).reshape(-1))
        mlp.layers[0].weight.copy_(weights[0].cuda())
        mlp.layers[2].weight.copy_(weights[1].cuda())
    feats = mlp(encoding(_cu(x)))
    got = loss_and_grads(feats, [encoding.encoding.params, mlp.layers[0].weight, mlp.layers[2].weight], target.cuda())
    f64, f32 = on_cpu(torch.float64), on_cpu(torch.float32)
    for what, a, b, c in zip(("features", "g_params", "g_weight0", "g_weight1"), got, f64, f32):
        _rule("mlp_%s" % what, _np(a).reshape(b.shape), b, c)


# ---------------------------------------------------------------------------------------------------------------- 5. the loop closes
STEPS = 10


def _field_geometry(kind):
    """A sphere of radius 0.3 on the Kuhn grid at R = 16 with a small feature network; kind: "kernel", or the op chain in "float32" or
    "float64" in place of the encoding (and, in float64, of the MLP's weights).  The same starting values in every kind."""
    from gaussianip_amd.utils.isosurface import TetrahedraSDFGrid
    torch.manual_seed(11)
    geom = TetrahedraSDFGrid(isosurface_resolution=16, shape_init="sphere", shape_init_params=0.3, n_feature_dims=3,
                             pos_encoding_config=dict(inputs.CONFIG_SMALL)).cuda()
    geom.initialize_shape()
    if kind != "kernel":
        dtype = torch.float32 if kind == "float32" else torch.float64
        inner = geom.encoding.encoding
        geom.encoding.encoding = reference.ChainEncoding(inner.layout, inner.params, dtype).cuda()
        geom.feature_network.to(dtype)
    return geom


def _views():
    flat = torch.diag(torch.tensor([1.0, 1.0, 0.5, 1.0]))              # the bbox [-1, 1]^3 seen along z, without perspective
    c, s = np.cos(1.1), np.sin(1.1)
    turn = torch.tensor([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1]], dtype=torch.float32)
    mvp = torch.stack((flat, flat @ turn)).cuda()
    eye = torch.tensor([[0.0, 0.0, -2.0], [2.0 * s, 0.0, -2.0 * c]]).cuda()
    return mvp, eye


class _Painted:
    """The geometry with its features replaced by a smooth function of the position: what the target is rendered from."""

    def __init__(self, geometry):
        self.geometry = geometry

    def isosurface(self):
        return self.geometry.isosurface()

    def __call__(self, positions):
        colour = 0.5 + 0.4 * torch.sin(positions.detach() * torch.tensor([9.0, 7.0, 5.0], device=positions.device) + 0.3)
        return {"features": torch.log(colour / (1.0 - colour))}


def _fit(kind, ctx, target=None):
    from gaussianip_amd.utils.rasterize import render_field_mesh
    geom = _field_geometry(kind)
    mvp, eye = _views()
    if target is None:
        with torch.no_grad():
            target = render_field_mesh(ctx, _Painted(geom), mvp, eye, 64, 64, bg_color=(0.1, 0.2, 0.3))["comp_rgb"]
    features = list(geom.encoding.parameters()) + list(geom.feature_network.parameters())
    optimizer = torch.optim.Adam(features, lr=0.01)
    losses, first = [], None
    for step in range(STEPS + 1):
        optimizer.zero_grad()
        geom.zero_grad()
        out = render_field_mesh(ctx, geom, mvp, eye, 64, 64, bg_color=(0.1, 0.2, 0.3))
        loss = ((out["comp_rgb"] - target) ** 2).mean()
        losses.append(float(loss.detach()))
        if step == STEPS:
            break
        loss.backward()
        if step == 0:
            first = dict(out=out, sdf_grad=geom.sdf.grad.clone(), deformation_grad=geom.deformation.grad.clone())
        optimizer.step()
    return geom, target, losses, first


def test_the_loop_closes():
    """render_field_mesh at 64 x 64 from two views, a target colour that is a smooth function of the surface position rendered through
    the same rasterizer, STEPS Adam steps on the feature parameters: the loss falls; the same steps with the op chain in place of the
    kernels give the same losses under the module's rule (the chain in float64 is the truth); and the signed distance receives a
    gradient through the positions, at grid vertices with a crossing edge and nowhere else."""
    from gaussianip_amd.utils.rasterize import DiffMeshRasterizerContext
    ctx = DiffMeshRasterizerContext()
    before = _counts()
    geom, target, losses, first = _fit("kernel", ctx)
    used = _launches(before)
    assert used["gip_hashgrid_forward"] == STEPS + 1 and used["gip_hashgrid_backward_table"] == STEPS == used["gip_hashgrid_backward_input"]
    out = first["out"]
    assert tuple(out["comp_rgb"].shape) == (2, 64, 64, 3) and tuple(out["opacity"].shape) == (2, 64, 64, 1)
    assert tuple(out["comp_normal"].shape) == (2, 64, 64, 3) and out["mesh"].t_pos_idx.shape[0] > 100
    covered = out["opacity"] > 0.999
    assert 300 < int(covered.sum()) < 64 * 64                        # two discs of radius 0.3 x 32 pixels
    background = out["opacity"][..., 0] == 0
    assert torch.allclose(out["comp_rgb"][background], torch.tensor([0.1, 0.2, 0.3], device="cuda").expand(int(background.sum()), 3))
    assert float(out["comp_normal"].min()) >= 0 and float(out["comp_normal"].max()) <= 1 + 1e-6 and not out["comp_normal"][background].any()
    print("losses", " ".join("%.6f" % v for v in losses))
    assert losses[-1] < losses[0]
    _, _, chain32, _ = _fit("float32", ctx, target)
    _, _, chain64, _ = _fit("float64", ctx, target)
    _rule("loop_losses", losses, chain64, chain32)
    _figures["loop"] = dict(steps=STEPS, loss_first=losses[0], loss_last=losses[-1])
    # the geometry hears of the colour: through the antialiased silhouette and through the positions the features are looked up at
    grid = geom.isosurface_helper.grid
    fresh = _field_geometry("kernel")                                  # the signed distance was not stepped: the same surface
    occ = fresh.sdf.detach().reshape(-1) > 0
    a, b = grid.edges[:, 0], grid.edges[:, 1]
    touched = torch.zeros(grid.num_vertices, dtype=torch.bool, device="cuda")
    crossing = occ[a] != occ[b]
    touched[a[crossing]] = True
    touched[b[crossing]] = True
    g = first["sdf_grad"].reshape(-1)
    assert torch.isfinite(g).all() and g.any() and not g[~touched].any()
    assert first["deformation_grad"].any() and not first["deformation_grad"][~touched].any()
    # through the positions alone: the features at the surface's own vertices
    with torch.no_grad():
        fresh.encoding.encoding.params.uniform_(-1.0, 1.0)
    mesh = fresh.isosurface()
    (g_pos,) = torch.autograd.grad(fresh(mesh.v_pos)["features"].square().sum(), fresh.sdf)
    g_pos = g_pos.reshape(-1)
    assert torch.isfinite(g_pos).all() and g_pos.any() and not g_pos[~touched].any()


# ---------------------------------------------------------------------------------------------------------------- 6. from the Gaussians
def test_features_from_the_gaussians():
    from gaussianip_amd.scene import GaussianModel
    cl, R, nb = field_inputs.case("b")
    gm = GaussianModel(0)
    gm._xyz, gm._opacity = _cu(cl["xyz"]), _cu(cl["opacity"])
    gm._scaling, gm._rotation = _cu(cl["scaling"]), _cu(cl["rotation"])
    P = cl["xyz"].shape[0]
    rng = np.random.default_rng(3)
    gm._features_dc = _cu(rng.standard_normal((P, 1, 3)).astype(np.float32))
    gm._features_rest = torch.zeros((P, 0, 3), device="cuda")
    gm.extract_fields(resolution=R, num_blocks=nb)
    probe = gm.to_tetrahedra_sdf_grid(resolution=12, density_thresh=1.0, field_resolution=R, num_blocks=nb)
    density = gm.sample_fields(probe.isosurface_helper.grid_vertices * (probe.isosurface_bbox[1] - probe.isosurface_bbox[0]) +
                               probe.isosurface_bbox[0], resolution=R, num_blocks=nb)["density"]
    thresh = 0.5 * float(density.max())
    kwargs = dict(resolution=12, density_thresh=thresh, field_resolution=R, num_blocks=nb, pos_encoding_config=dict(inputs.CONFIG_SMALL))
    assert probe.n_feature_dims == 0 and not hasattr(probe, "encoding")
    torch.manual_seed(21)
    fitted = gm.to_tetrahedra_sdf_grid(feature_steps=20, **kwargs)
    torch.manual_seed(21)
    untrained = gm.to_tetrahedra_sdf_grid(feature_steps=1, feature_lr=0.0, **kwargs)
    assert fitted.n_feature_dims == 3 and torch.equal(fitted.sdf, untrained.sdf) and fitted.mesh is None
    vertices = fitted.isosurface().v_pos.detach().contiguous()
    assert vertices.shape[0] > 50
    target = gm.sample_fields(vertices, resolution=R, num_blocks=nb)["color"]
    assert float(target.std()) > 1e-3                                  # the colours vary over the surface
    with torch.no_grad():
        mse = [float(((torch.sigmoid(g(vertices)["features"]) - target) ** 2).mean()) for g in (fitted, untrained)]
    print("vertex colour MSE: fitted %.5f, untrained %.5f" % tuple(mse))
    _figures["from_the_gaussians"] = dict(mse_fitted=mse[0], mse_untrained=mse[1], vertices=int(vertices.shape[0]))
    assert mse[0] < mse[1]
    with pytest.raises(ValueError):
        gm.to_tetrahedra_sdf_grid(feature_steps=-1, **kwargs)
