"""NeuS volume rendering restated three times (the definition: the header of gaussianip_amd/csrc/volume_sdf.hip).

  render_f64, render_backward_f64   numpy float64, sample by sample, with the hand-written backward: the division-free reverse
                                    recurrence for the weights and the closed form for alpha.  This is what the kernels and the op
                                    chain are measured against.  weights_from_alpha_f64 / weights_from_alpha_backward_f64 are the
                                    primitive alone, and weights_from_alpha_backward_division the textbook form that divides by
                                    1 - alpha.
  render_autograd                   torch autograd of the reference's formulas (ref_alpha below, alpha x the exclusive cumprod of
                                    1 - alpha, sums), ray by ray, in float64: the check of the hand-written backward.
  render_chain                      the float32 op chain ray by ray on the CPU: utils.sdf_volume.neus_alpha, alpha x the exclusive
                                    cumprod, index_add_.  The comparison for the tolerances.
All three return the same dict of float64 arrays: alphas, trans, weights, out, g_sdf, g_normals (with normals), g_values (with
values), g_inv_std."""
import numpy as np
import torch

EPS = 1e-5


def _f64(a):
    return None if a is None else np.asarray(a, np.float64)


def variant_arrays(c, with_normals, C):
    """(normals or None, values or None, g_out) of a variant of sdf_volume_inputs.composite()."""
    return (c["normals"] if with_normals else None), c["values"][C], c["g_out"][C]


# ------------------------------------------------------------------------------------------------------------------------ float64
def alpha_f64(sdf, normals, dirs, delta, beta, rho):
    """(alpha, and what its backward needs: t, prev, next, c, m, q) in float64; dirs per sample."""
    if normals is None:
        t, ic = np.zeros_like(sdf), -np.ones_like(sdf)
    else:
        t = (dirs * normals).sum(1)
        ic = -(np.maximum(-0.5 * t + 0.5, 0) * (1 - rho) + np.maximum(-t, 0) * rho)
    h = ic * delta * 0.5
    prev, nxt = sdf - h, sdf + h
    with np.errstate(over="ignore"):
        c, m = 1 / (1 + np.exp(-prev * beta)), 1 / (1 + np.exp(-nxt * beta))
    q = (c - m + EPS) / (c + EPS)
    return np.clip(q, 0, 1), (t, prev, nxt, c, m, q)


def weights_from_alpha_f64(alphas, offsets):
    """(weights, trans) [M] float64."""
    a = _f64(alphas)
    trans = np.ones_like(a)
    for r in range(len(offsets) - 1):
        T = 1.0
        for i in range(int(offsets[r]), int(offsets[r + 1])):
            trans[i] = T
            T = T * (1 - a[i])
    return trans * a, trans


def weights_from_alpha_backward_f64(alphas, offsets, g_weights):
    """g_alphas [M] float64 by the recurrence U_last = 0, U_i = a_(i+1) g_(i+1) + (1 - a_(i+1)) U_(i+1), g_alpha_i = trans_i (g_i - U_i)."""
    a, g = _f64(alphas), _f64(g_weights)
    _, trans = weights_from_alpha_f64(a, offsets)
    out = np.zeros_like(a)
    for r in range(len(offsets) - 1):
        U = 0.0
        for i in range(int(offsets[r + 1]) - 1, int(offsets[r]) - 1, -1):
            out[i] = trans[i] * (g[i] - U)
            U = a[i] * g[i] + (1 - a[i]) * U
    return out


def weights_from_alpha_backward_division(alphas, offsets, g_weights):
    """The textbook form g_alpha_i = g_i trans_i - (the sum over k > i of g_k w_k) / (1 - alpha_i): 0 / 0 at alpha_i == 1."""
    a, g = _f64(alphas), _f64(g_weights)
    w, trans = weights_from_alpha_f64(a, offsets)
    y = g * w
    later = np.zeros_like(y)
    for r in range(len(offsets) - 1):
        lo, hi = int(offsets[r]), int(offsets[r + 1])
        later[lo:hi] = np.cumsum(y[lo:hi][::-1])[::-1] - y[lo:hi]
    with np.errstate(all="ignore"):
        return g * trans - later / (1 - a)


def _tm(c):
    return (_f64(c["t_starts"]) + _f64(c["t_ends"])) * 0.5


def render_f64(c, beta, rho, normals, values):
    """dict(alphas, trans, weights [M], out [R, 2 + C]) in float64."""
    dirs = _f64(c["rays_d"])[c["ray_indices"]]
    alphas, _ = alpha_f64(_f64(c["sdf"]), _f64(normals), dirs, _f64(c["t_ends"]) - _f64(c["t_starts"]), beta, rho)
    weights, trans = weights_from_alpha_f64(alphas, c["offsets"])
    cols = [np.ones_like(weights)[:, None], _tm(c)[:, None]] + ([] if values is None else [_f64(values)])
    src = weights[:, None] * np.concatenate(cols, axis=1)
    out = np.zeros((c["n_rays"], src.shape[1]))
    for r in range(c["n_rays"]):
        out[r] = src[int(c["offsets"][r]):int(c["offsets"][r + 1])].sum(0)
    return dict(alphas=alphas, trans=trans, weights=weights, out=out)


def render_backward_f64(c, beta, rho, normals, values, g_out, g_weights):
    """dict(g_sdf [M], g_normals [M, 3] with normals, g_values [M, C] with values, g_inv_std) in float64, hand-written."""
    idx = c["ray_indices"]
    dirs = _f64(c["rays_d"])[idx]
    delta = _f64(c["t_ends"]) - _f64(c["t_starts"])
    alphas, (t, prev, nxt, cc, m, q) = alpha_f64(_f64(c["sdf"]), _f64(normals), dirs, delta, beta, rho)
    weights, trans = weights_from_alpha_f64(alphas, c["offsets"])
    go = _f64(g_out)[idx]
    g_w = (0 if g_weights is None else _f64(g_weights)) + go[:, 0] + go[:, 1] * _tm(c)
    out = {}
    if values is not None:
        g_w = g_w + (go[:, 2:] * _f64(values)).sum(1)
        out["g_values"] = weights[:, None] * go[:, 2:]
    g_alpha = weights_from_alpha_backward_f64(alphas, c["offsets"], g_w)
    g_q = np.where((q >= 0) & (q <= 1), g_alpha, 0.0)
    g_xp = g_q * m / (cc + EPS) ** 2 * cc * (1 - cc)
    g_xn = -g_q / (cc + EPS) * m * (1 - m)
    out["g_sdf"] = beta * (g_xp + g_xn)
    out["g_inv_std"] = np.array([(g_xp * prev + g_xn * nxt).sum()])
    if normals is not None:
        g_ic = beta * (g_xn - g_xp) * delta * 0.5
        slope = 0.5 * (1 - rho) * (-0.5 * t + 0.5 > 0) + rho * (t < 0)
        out["g_normals"] = (g_ic * slope)[:, None] * dirs
    return out


def render_all_f64(c, beta, rho, normals, values, g_out, g_weights):
    out = render_f64(c, beta, rho, normals, values)
    out.update(render_backward_f64(c, beta, rho, normals, values, g_out, g_weights))
    return out


# ------------------------------------------------------------------------------------------------------------------------ torch
def ref_alpha(sdf, normal, dirs, dists, inv_std, cos_anneal_ratio):
    """The reference's get_alpha (use_volsdf off) restated; normal None: its alpha_fn."""
    if normal is None:
        iter_cos = -1.0
    else:
        true_cos = (dirs * normal).sum(-1)
        iter_cos = -(torch.relu(-true_cos * 0.5 + 0.5) * (1.0 - cos_anneal_ratio) + torch.relu(-true_cos) * cos_anneal_ratio)
    estimated_next_sdf = sdf + iter_cos * dists * 0.5
    estimated_prev_sdf = sdf - iter_cos * dists * 0.5
    prev_cdf = torch.sigmoid(estimated_prev_sdf * inv_std)
    next_cdf = torch.sigmoid(estimated_next_sdf * inv_std)
    return ((prev_cdf - next_cdf + EPS) / (prev_cdf + EPS)).clip(0.0, 1.0)


def exclusive_cumprod(x):
    return torch.cat((torch.ones_like(x[:1]), torch.cumprod(x, 0)[:-1])) if x.shape[0] else x


def _render_torch(c, beta, rho, normals, values, g_out, g_weights, dtype, alpha_fn):
    def t(a, grad=False):
        return None if a is None else torch.from_numpy(np.array(a)).to(dtype).requires_grad_(grad)
    sdf, nrm, val, inv_std = t(c["sdf"], True), t(normals, True), t(values, True), torch.tensor([beta], dtype=dtype, requires_grad=True)
    ts, te, d = t(c["t_starts"]), t(c["t_ends"]), t(c["rays_d"])
    idx = torch.from_numpy(np.array(c["ray_indices"])).long()
    R, M = c["n_rays"], sdf.shape[0]
    alphas, trans = [], []
    for r in range(R):
        a, b = int(c["offsets"][r]), int(c["offsets"][r + 1])
        alpha = alpha_fn(sdf[a:b], None if nrm is None else nrm[a:b], d[r].expand(b - a, 3), te[a:b] - ts[a:b], inv_std, rho)
        alphas.append(alpha)
        trans.append(exclusive_cumprod(1 - alpha))
    alphas, trans = torch.cat(alphas), torch.cat(trans)
    weights = alphas * trans
    cols = [torch.ones((M, 1), dtype=dtype), ((ts + te) * 0.5)[:, None]] + ([] if val is None else [val])
    out = torch.zeros((R, 2 + (0 if val is None else val.shape[1])), dtype=dtype).index_add_(0, idx, weights[:, None] * torch.cat(cols, dim=1))
    loss = (out * t(g_out)).sum() + (0 if g_weights is None else (weights * t(g_weights)).sum())
    leaves = [x for x in (sdf, nrm, val, inv_std) if x is not None]
    grads = dict(zip([n for n, x in zip(("g_sdf", "g_normals", "g_values", "g_inv_std"), (sdf, nrm, val, inv_std)) if x is not None],
                     torch.autograd.grad(loss, leaves)))
    res = dict(alphas=alphas, trans=trans, weights=weights, out=out, **grads)
    return {k: v.detach().numpy().astype(np.float64) for k, v in res.items()}


def render_autograd(c, beta, rho, normals, values, g_out, g_weights):
    """torch float64 autograd of the reference's formulas, ray by ray."""
    return _render_torch(c, beta, rho, normals, values, g_out, g_weights, torch.float64, ref_alpha)


def render_chain(c, beta, rho, normals, values, g_out, g_weights):
    """The float32 op chain on the CPU, with the package's neus_alpha."""
    from gaussianip_amd.utils.sdf_volume import neus_alpha
    return _render_torch(c, beta, rho, normals, values, g_out, g_weights, torch.float32, neus_alpha)


def weights_chain(alphas, offsets, g_weights, dtype=torch.float32):
    """dict(weights, trans, g_alphas): alpha x the exclusive cumprod per ray with autograd, in dtype, on the CPU."""
    a = torch.from_numpy(np.array(alphas)).to(dtype).requires_grad_(True)
    trans = torch.cat([exclusive_cumprod(1 - a[int(offsets[r]):int(offsets[r + 1])]) for r in range(len(offsets) - 1)])
    weights = a * trans
    (g,) = torch.autograd.grad((weights * torch.from_numpy(np.array(g_weights)).to(dtype)).sum(), a)
    return {k: v.detach().numpy().astype(np.float64) for k, v in dict(weights=weights, trans=trans, g_alphas=g).items()}
