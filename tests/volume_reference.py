"""Volume rendering restated three times (the definition: the header of gaussianip_amd/csrc/volume.hip).

  march                         numpy float32, operation by operation as defined (numpy rounds every float32 operation on its own), with
                                the definition's min and max (`b < a ? b : a`, `b > a ? b : a`).  The kernels must equal it bit for bit.
  weights_f64, accumulate_f64   numpy float64 with sequential sums, and their analytic gradients weights_backward_f64 and
                                accumulate_backward_f64.  This is what the kernels and the op chain are measured against.
  chain_weights, chain_accumulate   a chain of torch ops, differentiable by autograd, on any device: a cumsum over all samples minus its
                                value at each ray's first sample (the segment cumsum), and index_add_.  In float32 it is the comparison
                                for the tolerances and for the benchmark; with dtype=torch.float64 it is a truth that autograd can
                                differentiate.  Chained(dtype) packs the two under the names utils/volume.py calls them by."""
import numpy as np
import torch

F = np.float32


def _min(a, b):
    return np.where(b < a, b, a)


def _max(a, b):
    return np.where(b > a, b, a)


# ------------------------------------------------------------------------------------------------------------------------ march
def ray_span(o, d, lo, hi, near, far):
    """(t_near, t_far) of one ray as float32 scalars, or None when the ray has no samples."""
    o, d = np.asarray(o, F), np.asarray(d, F)
    if not (np.isfinite(o).all() and np.isfinite(d).all() and (d != 0).any()):
        return None
    tn, tf = F(near), F(far)
    with np.errstate(all="ignore"):
        for a in range(3):
            if d[a] == 0:
                if not (lo[a] <= o[a] <= hi[a]):
                    return None
                continue
            inv = F(1) / d[a]
            ta, tb = (lo[a] - o[a]) * inv, (hi[a] - o[a]) * inv
            tn = F(_max(tn, _min(ta, tb)))
            tf = F(_min(tf, _max(ta, tb)))
    return (tn, tf) if tn < tf else None


def march_ray(o, d, occ, lo, hi, scale, dt, near, far, jitter, K_cap):
    """(t_starts, t_ends) float32 of one ray's kept candidates, in the order of k."""
    span = ray_span(o, d, lo, hi, near, far)
    none = np.zeros(0, F)
    if span is None:
        return none, none
    t_near, t_far = span
    o, d, G = np.asarray(o, F), np.asarray(d, F), occ.shape[0]
    with np.errstate(all="ignore"):
        k = np.arange(K_cap, dtype=F)
        ts = t_near + (k + F(jitter)) * F(dt)
        exists = ts < t_far
        te = _min(ts + F(dt), t_far).astype(F)
        tm = (ts + te) * F(0.5)
        cell = []
        for a in range(3):
            f = np.floor((o[a] + d[a] * tm - lo[a]) * scale[a])
            cell.append(np.where(f >= F(G - 1), G - 1, np.where(f > 0, f, 0)).astype(np.int64))      # a NaN fails both: cell 0
    assert ts.dtype == te.dtype == tm.dtype == F
    # the first candidate that does not exist ends the ray (ts does not decrease with k)
    assert not exists[int(np.argmin(exists)):].any() or exists.all()
    kept = exists & (occ[cell[0], cell[1], cell[2]] != 0)
    return ts[kept], te[kept]


def march(case):
    """(ray_indices [M] int32, t_starts [M], t_ends [M] float32, offsets [R + 1] int32) of a march case of tests/volume_inputs.py."""
    R = case["rays_o"].shape[0]
    rows = [march_ray(case["rays_o"][r], case["rays_d"][r], case["occ"], case["lo"], case["hi"], case["scale"], case["dt"], case["near"],
                      case["far"], 0.0 if case["jitter"] is None else case["jitter"][r], case["K_cap"]) for r in range(R)]
    counts = np.array([ts.shape[0] for ts, _ in rows], np.int64)
    offsets = np.concatenate(([0], np.cumsum(counts))).astype(np.int32)
    ray_indices = np.repeat(np.arange(R, dtype=np.int32), counts)
    t_starts = np.concatenate([ts for ts, _ in rows] + [np.zeros(0, F)]).astype(F)
    t_ends = np.concatenate([te for _, te in rows] + [np.zeros(0, F)]).astype(F)
    return ray_indices, t_starts, t_ends, offsets


# ------------------------------------------------------------------------------------------------------------------------ float64
def weights_f64(t_starts, t_ends, sigmas, offsets):
    """(weights, trans, alphas) [M] float64."""
    x = np.asarray(sigmas, np.float64) * (np.asarray(t_ends, np.float64) - np.asarray(t_starts, np.float64))
    trans = np.zeros_like(x)
    for r in range(len(offsets) - 1):
        a, b = int(offsets[r]), int(offsets[r + 1])
        trans[a:b] = np.exp(-(np.cumsum(x[a:b]) - x[a:b]))
    alphas = -np.expm1(-x)
    return trans * alphas, trans, alphas


def weights_backward_f64(t_starts, t_ends, sigmas, offsets, g_weights):
    """g_sigmas [M] float64: (te - ts) (g_w trans (1 - alpha) - the sum over the ray's later samples of g_w w)."""
    w, trans, alphas = weights_f64(t_starts, t_ends, sigmas, offsets)
    g = np.asarray(g_weights, np.float64)
    y = g * w
    later = np.zeros_like(y)
    for r in range(len(offsets) - 1):
        a, b = int(offsets[r]), int(offsets[r + 1])
        later[a:b] = np.cumsum(y[a:b][::-1])[::-1] - y[a:b]
    return (np.asarray(t_ends, np.float64) - np.asarray(t_starts, np.float64)) * (g * trans * (1 - alphas) - later)


def accumulate_f64(weights, values, offsets):
    """out [R, C] float64; values None: ones, C = 1."""
    w = np.asarray(weights, np.float64)
    v = np.ones((w.shape[0], 1)) if values is None else np.asarray(values, np.float64)
    out = np.zeros((len(offsets) - 1, v.shape[1]))
    for r in range(len(offsets) - 1):
        a, b = int(offsets[r]), int(offsets[r + 1])
        out[r] = (w[a:b, None] * v[a:b]).sum(0)
    return out


def accumulate_backward_f64(weights, values, ray_indices, g_out):
    """(g_weights [M], g_values [M, C]) float64; a ray index outside [0, R) gives zeros."""
    w, g_out = np.asarray(weights, np.float64), np.asarray(g_out, np.float64)
    v = np.ones((w.shape[0], 1)) if values is None else np.asarray(values, np.float64)
    idx = np.asarray(ray_indices, np.int64)
    ok = (idx >= 0) & (idx < g_out.shape[0])
    g = np.where(ok[:, None], g_out[np.where(ok, idx, 0)], 0.0)
    return (g * v).sum(1), w[:, None] * g


# ------------------------------------------------------------------------------------------------------------------------ op chain
def chain_weights(t_starts, t_ends, sigmas, ray_indices=None, n_rays=None, dtype=None):
    """(weights, trans, alphas) as a chain of torch ops in `dtype` (default: the sigmas')."""
    dtype = dtype or sigmas.dtype
    x = sigmas.to(dtype) * (t_ends.to(dtype) - t_starts.to(dtype))
    before = torch.cumsum(x, 0) - x                                  # over all samples
    if ray_indices is not None and x.shape[0]:
        idx = ray_indices.long()
        first = torch.searchsorted(idx, torch.arange(int(n_rays), device=idx.device)).clamp(max=x.shape[0] - 1)
        before = before - before[first][idx]                         # minus its value at the ray's first sample
    trans = torch.exp(-before)
    alphas = 1 - torch.exp(-x)
    return trans * alphas, trans, alphas


def chain_accumulate(weights, values=None, ray_indices=None, n_rays=None, dtype=None):
    """out [n_rays, C] by index_add_."""
    dtype = dtype or weights.dtype
    w = weights.to(dtype)
    src = w[:, None] if values is None else w[:, None] * values.to(dtype)
    if ray_indices is None:
        return src.sum(0, keepdim=True)
    return torch.zeros((int(n_rays), src.shape[1]), dtype=dtype, device=w.device).index_add_(0, ray_indices.long(), src)


# ------------------------------------------------------------------------------------------------------------------------ one case
def composite_f64(c):
    """Every compositing quantity of a case of volume_inputs.composite()'s layout by the float64 restatement: a dict of float64 arrays
    (weights, trans, alphas, g_sigmas, and per C out_cC, g_weights_cC, g_values_cC; out_none, g_weights_none for values None), and
    w_acc: the weights rounded once to float32, the input of every accumulate here, in the op chain and on the GPU."""
    w, trans, alphas = weights_f64(c["t_starts"], c["t_ends"], c["sigmas"], c["offsets"])
    out = dict(weights=w, trans=trans, alphas=alphas,
               g_sigmas=weights_backward_f64(c["t_starts"], c["t_ends"], c["sigmas"], c["offsets"], c["g_weights"]))
    w_acc = w.astype(np.float32)
    for C, v in c["values"].items():
        g_w, g_v = accumulate_backward_f64(w_acc, v, c["ray_indices"], c["g_out"][C])
        out.update({"out_c%d" % C: accumulate_f64(w_acc, v, c["offsets"]), "g_weights_c%d" % C: g_w, "g_values_c%d" % C: g_v})
    first = min(c["values"])
    out["out_none"] = accumulate_f64(w_acc, None, c["offsets"])
    out["g_weights_none"] = accumulate_backward_f64(w_acc, None, c["ray_indices"], c["g_out"][first][:, :1])[0]
    return out, w_acc


def composite_run(c, w_acc, weights_fn, accumulate_fn, device="cpu", dtype=torch.float32):
    """The same quantities through weights_fn / accumulate_fn (the op chain, or the kernels' Python surface) with leaves of `dtype`
    on `device`: a dict of float64 arrays under composite_f64's names."""
    def t(a, grad=False):
        x = torch.from_numpy(np.array(a)).to(device)
        return x.to(dtype).requires_grad_(True) if grad else (x.to(dtype) if x.is_floating_point() else x)
    ts, te, idx, R = t(c["t_starts"]), t(c["t_ends"]), t(c["ray_indices"]), c["n_rays"]
    sig = t(c["sigmas"], True)
    w, trans, alphas = weights_fn(ts, te, sig, idx, R)
    (g_sig,) = torch.autograd.grad((w * t(c["g_weights"])).sum(), sig)
    out = dict(weights=w, trans=trans, alphas=alphas, g_sigmas=g_sig)
    for C, v in c["values"].items():
        wv, vv = t(w_acc, True), t(v, True)
        acc = accumulate_fn(wv, vv, idx, R)
        g_w, g_v = torch.autograd.grad((acc * t(c["g_out"][C])).sum(), (wv, vv))
        out.update({"out_c%d" % C: acc, "g_weights_c%d" % C: g_w, "g_values_c%d" % C: g_v})
    wv = t(w_acc, True)
    acc = accumulate_fn(wv, None, idx, R)
    out["out_none"] = acc
    (out["g_weights_none"],) = torch.autograd.grad((acc * t(c["g_out"][min(c["values"])][:, :1])).sum(), wv)
    return {k: v.detach().cpu().numpy().astype(np.float64) for k, v in out.items()}


class Chained:
    """render_weight_from_density and accumulate_along_rays as the op chain in `dtype`: what a test puts in place of the kernels."""

    def __init__(self, dtype):
        self.dtype = dtype

    def render_weight_from_density(self, t_starts, t_ends, sigmas, ray_indices=None, n_rays=None):
        return chain_weights(t_starts, t_ends, sigmas, ray_indices, n_rays, self.dtype)

    def accumulate_along_rays(self, weights, values=None, ray_indices=None, n_rays=None):
        return chain_accumulate(weights, values, ray_indices, n_rays, self.dtype)
