"""Seeded inputs and the reference of tests/test_gpu_attention_variants.py (csrc/attention.hip).

Every generator returns fp16 CPU tensors q [B, Nq, H * D], k, v [B, Nkv, H * D] (heads interleaved along the last axis, the kernel's
layout) that depend on nothing but their arguments.  random() is the input of tests/test_gpu_attention.py: a softmax that is near
uniform over >= 1024 keys, where one key more or less moves the output by 1 / Nkv, inside the tolerance.  The other three make a
single key matter:

  planted     unit vectors u_j; k_j = s u_j, q_i = s u_t(i) with t(i) = (i + off) mod Nkv: the softmax of query i is one-hot on key
              t(i) (target_probability() >= 0.999 is asserted by the tests in float64), so the output row is v[t(i)] and a wrong key
              index, a dropped tail key or a key counted twice moves it by O(1).
  two_hot     planted, but in every (batch, head) one pair of key positions (a, b) from boundary_pairs() holds the SAME key row
              (k_b = k_a, different values) and every even query aims at it: its output is (v_a + v_b) / 2 — a dropped key gives one
              of the rows, a doubled one a 1/3 - 2/3 mix.  The pair is dealt out by (batch, head) index, odd queries stay planted.
  staircase   random q and 0.5 * random k with feature 0 overwritten: q[i, 0] = +8 / -8 for even / odd i, k[j, 0] = 60 (j / Nkv)^2.
              The row maximum of consecutive 64-key blocks climbs (even queries) or falls (odd) by 0 to about 11 exp2-units a block
              (20 blocks): both sides of the kernel's deferred-maximum threshold of 8, and the lanes of one wave disagree about it.
  constant    every key row equal: all scores of a query are equal and the output is the mean of v over the keys.

S[D] is the planted scale: s^2 / sqrt(D) * (1 - max coherence of random unit vectors in D dims) must leave ~ 12 nats between the
target and every other key.  18 / 15 / 14 for D = 40 / 64 / 80; D = 160 needs 20 (14 gives 0.9995)."""
import math

import torch

S = {40: 18.0, 64: 15.0, 80: 14.0, 160: 20.0}


def _gen(*seed):
    g = torch.Generator()
    s = 0
    for x in seed:
        s = (s * 1000003 + int(x) + 1) % 2147483647
    g.manual_seed(s)
    return g


def _units(g, B, N, H, D):
    u = torch.randn(B, N, H, D, generator=g, dtype=torch.float64)
    return u / u.norm(dim=-1, keepdim=True)


def random(B, H, Nq, Nkv, D, spread, seed=0):
    g = _gen(1, B, H, Nq, Nkv, D, int(spread), seed)
    q = (torch.randn(B, Nq, H * D, generator=g) * spread).half()
    k = (torch.randn(B, Nkv, H * D, generator=g) * spread).half()
    v = torch.randn(B, Nkv, H * D, generator=g).half()
    return q, k, v


def planted_targets(Nq, Nkv, off=0):
    return (torch.arange(Nq) + off) % Nkv


def planted(B, H, Nq, Nkv, D, off=0, seed=0):
    """-> q, k, v, targets [Nq] (the key every query's softmax is one-hot on)."""
    g = _gen(2, B, H, Nq, Nkv, D, seed)
    u = _units(g, B, Nkv, H, D)
    t = planted_targets(Nq, Nkv, off)
    k = (S[D] * u).reshape(B, Nkv, H * D).half()
    q = (S[D] * u[:, t]).reshape(B, Nq, H * D).half()
    v = torch.randn(B, Nkv, H * D, generator=g).half()
    return q, k, v, t


def boundary_pairs(Nkv):
    """Key pairs that straddle what the kernel splits the keys by: the whole range, the two 32-key tiles of a block, two blocks, the
    last two keys, the first and last key of the last (ragged) block, the two lane halves (keys 4 hh + 0..3 of every 8)."""
    last0 = (Nkv - 1) // 64 * 64
    pairs = [(0, Nkv - 1), (31, 32), (63, 64), (Nkv - 2, Nkv - 1), (last0, Nkv - 1), (3, 4)]
    return [(a, b) for a, b in pairs if 0 <= a < b < Nkv]


def two_hot(B, H, Nq, Nkv, D, seed=0):
    """-> q, k, v, ta, tb [B, H, Nq]: the two keys of every query's softmax (ta == tb where it is one-hot)."""
    g = _gen(3, B, H, Nq, Nkv, D, seed)
    u = _units(g, B, Nkv, H, D)
    pairs = boundary_pairs(Nkv)
    ta = planted_targets(Nq, Nkv).repeat(B, H, 1)
    tb = ta.clone()
    for b in range(B):
        for h in range(H):
            a_, b_ = pairs[(b * H + h + seed) % len(pairs)]
            u[b, b_, h] = u[b, a_, h]
            ta[b, h, 0::2] = a_
            # an odd (planted) query that lands on one of the pair's keys is two-hot as well
            on = (ta[b, h] == a_) | (ta[b, h] == b_)
            ta[b, h, on] = a_
            tb[b, h] = ta[b, h]
            tb[b, h, on] = b_
    qu = torch.gather(u.permute(0, 2, 1, 3), 2, ta[..., None].expand(B, H, Nq, D)).permute(0, 2, 1, 3)
    k = (S[D] * u).reshape(B, Nkv, H * D).half()
    q = (S[D] * qu).reshape(B, Nq, H * D).half()
    v = torch.randn(B, Nkv, H * D, generator=g).half()
    return q, k, v, ta, tb


def staircase(B, H, Nq, Nkv, D, seed=0):
    g = _gen(4, B, H, Nq, Nkv, D, seed)
    q = torch.randn(B, Nq, H, D, generator=g)
    k = torch.randn(B, Nkv, H, D, generator=g) * 0.5
    v = torch.randn(B, Nkv, H * D, generator=g).half()
    q[:, 0::2, :, 0] = 8.0
    q[:, 1::2, :, 0] = -8.0
    k[..., 0] = (60.0 * (torch.arange(Nkv, dtype=torch.float64) / Nkv) ** 2).float()[None, :, None]
    return q.reshape(B, Nq, H * D).half(), k.reshape(B, Nkv, H * D).half(), v


def constant(B, H, Nq, Nkv, D, seed=0):
    g = _gen(5, B, H, Nq, Nkv, D, seed)
    q = torch.randn(B, Nq, H * D, generator=g).half()
    k = torch.randn(B, 1, H * D, generator=g).half().expand(B, Nkv, H * D).contiguous()
    v = torch.randn(B, Nkv, H * D, generator=g).half()
    return q, k, v


def _heads(t, H):
    B, N, C = t.shape
    return t.view(B, N, H, C // H).transpose(1, 2)          # [B, H, N, D]


def reference(q, k, v, H, dtype=torch.float32):
    """softmax(q k^T / sqrt(D)) v of the fp16 operands in `dtype`, spelled out (one batch at a time: the scores of the largest case
    are 400 MB in float32) -> [B, Nq, H * D] in `dtype`."""
    B, Nq, C = q.shape
    out = torch.empty(B, Nq, C, dtype=dtype, device=q.device)
    scale = 1.0 / math.sqrt(C // H)
    for b in range(B):
        qb, kb, vb = [_heads(t[b:b + 1].to(dtype), H)[0] for t in (q, k, v)]
        p = torch.softmax(qb @ kb.transpose(1, 2) * scale, dim=-1)
        out[b] = (p @ vb).transpose(0, 1).reshape(Nq, C)
    return out


def target_probability(q, k, H, ta, tb=None):
    """Smallest float64 softmax mass, over all queries, on the target keys ta (and tb) [Nq] or [B, H, Nq]; with tb also the
    largest |p[ta] - p[tb]| where ta != tb -> (min mass, max imbalance)."""
    B, Nq, C = q.shape
    scale = 1.0 / math.sqrt(C // H)
    lo, imb = 1.0, 0.0
    for b in range(B):
        qb, kb = [_heads(t[b:b + 1].double(), H)[0] for t in (q, k)]
        p = torch.softmax(qb @ kb.transpose(1, 2) * scale, dim=-1)                # [H, Nq, Nkv]
        ia = (ta if ta.dim() == 1 else ta[b]).to(q.device).expand(H, Nq)[..., None]
        pa = p.gather(2, ia)[..., 0]
        mass = pa
        if tb is not None:
            ib = (tb if tb.dim() == 1 else tb[b]).to(q.device).expand(H, Nq)[..., None]
            pb = p.gather(2, ib)[..., 0]
            two = ia[..., 0] != ib[..., 0]
            mass = torch.where(two, pa + pb, pa)
            if bool(two.any()):
                imb = max(imb, float((pa - pb).abs()[two].max()))
        lo = min(lo, float(mass.min()))
    return lo, imb
