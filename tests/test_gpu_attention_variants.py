"""Every kernel instantiation behind gip_attention_fwd_strided2_f16 (csrc/attention.hip) against softmax(QK^T / sqrt(D)) V in float32 on
the same fp16 operands, at the edges of each: ragged key tails, workgroups with query-less waves, the XCD remap at several grid
shapes, strided q / k / v, both second-key-set kernels at their block boundaries.  The bar is the one of tests/test_gpu_attention.py
(probabilities and the output are rounded to half once each): max|o - ref| <= 3e-3 * max(1, max|ref|) over every element.

On random data with >= 1024 keys that bar cannot see one key too few or too many (1 / Nkv of the output's scale), so the inputs of
tests/attention_inputs.py make single keys carry the whole output (planted, two_hot), walk the deferred running maximum over its
threshold (staircase) or make the answer a plain mean (constant).  Every call asserts which kernel ran (gip_dbg_attn_last_variant);
the long-key variants are switched in-process by gip_dbg_attn_qt / gip_dbg_attn_nw and must be BIT-equal to the plain loop."""
import contextlib
import ctypes
import functools

import pytest
import torch

import attention_inputs as ai

pytestmark = pytest.mark.gpu

# enum AttnVariant of csrc/attention.hip
PLAIN, SET2_SMALL, SET2_LONG, WIDE8, Q2_8, Q2_4 = range(6)
ALL_INSTANTIATIONS = ({(var, D) for var in (PLAIN, SET2_SMALL, SET2_LONG) for D in (40, 64, 80, 160)} |
                      {(WIDE8, 40), (Q2_8, 40), (Q2_4, 40)})
SEEN = set()            # (variant, D) of every call this module made

# D = 40, >= 1024 keys, Nq % 64 == 0 and ceil(Nq / 512) * B * H >= 192: two query tiles per wave, 512 queries per workgroup
Q2_SHAPES = [(24, 8, 64, 1061),     # gx = 1, 192 workgroups (remap on), 7 of 8 waves without queries, ragged keys (16 * 64 + 37)
             (8, 8, 1536, 1030),    # gx = 3, 192 workgroups: remap on with a gx that is no power of two; 6 keys in the last block
             (5, 13, 1088, 1024)]   # gx = 3, 195 workgroups: no multiple of 8, remap off; last workgroup has one live wave; whole blocks
NEAR_MISSES = [(24, 8, 96, 1061),   # Nq % 64 != 0
               (24, 8, 64, 1023),   # Nkv < 1024
               (23, 8, 64, 1061)]   # 184 workgroups < 192
SMALL_GRIDS = [(2, 2, 256, 1061), (1, 8, 512, 1090)]        # reach the long-key variants only through the knobs
GENERATORS = ("random1", "random6", "planted", "two_hot", "staircase")
# (gip_dbg_attn_qt, gip_dbg_attn_nw) -> the variant a D = 40, >= 1024-key shape must report
SETTINGS = {"plain": (1, -1), "wide": (1, 8), "nw4": (-1, 4), "q2": (2, -1), "q2_nw4": (2, 4)}


def expected_variant(setting, shape):
    B, H, Nq, Nkv = shape
    if setting == "plain":
        return PLAIN
    if setting == "wide":
        return WIDE8 if Nq % 256 == 0 else PLAIN
    if setting == "nw4":          # 4 waves where the default dispatch takes the two-tile kernel; never the 8-wave plain loop
        return Q2_4 if shape in Q2_SHAPES else PLAIN
    return Q2_8 if setting == "q2" else Q2_4


def _knob(name):
    from gaussianip_amd import _lib
    return ctypes.c_int.in_dll(_lib.nn_lib()._lib, "gip_dbg_attn_" + name)


@contextlib.contextmanager
def knobs(qt=-1, nw=-1):
    kq, kn = _knob("qt"), _knob("nw")
    kq.value, kn.value = qt, nw
    try:
        yield
    finally:
        kq.value = kn.value = -1


def attend(q, k, v, H, expect, k2=None, v2=None, w2=1.0):
    """fused.attention, twice (bitwise equal), asserting the kernel that ran and what the dispatch function says would run."""
    from gaussianip_amd import _lib
    from gaussianip_amd.guidance import fused
    B, Nq, C = q.shape
    D = C // H
    last = _knob("last_variant")
    last.value = -1
    assert fused.attention_supported(q, k, H)
    with torch.no_grad():
        o = fused.attention(q, k, v, H, k2, v2, w2)
        assert last.value == expect, (last.value, expect)
        assert _lib.nn_lib().gip_attention_variant(B, H, Nq, k.shape[1], D, 0 if k2 is None else k2.shape[1]) == expect
        SEEN.add((expect, D))
        assert torch.equal(fused.attention(q, k, v, H, k2, v2, w2), o), "the same call twice differs"
    return o


def close(o, ref):
    err = float((o.float() - ref.float()).abs().max())
    bar = 3e-3 * max(1.0, float(ref.abs().max()))
    return err <= bar, (err, bar)


def within_one_half_rounding(a, b):
    """Every element of the half tensors a, b equal or neighbouring halves (their sign-magnitude bit patterns, read as integers
    that grow with the value, differ by at most 1)."""
    def ordinal(h):
        i = h.contiguous().view(torch.int16).int()
        return torch.where(i < 0, -(i & 0x7fff), i)
    return bool(((ordinal(a) - ordinal(b)).abs() <= 1).all())


@functools.lru_cache(maxsize=None)
def case(gen, B, H, Nq, Nkv, D=40):
    """-> q, k, v on the GPU and the float32 reference (computed once, shared by the tests, never written).  The planted
    generators' condition — the float64 softmax is (one-, two-)hot to 0.999 — is asserted here, before any kernel is judged."""
    if gen in ("random1", "random6"):
        q, k, v = ai.random(B, H, Nq, Nkv, D, float(gen[-1]))
    elif gen == "planted":
        q, k, v, t = ai.planted(B, H, Nq, Nkv, D, off=max(0, Nkv - Nq))      # Nq < Nkv: the LAST Nq keys are the targets
    elif gen == "two_hot":
        q, k, v, ta, tb = ai.two_hot(B, H, Nq, Nkv, D)
    elif gen == "staircase":
        q, k, v = ai.staircase(B, H, Nq, Nkv, D)
    else:
        q, k, v = ai.constant(B, H, Nq, Nkv, D)
    q, k, v = q.cuda(), k.cuda(), v.cuda()
    if gen == "planted":
        lo, _ = ai.target_probability(q, k, H, t)
        assert lo >= 0.999, lo
    if gen == "two_hot":
        lo, imbalance = ai.target_probability(q, k, H, ta, tb)
        assert lo >= 0.999 and imbalance <= 1e-9 and int((ta != tb).sum()) >= B * H * Nq // 2, (lo, imbalance)
    ref = v.float().mean(dim=1, keepdim=True).expand(B, Nq, H * D) if gen == "constant" else ai.reference(q, k, v, H)
    return q, k, v, ref


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    yield
    case.cache_clear()
    two_set_case.cache_clear()


# ---- 1. the two-tile kernel by default dispatch -------------------------------------------------------------------------------------

@pytest.mark.parametrize("gen", GENERATORS)
@pytest.mark.parametrize("shape", Q2_SHAPES)
def test_q2_kernel_by_default_dispatch(shape, gen):
    B, H, Nq, Nkv = shape
    q, k, v, ref = case(gen, *shape)
    ok, figures = close(attend(q, k, v, H, Q2_8), ref)
    assert ok, figures
    if gen == "planted" and Nq < Nkv:
        # 64 queries cannot aim at 1061 keys at once: a few more windows of targets, the first keys included
        for off in (0, 509, Nkv - Nq - 1):
            qo, ko, vo, t = [x.cuda() for x in ai.planted(B, H, Nq, Nkv, 40, off=off)]
            assert ai.target_probability(qo, ko, H, t)[0] >= 0.999
            ok, figures = close(attend(qo, ko, vo, H, Q2_8), ai.reference(qo, ko, vo, H))
            assert ok, (off, figures)


@pytest.mark.parametrize("pad", [0, 64])
@pytest.mark.parametrize("shape", Q2_SHAPES)
def test_q2_kernel_reads_q_k_v_as_column_ranges_of_one_matrix(shape, pad):
    """q, k, v as column ranges of rows 3C (+ 64) halves long (the fused q | k | v projection: ld_q = ld_kv = the row length; the
    query and key counts differ here, so q's rows are one tensor and k's and v's another of the same row length) give the bits
    of the packed call."""
    from gaussianip_amd import _lib
    B, H, Nq, Nkv = shape
    C = H * 40
    for gen in ("planted", "random1"):
        q, k, v, ref = case(gen, *shape)
        packed = attend(q, k, v, H, Q2_8)
        g = torch.Generator(device="cuda").manual_seed(5)
        wq = torch.randn(B, Nq, 3 * C + pad, device="cuda", generator=g).half()          # what lies between the ranges is not read
        wkv = wq if Nq == Nkv else torch.randn(B, Nkv, 3 * C + pad, device="cuda", generator=g).half()
        off = pad // 2                                                                   # 32 halves: still 16-byte aligned
        wq[:, :, off:off + C] = q
        wkv[:, :, C + off:2 * C + off] = k
        wkv[:, :, 2 * C + pad:3 * C + pad] = v
        qs, ks, vs = wq[:, :, off:off + C], wkv[:, :, C + off:2 * C + off], wkv[:, :, 2 * C + pad:3 * C + pad]
        assert not qs.is_contiguous() and not ks.is_contiguous()
        before = _lib.call_counts.get("gip_attention_fwd_strided2_f16", 0)
        strided = attend(qs, ks, vs, H, Q2_8)
        assert _lib.call_counts.get("gip_attention_fwd_strided2_f16", 0) - before == 2      # in place: attend() calls twice
        assert torch.equal(strided, packed), gen
        ok, figures = close(strided, ref)
        assert ok, figures


# ---- 2. shapes that narrowly miss it -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("gen", GENERATORS)
@pytest.mark.parametrize("shape", NEAR_MISSES)
def test_shapes_that_narrowly_miss_the_q2_kernel_take_the_plain_loop(shape, gen):
    q, k, v, ref = case(gen, *shape)
    ok, figures = close(attend(q, k, v, shape[1], PLAIN), ref)
    assert ok, figures


# ---- 3. forced variants ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("gen", GENERATORS)
@pytest.mark.parametrize("shape", Q2_SHAPES + SMALL_GRIDS)
def test_forced_variants_match_the_reference_and_the_plain_loop_bit_for_bit(shape, gen):
    """attention.hip: "same arithmetic per (query, key): bit-identical outputs" — plain loop, 8-wave plain loop and the two-tile
    kernel with 8 and 4 waves on the same inputs."""
    H = shape[1]
    q, k, v, ref = case(gen, *shape)
    outs = {}
    for setting, (qt, nw) in SETTINGS.items():
        with knobs(qt, nw):
            outs[setting] = attend(q, k, v, H, expected_variant(setting, shape))
        ok, figures = close(outs[setting], ref)
        assert ok, (setting, figures)
    assert _knob("qt").value == -1 and _knob("nw").value == -1
    for setting, o in outs.items():
        assert torch.equal(o, outs["plain"]), (setting, float((o.float() - outs["plain"].float()).abs().max()))


# ---- 4. / 5. a second key set ------------------------------------------------------------------------------------------------------

def two_set_inputs(gen, B, H, Nq, Nkv, Nkv2, D):
    """-> q, (k, v), (k2, v2) on the CPU.  first / second: the queries are planted on the keys of that set (the other set holds
    unrelated planted keys: a diffuse softmax).  both: set 2 repeats set 1's key rows (row j = row j mod Nkv, own values), so query i
    is one-hot on key i mod Nkv of set 1 and on every key j = i (mod Nkv) of set 2 — two keys in different blocks where
    Nkv2 > Nkv + 64 — and row 64 of set 2 is row 63 again: the query planted there is two-hot across the block boundary."""
    if gen == "random":
        q, k, v = ai.random(B, H, Nq, Nkv, D, 1.0)
        _, k2, v2 = ai.random(B, H, Nq, Nkv2, D, 1.0, seed=1)
    elif gen == "first":
        q, k, v, _ = ai.planted(B, H, Nq, Nkv, D, off=max(0, Nkv - Nq))
        _, k2, v2, _ = ai.planted(B, H, Nq, Nkv2, D, seed=1)
    elif gen == "second":
        q, k2, v2, _ = ai.planted(B, H, Nq, Nkv2, D, off=max(0, Nkv2 - Nq))
        _, k, v, _ = ai.planted(B, H, Nq, Nkv, D, seed=1)
    else:
        q, k, v, _ = ai.planted(B, H, Nq, Nkv, D)
        k2 = k[:, torch.arange(Nkv2) % Nkv].clone()
        if Nkv2 > 64:
            k2[:, 64] = k2[:, 63]
        v2 = ai.random(B, H, Nq, Nkv2, D, 1.0, seed=2)[2]
    return q, (k, v), (k2, v2)


@functools.lru_cache(maxsize=None)
def two_set_case(gen, B, H, Nq, Nkv, Nkv2, D):
    """-> q, k, v, k2, v2 on the GPU and the two float32 references softmax(q k^T) v and softmax(q k2^T) v2."""
    q, (k, v), (k2, v2) = two_set_inputs(gen, B, H, Nq, Nkv, Nkv2, D)
    q, k, v, k2, v2 = [t.cuda() for t in (q, k, v, k2, v2)]
    t = ai.planted_targets(Nq, Nkv, max(0, Nkv - Nq) if gen == "first" else 0)
    t2 = ai.planted_targets(Nq, Nkv2, max(0, Nkv2 - Nq))
    if gen in ("first", "both"):
        assert ai.target_probability(q, k, H, t)[0] >= 0.999
    if gen == "second":
        assert ai.target_probability(q, k2, H, t2)[0] >= 0.999
    if gen == "both" and Nkv2 > 64:
        lo, imbalance = ai.target_probability(q[:, 63:64], k2, H, torch.tensor([63]), torch.tensor([64]))
        assert lo >= 0.999 and imbalance <= 1e-9, (lo, imbalance)
    return q, k, v, k2, v2, ai.reference(q, k, v, H), ai.reference(q, k2, v2, H)


@pytest.mark.parametrize("Nkv2", [65, 128, 130])          # 65: one full block and a single live key in the second
@pytest.mark.parametrize("D", [40, 64, 80, 160])
def test_long_second_key_set(D, Nkv2):
    """attn_fwd_kernel<D, 2>: sdpa(q, k, v) + w2 * sdpa(q, k2, v2), two accumulators."""
    B, H, Nq, Nkv = 2, 2, 96, 77
    for gen in ("random", "first", "second", "both"):
        q, k, v, k2, v2, r1, r2 = two_set_case(gen, B, H, Nq, Nkv, Nkv2, D)
        for w2 in (0.5, 0.0):
            ok, figures = close(attend(q, k, v, H, SET2_LONG, k2, v2, w2), r1 + w2 * r2)
            assert ok, (gen, w2, figures)


def test_long_second_key_set_as_column_ranges():
    """k2 / v2 (and k / v) with rows ld_kv2 > C apart give the bits of the packed call."""
    B, H, Nq, Nkv, Nkv2, D = 2, 2, 96, 77, 130, 40
    C = H * D
    q, k, v, k2, v2, r1, r2 = two_set_case("both", B, H, Nq, Nkv, Nkv2, D)
    g = torch.Generator(device="cuda").manual_seed(6)
    wide = torch.randn(B, Nkv, 2 * C + 8, device="cuda", generator=g).half()
    wide2 = torch.randn(B, Nkv2, 3 * C + 64, device="cuda", generator=g).half()
    wide[:, :, :C], wide[:, :, C + 8:] = k, v
    wide2[:, :, C:2 * C], wide2[:, :, 2 * C + 64:] = k2, v2
    packed = attend(q, k, v, H, SET2_LONG, k2, v2, 0.5)
    strided = attend(q, wide[:, :, :C], wide[:, :, C + 8:], H, SET2_LONG, wide2[:, :, C:2 * C], wide2[:, :, 2 * C + 64:], 0.5)
    assert torch.equal(strided, packed)
    ok, figures = close(strided, r1 + 0.5 * r2)
    assert ok, figures


@pytest.mark.parametrize("Nkv", [77, 64])                 # first set ragged / a whole block
@pytest.mark.parametrize("D", [40, 64, 80, 160])
def test_short_second_key_set(D, Nkv):
    """attn_fwd_kernel<D, 1>: the second set's probabilities are scaled by w2 / l2 before their PV product and share the first
    set's accumulator.  64 keys is the last count it takes (asserted); 65 is the long kernel's."""
    B, H, Nq = 2, 2, 96
    for Nkv2 in (1, 4, 33, 64):
        for gen in ("random", "second", "both"):
            q, k, v, k2, v2, r1, r2 = two_set_case(gen, B, H, Nq, Nkv, Nkv2, D)
            ok, figures = close(attend(q, k, v, H, SET2_SMALL, k2, v2, 0.5), r1 + 0.5 * r2)
            assert ok, (Nkv2, gen, figures)
            # weight 0: the second set's probabilities are multiplied by 0 / l2 = 0 before the PV product, which then adds exact
            # zeros to the normalised accumulator of the first set: the one-set call's value to one rounding of the output.
            # Not its bits: the one-set kernel's O * (1 / l) goes to half in ONE instruction (v_fma_mixlo_f16: the exact product
            # rounded once), while here the product must first exist in float32 as the PV product's accumulator and is rounded
            # to half from there — on a few elements in 10^5 the two roundings land on neighbouring halves.
            one = attend(q, k, v, H, PLAIN)
            zero = attend(q, k, v, H, SET2_SMALL, k2, v2, 0.0)
            assert within_one_half_rounding(zero, one), (Nkv2, gen, float((zero.float() - one.float()).abs().max()))
    q, k, v, k2, v2, r1, r2 = two_set_case("random", B, H, Nq, Nkv, 65, D)
    attend(q, k, v, H, SET2_LONG, k2, v2, 0.5)


# ---- 6. constant scores ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Nkv", [1, 63, 65, 1061])
@pytest.mark.parametrize("D", [40, 64, 80, 160])
def test_constant_scores_give_the_mean_of_the_values(D, Nkv):
    """Equal key rows: every probability is 1 / Nkv whatever the query.  D = 40 and 80 take the denominator from the ones column
    of the PV product, D = 64 and 160 sum it in registers; past-the-end keys of the last block must add nothing to either."""
    B, H, Nq = 2, 2, 256
    q, k, v, ref = case("constant", B, H, Nq, Nkv, D)
    long_keys = D == 40 and Nkv >= 1024
    for setting, (qt, nw) in SETTINGS.items() if long_keys else [("default", (-1, -1))]:
        with knobs(qt, nw):
            o = attend(q, k, v, H, expected_variant(setting, (B, H, Nq, Nkv)) if long_keys else PLAIN)
        ok, figures = close(o, ref)
        assert ok, (setting, figures)


# ---- 7. argument checks ------------------------------------------------------------------------------------------------------------

def test_rejected_calls_return_1_and_write_nothing():
    from gaussianip_amd import _lib
    fn = _lib.nn_lib().gip_attention_fwd_strided2_f16
    B, H, D = 1, 2, 40
    C = H * D
    g = torch.Generator(device="cuda").manual_seed(7)
    q, k, v, k2, v2 = [torch.randn(B, 128, C, device="cuda", generator=g).half() for _ in range(5)]
    o = torch.full((B, 128, C), 7.0, device="cuda", dtype=torch.float16)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else None)  # noqa: E731

    def call(Nq=128, Nkv=128, D=D, k2=None, v2=None, Nkv2=0, ld_q=C, ld_kv=C, ld_kv2=C):
        return fn(p(q), p(k), p(v), p(o), B, H, Nq, Nkv, D, float(D) ** -0.5, p(k2), p(v2), Nkv2, 0.5, ld_q, ld_kv, ld_kv2, st)
    assert call() == 0                                          # the arguments every rejected call below departs from in one place
    torch.cuda.synchronize()
    assert float(o.min()) < 7.0
    o.fill_(7.0)
    last = _knob("last_variant")
    last.value = 77
    bad = [dict(Nq=0), dict(Nq=16), dict(Nq=48), dict(Nkv=0), dict(D=48), dict(ld_q=C - 8), dict(ld_q=C + 4), dict(ld_kv=C + 4),
           dict(ld_kv=C - 8), dict(k2=k2), dict(v2=v2), dict(k2=k2, v2=v2, Nkv2=0), dict(k2=k2, v2=v2, Nkv2=4, ld_kv2=C + 4)]
    for kw in bad:
        assert call(**kw) == 1, kw
        assert last.value == 77, kw
    torch.cuda.synchronize()
    assert bool((o == 7.0).all())


# ---- every instantiation ran -------------------------------------------------------------------------------------------------------

def test_every_kernel_instantiation_was_reported(request):
    """Runs last: the (variant, head dim) pairs gip_dbg_attn_last_variant reported above are all fifteen instantiations, so a
    change of the dispatch table cannot leave one of them without a test.  (With tests picked by -k or by id: no stranger.)"""
    assert SEEN <= ALL_INSTANTIATIONS, SEEN - ALL_INSTANTIATIONS
    picked = request.config.getoption("keyword") or any("::" in a for a in request.config.args)
    if not picked:
        assert SEEN == ALL_INSTANTIATIONS, sorted(ALL_INSTANTIATIONS - SEEN)
