"""UNet glue kernels on the GPU: the two-pass NHWC GroupNorm (thread-fixed
channel slots, partial sums without atomics, optional per-sample addend), the
parameter handling of the three norm launchers, and act_mul on row-strided
operands.

References and bounds are those of kernel_bounds (fp64 from the bf16-exact
inputs; 2U*|ref| + 2^-16*mag for GroupNorm, (2U + 2^-16)*|ref| for act_mul).
Before every kernel call the caching allocator is poisoned: NaN-filled
tensors of the sizes the call allocates are created and freed, so the call's
torch::empty buffers come back holding NaN and a partial-sum entry that the
stats pass leaves unwritten reaches the output.
"""

import functools

import pytest
import torch

import kernel_bounds as kb

pytestmark = pytest.mark.gpu

EPS = 1e-5


@pytest.fixture(scope="module")
def extmod():
    from comfyui_distributed_amd.ops import ext

    return ext.get_ext(required=True)


def _poison(*specs):
    """specs: (numel, dtype). Allocate all, fill with NaN, free all."""
    held = [torch.full((max(int(n), 1),), float("nan"), dtype=dt,
                       device="cuda") for n, dt in specs]
    torch.cuda.synchronize()
    del held


def _gn_poison(extmod, shape, groups):
    b, c, h, w = shape
    plan = extmod.group_norm_nhwc_plan(b, h * w, c)
    bpi = plan[3]
    _poison((b * c * h * w, kb.BF), (b * bpi * groups * 2, torch.float32),
            (b * groups * 2, torch.float32))


def _nhwc(x_nchw):
    return x_nchw.permute(0, 2, 3, 1).contiguous().to(kb.BF).cuda()


# (shape NCHW, G): the path each reaches is named in GN_WHY
GN_CASES = [
    ((2, 320, 7, 9), 32),
    ((1, 960, 3, 5), 32),
    ((1, 1920, 2, 3), 32),
    ((1, 2560, 3, 3), 32),
    ((1, 128, 5, 7), 32),
    ((1, 512, 3, 3), 64),
    ((3, 320, 40, 40), 32),
    ((1, 640, 5, 5), 32),
]
GN_WHY = {
    (2, 320, 7, 9): "HW = 63 is no multiple of the 6 pixels of a block step",
    (1, 960, 3, 5): "Cg = 30, concat width",
    (1, 1920, 2, 3): "Cg = 60, concat width",
    (1, 2560, 3, 3): "V = 320 slots for 160 lanes: two slots per lane",
    (1, 128, 5, 7): "Cg = 4: a vector is two whole groups",
    (1, 512, 3, 3): "G = 64, the group-count limit",
    (3, 320, 40, 40): "many blocks per image, three images",
    (1, 640, 5, 5): "by the launcher's rule, blocks with an empty stripe",
}
EMPTY_STRIPE_SHAPE = (1, 640, 5, 5)


@functools.lru_cache(maxsize=None)
def _gn_case(shape, groups):
    """Inputs and the fp64 references (SiLU off, on), computed once."""
    x, w, b = kb.norm_inputs(sum(shape) + groups, shape)
    refs = {silu: kb.group_norm_ref(x, groups, w, b, EPS, silu)
            for silu in (False, True)}
    return x, w, b, refs


def _nchw(y_nhwc):
    return y_nhwc.permute(0, 3, 1, 2)


def test_gn_plan_rules(extmod):
    """The launcher's rule as the tests rely on it: the block step of each
    case, and that EMPTY_STRIPE_SHAPE has stats blocks past the image's last
    pixel ((bpi - 1) * ppb >= HW)."""
    threads, p, ns, bpi, ppb = extmod.group_norm_nhwc_plan(2, 63, 320)
    assert (threads, p, ns) == (256, 6, 1) and 63 % p != 0
    assert ppb % p == 0 and bpi * ppb >= 63
    threads, p, ns, bpi, ppb = extmod.group_norm_nhwc_plan(1, 9, 2560)
    assert (threads, p, ns) == (192, 1, 2)      # 160 lanes, slots t and t+160
    b, c, h, w = EMPTY_STRIPE_SHAPE
    threads, p, ns, bpi, ppb = extmod.group_norm_nhwc_plan(b, h * w, c)
    assert ppb % p == 0 and bpi * ppb >= h * w
    assert (bpi - 1) * ppb >= h * w, (bpi, ppb)  # the last block is empty
    threads, p, ns, bpi, ppb = extmod.group_norm_nhwc_plan(3, 1600, 320)
    assert bpi > 100 and -(-1600 // ppb) > 100   # many live blocks per image
    # the flagship's own launches: at most 64 blocks per image at B = 32
    for hw, c in ((4624, 320), (1156, 640), (289, 1280), (81, 2560)):
        threads, p, ns, bpi, ppb = extmod.group_norm_nhwc_plan(32, hw, c)
        assert bpi * 32 <= 2048 and bpi * ppb >= hw


@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("shape,groups", GN_CASES)
def test_gn_nhwc_two_pass(extmod, shape, groups, silu):
    x, w, b, refs = _gn_case(shape, groups)
    ref, bound = refs[silu]
    xd, wd, bd = _nhwc(x), w.cuda(), b.cuda()
    _gn_poison(extmod, shape, groups)
    y1 = extmod.group_norm_nhwc(xd, groups, wd, bd, EPS, silu)
    _gn_poison(extmod, shape, groups)
    y2 = extmod.group_norm_nhwc(xd, groups, wd, bd, EPS, silu)
    kb.check(_nchw(y1), ref, bound,
             f"gn_nhwc {shape} G={groups} silu={silu} ({GN_WHY[shape]})")
    assert torch.equal(y1, y2), "two calls on one input differ"


def test_gn_nhwc_graph_replay(extmod):
    shape, groups = (3, 320, 40, 40), 32
    x, w, b, refs = _gn_case(shape, groups)
    xd, wd, bd = _nhwc(x), w.cuda(), b.cuda()
    _gn_poison(extmod, shape, groups)
    eager = extmod.group_norm_nhwc(xd, groups, wd, bd, EPS, True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = extmod.group_norm_nhwc(xd, groups, wd, bd, EPS, True)
    for i in range(3):
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager), f"replay {i} differs from eager"
    kb.check(_nchw(out), *refs[True], "gn_nhwc graph replay")


def _gn_addend_check(extmod, shape, groups, silu):
    c = shape[1]
    x, w, b = kb.norm_inputs(11 + c, shape)
    g = torch.Generator().manual_seed(12 + c)
    add = torch.randn(shape[0], c, generator=g).to(kb.BF)
    xd, wd, bd, ad = _nhwc(x), w.cuda(), b.cuda(), add.cuda()
    summed = (xd + ad[:, None, None, :]).contiguous()
    assert summed.dtype == kb.BF
    _gn_poison(extmod, shape, groups)
    fused = extmod.group_norm_nhwc(xd, groups, wd, bd, EPS, silu, ad)
    _gn_poison(extmod, shape, groups)
    plain = extmod.group_norm_nhwc(summed, groups, wd, bd, EPS, silu)
    assert torch.equal(fused, plain)
    ref, bound = kb.group_norm_ref(_nchw(summed.float().cpu()), groups, w, b,
                                   EPS, silu)
    kb.check(_nchw(fused), ref, bound,
             f"gn_nhwc addend {shape} G={groups} silu={silu}")


@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("c", [320, 1280])
def test_gn_nhwc_addend(extmod, c, silu):
    """group_norm_nhwc(x, addend) is bit-identical to the kernel run on
    torch's bf16 sum x + addend[:, None, None, :], and inside the bound of
    the reference on that sum. B = 3: a wrong batch index shows."""
    _gn_addend_check(extmod, (3, c, 5, 7), 32, silu)


@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("shape,groups", [((3, 64, 3, 3), 32),
                                          ((2, 576, 3, 3), 72)])
def test_gn_nhwc_addend_per_group(extmod, shape, groups, silu):
    """The same on the shapes the per-(n, g) kernel takes (Cg = 2; G > 64),
    where the launcher forms x + addend itself."""
    _gn_addend_check(extmod, shape, groups, silu)


@pytest.mark.parametrize("silu", [False, True])
def test_gn_nhwc_addend_unaligned(extmod, silu):
    """A contiguous addend that starts 8 bytes past a 16-byte boundary: the
    launcher copies it for the two-pass kernels' 16-byte loads, and the result
    is that of the aligned addend."""
    shape, groups = (3, 320, 5, 7), 32
    b, c = shape[:2]
    x, w, bias = kb.norm_inputs(21 + c, shape)
    g = torch.Generator().manual_seed(22 + c)
    ad = torch.randn(b, c, generator=g).to(kb.BF).cuda()
    buf = torch.zeros(b * c + 8, dtype=kb.BF, device="cuda")
    shifted = buf[4:4 + b * c].view(b, c)
    shifted.copy_(ad)
    assert ad.data_ptr() % 16 == 0
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 == 8
    xd, wd, bd = _nhwc(x), w.cuda(), bias.cuda()
    _gn_poison(extmod, shape, groups)
    want = extmod.group_norm_nhwc(xd, groups, wd, bd, EPS, silu, ad)
    _gn_poison(extmod, shape, groups)
    got = extmod.group_norm_nhwc(xd, groups, wd, bd, EPS, silu, shifted)
    assert torch.equal(got, want)


# ---------------------------------------------------------------------------
# weight / bias handed straight to the three norm launchers
# ---------------------------------------------------------------------------

PARAM_GN = ((2, 320, 7, 9), 32)
PARAM_LN = (5, 324)


@functools.lru_cache(maxsize=None)
def _ln_case():
    x, w, b = kb.norm_inputs(PARAM_LN[1], PARAM_LN)
    return x, w, b, kb.layer_norm_ref(x, w, b, EPS)


def _param_case(extmod, launcher):
    """(call, w, b, (ref, bound)) for one launcher: call(w, b) runs it on the
    case's x and returns the output in the reference's layout; w, b are the
    fp32 parameters on the CPU."""
    if launcher == "layer_norm":
        x, w, b, refs = _ln_case()
        xd = x.to(kb.BF).cuda()
        return (lambda w, b: extmod.layer_norm(xd, w, b, EPS)), w, b, refs
    groups = PARAM_GN[1]
    x, w, b, refs = _gn_case(*PARAM_GN)
    if launcher == "group_norm_fused":
        xd = x.to(kb.BF).cuda()
        return (lambda w, b: extmod.group_norm_fused(xd, groups, w, b, EPS,
                                                     True)), w, b, refs[True]
    xd = _nhwc(x)
    return (lambda w, b: _nchw(extmod.group_norm_nhwc(xd, groups, w, b, EPS,
                                                      True))), w, b, refs[True]


LAUNCHERS = ["group_norm_fused", "group_norm_nhwc", "layer_norm"]


@pytest.mark.parametrize("launcher", LAUNCHERS)
def test_norm_bf16_params(extmod, launcher):
    """bf16 weight/bias: the launcher casts them, and gives what it gives for
    the fp32 copy of the same values."""
    call, w, b, _ = _param_case(extmod, launcher)
    wh, bh = w.to(kb.BF).cuda(), b.to(kb.BF).cuda()
    assert torch.equal(call(wh, bh), call(wh.float(), bh.float()))


@pytest.mark.parametrize("launcher", LAUNCHERS)
def test_norm_rejects_bad_params(extmod, launcher):
    """A weight of C - 1 elements, or one in host memory, is an error raised
    before anything is launched: the next correct call is inside its bound."""
    call, w, b, (ref, bound) = _param_case(extmod, launcher)
    wd, bd = w.cuda(), b.cuda()
    with pytest.raises(RuntimeError):
        call(wd[:-1].contiguous(), bd)
    with pytest.raises(RuntimeError):
        call(w, bd)
    kb.check(call(wd, bd), ref, bound, f"{launcher} after rejected calls")


# ---------------------------------------------------------------------------
# act_mul on row-strided operands
# ---------------------------------------------------------------------------

BIG = 64.0 * kb.FILLER   # what the half that is not being read holds


@functools.lru_cache(maxsize=None)
def _am_case(shape):
    a, b = kb.act_mul_inputs(sum(shape), shape)
    refs = {gelu: kb.act_mul_ref(a, b, gelu) for gelu in (False, True)}
    return a, b, refs


def _halves(a, b):
    """a and b as the chunk(2, -1) halves of two parent buffers [..., 2*I];
    in each buffer the other half holds BIG, so a read across the split
    shows. Returns (a_view, b_view): a is a first half, b a second half."""
    shape = list(a.shape)
    shape[-1] *= 2
    buf_a = torch.full(shape, BIG, dtype=kb.BF, device="cuda")
    buf_b = torch.full(shape, BIG, dtype=kb.BF, device="cuda")
    va = buf_a.chunk(2, dim=-1)[0]
    vb = buf_b.chunk(2, dim=-1)[1]
    va.copy_(a.to(kb.BF))
    vb.copy_(b.to(kb.BF))
    return va, vb


def _am_check(extmod, va, vb, a, refs, gelu, what):
    assert not va.is_contiguous() and not vb.is_contiguous()
    _poison((a.numel(), kb.BF))
    y = extmod.act_mul(va, vb, gelu)
    _poison((a.numel(), kb.BF))
    yc = extmod.act_mul(va.contiguous(), vb.contiguous(), gelu)
    assert y.is_contiguous() and y.shape == va.shape
    assert torch.equal(y, yc), f"{what}: strided and copied operands differ"
    kb.check(y, *refs[gelu], f"act_mul {what} gelu={gelu}")


# (2, 77, 1280) and (3, 5, 5120): in place. (5, 1003): the second half starts
# 1003 elements in, not 16-byte aligned -> copy path. (2053, 2048): 525 568
# vectors, more than the 2048 * 256 of one grid: a second trip.
@pytest.mark.parametrize("gelu", [True, False])
@pytest.mark.parametrize("shape", [(2, 77, 1280), (3, 5, 5120), (5, 1003),
                                   (2053, 2048)])
def test_act_mul_halves(extmod, shape, gelu):
    assert shape != (2053, 2048) or 2053 * 2048 > kb.ACT_MUL_GRID
    a, b, refs = _am_case(shape)
    # both operands out of ONE buffer, as GEGLUFeedForward hands them over
    buf = torch.empty(*shape[:-1], 2 * shape[-1], dtype=kb.BF, device="cuda")
    va, vb = buf.chunk(2, dim=-1)
    va.copy_(a.to(kb.BF))
    vb.copy_(b.to(kb.BF))
    _am_check(extmod, va, vb, a, refs, gelu, f"halves of one {shape}")
    # and out of two buffers whose other half holds BIG
    if shape != (2053, 2048):
        va, vb = _halves(a, b)
        _am_check(extmod, va, vb, a, refs, gelu, f"halves {shape}, filler")


@pytest.mark.parametrize("gelu", [True, False])
def test_act_mul_odd_pitch(extmod, gelu):
    """Aligned start, row pitch 1284 (no multiple of 8): the copy path."""
    shape = (5, 1280)
    a, b, refs = _am_case(shape)
    buf_a = torch.full((5, 1284), BIG, dtype=kb.BF, device="cuda")
    buf_b = torch.full((5, 1284), BIG, dtype=kb.BF, device="cuda")
    va, vb = buf_a[:, :1280], buf_b[:, :1280]
    assert va.storage_offset() % 8 == 0 and va.stride(0) % 8 != 0
    va.copy_(a.to(kb.BF))
    vb.copy_(b.to(kb.BF))
    _am_check(extmod, va, vb, a, refs, gelu, "pitch 1284")
