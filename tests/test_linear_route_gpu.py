"""gemm256_linear (gemm.hip): the plain-GEMM entry with the N-tile width, the
K split, the stream-K tail and the residual operand, and the Linear routing of
dispatch.linear_mfma / models.unet built on it.

Kernel cases run through gemm256_linear_ex, which pins (bn, mode), at the
smallest shapes that cross every boundary: M in {1, 255, 256, 257, 300, 513}
(under, at and over one 256-row tile, three tiles), N in {64, 72, 320, 336,
960} (72: the masked 4-column groups of a partial fragment; 336: a second
block at every width), K in {64, 128, 320} (1, 2 and 5 K-tiles). Per case:

  * the fp64 reference under kernel_bounds' conv / GEMM bound with n = K + 1,
    the residual added to ref and |residual| to mag as conv_ref does; the
    running worst err / bound is printed with each case;
  * the allocator poisoned with NaN before each call (output, split-K slabs,
    stream-K slots), as test_gemm_ktile_gpu.py does;
  * two calls bit-identical.

Flag sets: none, all of (bias, SiLU, residual), and bias + residual (the
UNet's use), on every (bn, mode).
"""

import functools
from collections import Counter

import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

import kernel_bounds as kb
import module_refs as mr
from comfyui_distributed_amd.models import unet as U
from comfyui_distributed_amd.ops import dispatch

pytestmark = pytest.mark.gpu

BNS = (128, 256, 320)
NONE, ALL, BIAS_RES = (False, False, False), (True, True, True), \
    (True, False, True)
FLAGS = (NONE, ALL, BIAS_RES)

# (m, n, k): every M, N and K of the lists above at least once
PLAIN_SHAPES = ((1, 64, 64), (255, 72, 128), (256, 320, 320), (257, 336, 64),
                (300, 960, 128), (513, 72, 320))
# split-K: 5 K-tiles in 2 (3 + 2) and 3 (2 + 2 + 1) slices, 2 K-tiles in 2
SPLIT_SHAPES = ((300, 336, 320, 2), (513, 72, 320, 3), (257, 320, 128, 2))
# stream-K at m 513, n 336, k 320: 5 K-tiles per tile, the last 5 tiles (25
# units) cut into sk_wgs ranges. 8 ranges (4 3 3 3 3 3 3 3): tiles in 2 and 3
# pieces; 12 ranges (3 2 2 ...): tiles in 3 pieces; 3 ranges (9 8 8): whole
# tiles inside a range beside tiles cut in 2. test_sk_case_list checks this
# against the kernel's own walk.
SK_SHAPE = (513, 336, 320)
SK_WGS = (8, 12, 3)
SK_TAIL = 5


def _sk_dp(bn):
    m, n, _ = SK_SHAPE
    return -(-m // 256) * -(-n // bn) - SK_TAIL


def _cases():
    out = []
    for bn in BNS:
        for i, (m, n, k) in enumerate(PLAIN_SHAPES):
            for f in (FLAGS if i in (2, 5) else (FLAGS[i % 3],)):
                out.append((m, n, k, f, bn, "plain", 1))
        for m, n, k, s in SPLIT_SHAPES:
            for f in FLAGS:
                out.append((m, n, k, f, bn, "split", s))
        for wgs in SK_WGS:
            for f in FLAGS:
                out.append((*SK_SHAPE, f, bn, "sk", wgs))
    return out


CASES = _cases()
WORST = {}


def case_id(case):
    m, n, k, (b, s, r), bn, mode, arg = case
    return f"{m}x{n}x{k}-b{int(b)}s{int(s)}r{int(r)}-bn{bn}-{mode}{arg}"


@functools.lru_cache(maxsize=None)
def _problem(m, n, k):
    """CPU-seeded operands, bf16-exact fp32, and their device copies."""
    g = torch.Generator().manual_seed(m * 1000003 + n * 1009 + k)
    x = kb.bf16_exact(torch.randn(m, k, generator=g) / 4)
    w = kb.bf16_exact(torch.randn(n, k, generator=g) / 4)
    bias = kb.bf16_exact(torch.randn(n, generator=g))
    res = kb.bf16_exact(torch.randn(m, n, generator=g))
    dev = (x.to(kb.BF).cuda(), w.to(kb.BF).cuda(), bias.cuda(),
           res.to(kb.BF).cuda())
    return (x, w, bias, res), dev


@functools.lru_cache(maxsize=None)
def _reference(m, n, k, flags):
    """(ref, bound) fp64: linear_ref's terms, the residual as in conv_ref."""
    (x, w, bias, res), _ = _problem(m, n, k)
    has_bias, silu, has_res = flags
    xd, wd = x.double(), w.double()
    ref = xd @ wd.t()
    mag = xd.abs() @ wd.abs().t()
    if has_bias:
        ref = ref + bias.double()
        mag = mag + bias.double().abs()
    if not has_res:
        want = kb.linear_ref(x, w, bias if has_bias else None, silu=silu)
        if silu:
            ref = torch.nn.functional.silu(ref)
        assert torch.equal(ref, want[0])
        return want
    if silu:
        ref = torch.nn.functional.silu(ref)
    ref = ref + res.double()
    mag = mag + res.double().abs()
    bound = 2 * kb.U * ref.abs() + (1.1 if silu else 1.0) * (k + 1) \
        * 2.0 ** -23 * mag
    return ref, bound


def _allocs(case):
    m, n, k, _, bn, mode, arg = case
    allocs = [(m * n, kb.BF)]
    if mode == "split":
        allocs.append((arg * m * n, torch.float32))
    if mode == "sk":
        allocs.append(((arg + SK_TAIL - 1) * 256 * bn, torch.float32))
    return allocs


def poison(allocs):
    held = [torch.full((max(int(n), 1),), float("nan"), dtype=dt,
                       device="cuda") for n, dt in allocs]
    torch.cuda.synchronize()
    del held


def run(extmod, case):
    m, n, k, (has_bias, silu, has_res), bn, mode, arg = case
    _, (x, w, bias, res) = _problem(m, n, k)
    b = bias if has_bias else torch.empty(0, device="cuda")
    r = res if has_res else torch.empty(0, device="cuda", dtype=kb.BF)
    if mode == "sk":
        return extmod.gemm256_linear_ex(x, w, b, r, silu, bn, 1, _sk_dp(bn),
                                        arg)
    return extmod.gemm256_linear_ex(x, w, b, r, silu, bn, arg, 0, 0)


@pytest.fixture(scope="module")
def extmod():
    from comfyui_distributed_amd.ops import ext

    return ext.get_ext(required=True)


def test_case_list():
    ids = [case_id(c) for c in CASES]
    assert len(set(ids)) == len(ids)
    assert {c[0] for c in CASES} == {1, 255, 256, 257, 300, 513}
    assert {c[1] for c in CASES} == {64, 72, 320, 336, 960}
    assert {c[2] for c in CASES} == {64, 128, 320}
    for bn in BNS:
        for mode, args in (("plain", {1}), ("split", {2, 3}),
                           ("sk", set(SK_WGS))):
            mine = [c for c in CASES if c[4] == bn and c[5] == mode]
            assert {c[6] for c in mine} == args
            for arg in args:
                assert {c[3] for c in mine if c[6] == arg} == set(FLAGS)


def test_sk_case_list(extmod):
    """The pinned tails cut tiles as the docstring says, by the kernel's own
    walk (conv256_sk_segments runs SkSched's functions on the host)."""
    kt = SK_SHAPE[2] // 64
    pieces = {}
    for wgs in SK_WGS:
        segs = extmod.conv256_sk_segments(SK_TAIL, kt, 0, wgs)
        per_tile = Counter(t for _, t, _, _, slot in segs if slot >= 0)
        whole = sum(1 for s in segs if s[4] < 0)
        pieces[wgs] = (set(per_tile.values()), whole)
    assert 2 in pieces[8][0] and pieces[8][1] == 0
    assert max(pieces[12][0]) >= 3 and pieces[12][1] == 0
    assert pieces[3][1] >= 1 and 2 in pieces[3][0]
    for bn in BNS:
        assert _sk_dp(bn) >= 1  # a data-parallel tile beside the tail


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_linear_case(extmod, case):
    m, n, k, flags = case[:4]
    ref, bound = _reference(m, n, k, flags)
    allocs = _allocs(case)
    poison(allocs)
    y1 = run(extmod, case)
    poison(allocs[1:])      # y1 is held: the workspace alone
    y2 = run(extmod, case)
    assert y1.shape == (m, n) and y1.dtype == kb.BF
    ratio = kb.err_ratio(y1, ref, bound)
    WORST[case_id(case)] = ratio
    print(f"LINEAR_ROUTE {case_id(case)} err/bound {ratio:.4f} (worst so far "
          f"{max(WORST.values()):.4f})")
    kb.check(y1, ref, bound, case_id(case))
    assert torch.equal(y1, y2), "two calls differ"


@pytest.mark.parametrize("bn,mode,arg", [(320, "plain", 1), (256, "split", 3),
                                         (320, "sk", 12), (128, "sk", 3)])
def test_fused_residual_against_unfused(extmod, bn, mode, arg):
    """With p the fp32 value before the store (accumulators + bias), the
    unfused call returns u = rn(p) and the fused one f = rn(fl32(p + r)).
    So |f - (u + r)| <= |p - u| + |f - (p + r)| <= hulp(u) + hulp(p + r) +
    2^-24 |p + r|. Asserted as hulp(u) + hulp(top) + 2^-23 top with top the
    larger of |f| and |u + r|: p + r is within hulp(u) of u + r, so
    |p + r| <= 2 top and 2^-24 |p + r| <= 2^-23 top."""
    m, n, k = SK_SHAPE
    case_u = (m, n, k, (True, False, False), bn, mode, arg)
    case_f = (m, n, k, (True, False, True), bn, mode, arg)
    _, (_, _, _, res) = _problem(m, n, k)
    u = run(extmod, case_u).double().cpu()
    f = run(extmod, case_f).double().cpu()
    s = u + res.double().cpu()
    top = torch.maximum(f.abs(), s.abs()).clamp_min(2.0 ** -120)
    allowed = kb.hulp(u.abs().clamp_min(2.0 ** -120)) + kb.hulp(top) \
        + 2.0 ** -23 * top
    assert bool(((f - s).abs() <= allowed).all())
    assert not torch.equal(f, u)


@pytest.mark.parametrize("case", [
    (513, 336, 320, BIAS_RES, 320, "plain", 1),
    (513, 336, 320, BIAS_RES, 256, "split", 3),   # two kernels, slabs
    (513, 336, 320, ALL, 320, "sk", 12),          # two kernels, slots
], ids=case_id)
def test_under_graph_capture(extmod, case):
    """One call captured and replayed three times: each replay equals the
    eager result bit for bit."""
    eager = run(extmod, case)
    torch.cuda.synchronize()
    poison(_allocs(case))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = run(extmod, case)
    for _ in range(3):
        y.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, eager)


def test_chooser_is_the_pinned_call(extmod):
    """gemm256_linear equals the pinned call of gemm256_linear_plan's answer,
    and the flagship widths come out as the routing assumes: N = 320 one
    320-wide block, N = 960 three."""
    assert tuple(extmod.gemm256_linear_plan(147968, 320, 320))[:2] == (320, 1)
    assert tuple(extmod.gemm256_linear_plan(147968, 960, 320))[:2] == (320, 1)
    assert tuple(extmod.gemm256_linear_plan(147968, 320, 1280))[:2] == (320, 1)
    for m, n, k in ((513, 336, 320), (300, 960, 128), (2464, 640, 768)):
        g = torch.Generator().manual_seed(m + n + k)
        x = (torch.randn(m, k, generator=g) / 4).to(kb.BF).cuda()
        w = (torch.randn(n, k, generator=g) / 4).to(kb.BF).cuda()
        b = torch.randn(n, generator=g).cuda()
        r = torch.randn(m, n, generator=g).to(kb.BF).cuda()
        bn, split, dp, wgs = extmod.gemm256_linear_plan(m, n, k)
        y = extmod.gemm256_linear(x, w, b, r, False)
        if wgs:
            z = extmod.gemm256_linear_ex(x, w, b, r, False, bn, 1, dp, wgs)
        else:
            z = extmod.gemm256_linear_ex(x, w, b, r, False, bn, split, 0, 0)
        assert torch.equal(y, z)


def test_entry_rejects_bad_operands(extmod):
    _, (x, w, bias, res) = _problem(300, 336, 320)
    none = torch.empty(0, device="cuda", dtype=kb.BF)
    with pytest.raises(RuntimeError):
        extmod.gemm256_linear_ex(x, w, bias, res[:, :300], False, 0, 0, 0, 0)
    with pytest.raises(RuntimeError):
        extmod.gemm256_linear_ex(x, w, bias, none, False, 192, 0, 0, 0)
    with pytest.raises(RuntimeError):  # dp_tiles above the tile count
        extmod.gemm256_linear_ex(x, w, bias, none, False, 256, 1, 99, 4)
    with pytest.raises(RuntimeError):
        extmod.gemm256_linear_ex(x[:, :100].contiguous(), w, bias, none,
                                 False, 0, 0, 0, 0)


# ---------------------------------------------------------------------------
# module level: TransformerBlock and SpatialTransformer at dim 320, 8 heads of
# 40, an 18x18 token grid, batch 2 (M = 648), with every Linear of theirs
# that has a flagship route sent to the kernel at this M
# ---------------------------------------------------------------------------

RMS_LIMIT, MAX_LIMIT = 2.0, 3.0   # test_module_bounds_gpu.py's multiples

TEST_ROUTES = (
    (320, 320, 1, 10 ** 6, True),    # to_q, to_out, proj_in, proj_out
    (320, 960, 1, 10 ** 6, True),    # fused QKV
    (1280, 320, 1, 10 ** 6, True),   # feed-forward proj_out
    (768, 640, 1, 10 ** 6, True),    # fused KV of the context
)

TB_CASE = mr.Case(
    "tblock320_routed", lambda: U.TransformerBlock(320, 768, 8, 40),
    lambda: (mr.randn_bf16(21, 2, 324, 320), mr.randn_bf16(22, 2, 77, 768)),
    lambda P, x, ctx, rnd=mr.ident, defect=None: mr.transformer_block_ref(
        P, x, ctx, 8, rnd, defect),
    {"layer_norm": 3, "attn_fwd_qkv": 1, "attn_fwd_q_kv": 1, "act_mul": 1,
     "gemm256_linear": 6}, branch=True)
ST_CASE = mr.Case(
    "st320_routed", lambda: U.SpatialTransformer(320, 768, 8, 40),
    lambda: (mr.randn_bf16(23, 2, 320, 18, 18),
             mr.randn_bf16(24, 2, 77, 768)),
    lambda P, x, ctx, rnd=mr.ident, defect=None: mr.spatial_transformer_ref(
        P, x, ctx, 8, rnd, defect),
    {"group_norm_nhwc": 1, "layer_norm": 3, "attn_fwd_qkv": 1,
     "attn_fwd_q_kv": 1, "act_mul": 1, "gemm256_linear": 8}, branch=True)


@functools.lru_cache(maxsize=None)
def _case_data(name):
    case = {c.name: c for c in (TB_CASE, ST_CASE)}[name]
    module = mr.seeded(case.build, 1000 + len(name))
    inputs = case.inputs()
    mr.check_inputs(inputs)
    P = mr.params_of(module)
    with torch.no_grad():
        ref, inter_ref = case.ref(P, *mr.to64(inputs), rnd=mr.ident)
        yard, inter_yard = case.ref(P, *mr.to64(inputs), rnd=mr.bf16)
    return mr.CaseData(case, module, inputs, ref, yard, inter_ref, inter_yard,
                       P)


class _Proxy:
    def __init__(self, mod, counter):
        self._mod, self._counter = mod, counter

    def __getattr__(self, name):
        fn = getattr(self._mod, name)
        if not callable(fn):
            return fn

        def counted(*args, **kwargs):
            self._counter[name] += 1
            return fn(*args, **kwargs)

        return counted


class _AddCounter(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.adds = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        if func in (torch.ops.aten.add.Tensor, torch.ops.aten.add_.Tensor):
            self.adds += 1
        return func(*args, **(kwargs or {}))


@pytest.mark.parametrize("name", ["tblock320_routed", "st320_routed"])
def test_module_on_the_linear_route(name, monkeypatch):
    import copy

    cd = _case_data(name)
    monkeypatch.setattr(dispatch, "_GEMM256", True)
    monkeypatch.setattr(dispatch, "_LINEAR_ROUTES", TEST_ROUTES)
    counter = Counter()
    real = dispatch.ext.get_ext
    monkeypatch.setattr(
        dispatch.ext, "get_ext",
        lambda required=None: _Proxy(real(required), counter))
    module = copy.deepcopy(cd.module).to(mr.BF).cuda()
    inputs = []
    for t in cd.inputs:
        t = t.to(mr.BF).cuda()
        if t.dim() == 4:
            t = t.contiguous(memory_format=torch.channels_last)
        inputs.append(t)
    with torch.no_grad(), _AddCounter() as adds:
        y = cd.forward(module, inputs)
    torch.cuda.synchronize()
    assert y.dtype == mr.BF and y.shape == cd.ref.shape
    assert dict(counter) == cd.case.routes
    # the skip adds went into epilogues: attn1, attn2, ff (+ proj_out)
    assert adds.adds == 0
    got, yard = cd.metrics(y), cd.yard_metrics()
    for key, (e_rms, e_max) in got.items():
        r_rms, r_max = e_rms / yard[key][0], e_max / yard[key][1]
        print(f"LINEAR_ROUTE {name} {key} e_rms_ratio {r_rms:.3f} "
              f"e_max_ratio {r_max:.3f}")
        assert r_rms <= RMS_LIMIT and r_max <= MAX_LIMIT, (key, r_rms, r_max)


def test_module_unfused_site_keeps_its_add(monkeypatch):
    """A routed row with fuse False: the product on the kernel, the residual
    by a separate add, and the same result as the product call plus the add."""
    monkeypatch.setattr(dispatch, "_GEMM256", True)
    monkeypatch.setattr(dispatch, "_LINEAR_ROUTES",
                        ((320, 336, 1, 10 ** 6, False),))
    _, (x, w, bias, res) = _problem(300, 336, 320)
    with _AddCounter() as adds:
        y = dispatch.linear_mfma(x, w, bias.to(kb.BF), residual=res)
    assert adds.adds == 1
    z = dispatch.linear_mfma(x, w, bias.to(kb.BF)) + res
    assert torch.equal(y, z)
    # a fused row and a residual that is not the output's shape (a row
    # vector) or dtype: the separate add, as on the hipBLASLt path
    monkeypatch.setattr(dispatch, "_LINEAR_ROUTES",
                        ((320, 336, 1, 10 ** 6, True),))
    prod = dispatch.linear_mfma(x, w, bias.to(kb.BF))
    assert torch.equal(dispatch.linear_mfma(x, w, bias.to(kb.BF),
                                            residual=res[0]), prod + res[0])
    assert torch.equal(dispatch.linear_mfma(x, w, bias.to(kb.BF),
                                            residual=res.float()),
                       prod + res.float())
    monkeypatch.setattr(dispatch, "_GEMM256", False)
    lt = torch.nn.functional.linear(x, w, bias.to(kb.BF)) + res
    assert torch.equal(dispatch.linear_mfma(x, w, bias.to(kb.BF),
                                            residual=res), lt)
