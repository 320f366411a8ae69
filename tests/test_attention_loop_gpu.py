"""GPU numerics for the flash-attention tile loop: K staged through LDS,
P kept in registers (V^T keys permuted), exp2-domain softmax with defer-max,
key-tail masking on the last tile only, lane-local row sums, per-XCD
workgroup renumbering.

Reference everywhere: the CPU fp32 path of ``dispatch.attention*`` on the
same bf16-rounded inputs the kernel sees. Bounds as in test_ops_gpu.py:
0.03 max abs error, 0.05 where the defer-max path is forced, 0.01 for the
uniform-V row-sum check. Every comparison also goes through the per-element
attention bound of kernel_bounds.py (fp64 reference, bound that scales with
the output), which prints max(err / bound).
"""

import math

import pytest
import torch

import kernel_bounds as kb

pytestmark = pytest.mark.gpu

KT = 64  # keys per tile in the kernel


@pytest.fixture(scope="module")
def extmod():
    from comfyui_distributed_amd.ops import ext

    return ext.get_ext(required=True)


def _bf16(x):
    return x.to(torch.bfloat16)


def _round(x):
    """fp32 tensor holding exactly the values the bf16 kernel input has."""
    return x.to(torch.bfloat16).float()


def test_one_hot_key_sweep(extmod):
    """Query row i puts (nearly) all its weight on key i % Nk, so the output
    row is that key's V row: a key that lands in the wrong PV k-slot, in
    either full tile or in the 22-key tail, returns another key's V."""
    from comfyui_distributed_amd.ops import dispatch

    torch.manual_seed(40)
    bh, nq, nk, d = 2, 160, 150, 40
    k = torch.nn.functional.normalize(torch.randn(bh, nk, d), dim=-1)
    tgt = torch.arange(nq) % nk
    q = _round(250.0 * k[:, tgt])
    k = _round(k)
    v = _round(torch.randn(bh, nk, d))

    w = torch.softmax(torch.bmm(q, k.transpose(1, 2)) / math.sqrt(d), dim=-1)
    w_tgt = w[:, torch.arange(nq), tgt]
    assert w_tgt.min().item() >= 0.999, w_tgt.min().item()
    assert set(tgt.tolist()) == set(range(nk))  # every column of every tile

    ref = dispatch.attention(q, k, v, heads=1)
    out = dispatch.attention(_bf16(q).cuda(), _bf16(k).cuda(), _bf16(v).cuda(),
                             heads=1).float().cpu()
    err = (out - ref).abs().max().item()
    print(f"one-hot sweep: min target weight {w_tgt.min().item():.6f} "
          f"max err {err:.5f}")
    assert err < 0.03, f"one-hot key sweep err {err}"
    ref64, bound = kb.attention_ref(q, k, v)
    kb.check(out, ref64, bound, "one-hot sweep")


@pytest.mark.parametrize("d", [40, 64, 80, 128, 160])
@pytest.mark.parametrize("nk", [1, 13, 63, 64, 65, 77, 128, 141])
def test_tail_and_no_tail(extmod, d, nk):
    from comfyui_distributed_amd.ops import dispatch

    torch.manual_seed(d * 1000 + nk)
    bh, nq = 4, 40
    q = _round(torch.randn(bh, nq, d) / 2)
    k = _round(torch.randn(bh, nk, d) / 2)
    v = _round(torch.randn(bh, nk, d))
    ref = dispatch.attention(q, k, v, heads=2)
    out = dispatch.attention(_bf16(q).cuda(), _bf16(k).cuda(), _bf16(v).cuda(),
                             heads=2).float().cpu()
    err = (out - ref).abs().max().item()
    print(f"tail d={d} nk={nk}: max err {err:.5f}")
    assert err < 0.03, f"max err {err} at d={d} nk={nk}"
    ref64, bound = kb.attention_ref(q, k, v, heads=2)
    kb.check(out, ref64, bound, f"tail d={d} nk={nk}")


def test_strided_fused_qkv(extmod):
    from comfyui_distributed_amd.ops import dispatch

    torch.manual_seed(21)
    b, n, h, d = 2, 100, 3, 40
    qkv = _round(torch.randn(b, n, 3 * h * d) / 2)
    ref = dispatch.attention_qkv(qkv, heads=h)
    out = dispatch.attention_qkv(_bf16(qkv).cuda(), heads=h).float().cpu()
    err = (out - ref).abs().max().item()
    print(f"fused qkv: max err {err:.5f}")
    assert err < 0.03, err
    ref64, bound = kb.attention_qkv_ref(qkv, heads=h)
    kb.check(out, ref64, bound, "fused qkv")


def test_strided_fused_q_kv(extmod):
    from comfyui_distributed_amd.ops import dispatch

    torch.manual_seed(22)
    b, nq, nk, h, d = 2, 100, 77, 3, 40
    q = _round(torch.randn(b, nq, h * d) / 2)
    kv = _round(torch.randn(b, nk, 2 * h * d) / 2)
    ref = dispatch.attention_q_kv(q, kv, heads=h)
    out = dispatch.attention_q_kv(_bf16(q).cuda(), _bf16(kv).cuda(),
                                  heads=h).float().cpu()
    err = (out - ref).abs().max().item()
    print(f"fused q+kv: max err {err:.5f}")
    assert err < 0.03, err
    ref64, bound = kb.attention_q_kv_ref(q, kv, heads=h)
    kb.check(out, ref64, bound, "fused q+kv")


def test_strided_gqa(extmod):
    from comfyui_distributed_amd.ops import dispatch

    torch.manual_seed(23)
    b, h, hkv, n, d = 2, 4, 2, 100, 40
    q = _round(torch.randn(b * h, n, d) / 2)
    k = _round(torch.randn(b * hkv, n, d) / 2)
    v = _round(torch.randn(b * hkv, n, d))
    ref = dispatch.attention(q, k, v, heads=h, kv_heads=hkv)
    out = dispatch.attention(_bf16(q).cuda(), _bf16(k).cuda(), _bf16(v).cuda(),
                             heads=h, kv_heads=hkv).float().cpu()
    err = (out - ref).abs().max().item()
    print(f"gqa: max err {err:.5f}")
    assert err < 0.03, err
    ref64, bound = kb.attention_ref(q, k, v, heads=h, kv_heads=hkv)
    kb.check(out, ref64, bound, "gqa")


@pytest.mark.parametrize("b,h", [(2, 8), (1, 24), (3, 3)])
def test_workgroup_renumbering(extmod, b, h):
    """Several q-blocks per head with B*H a multiple of 8 (workgroups are
    renumbered per XCD) and not (plain grid): every (head, q-block) pair
    must still be computed exactly once, on its own head's K/V."""
    from comfyui_distributed_amd.ops import dispatch

    torch.manual_seed(b * 100 + h)
    n, d = 300, 40  # 3 q-blocks of 128 rows, the last one partial
    qkv = _round(torch.randn(b, n, 3 * h * d) / 2)
    ref = dispatch.attention_qkv(qkv, heads=h)
    out = dispatch.attention_qkv(_bf16(qkv).cuda(), heads=h).float().cpu()
    err = (out - ref).abs().max().item()
    print(f"renumbering b={b} h={h}: max err {err:.5f}")
    assert err < 0.03, err
    ref64, bound = kb.attention_qkv_ref(qkv, heads=h)
    kb.check(out, ref64, bound, f"renumbering b={b} h={h}")


def _rescale_tiles(scores, row, thr=8.0):
    """Tiles at which the 16-row group (one wave) holding ``row`` rescales:
    any row of the group whose tile max exceeds its running max by more than
    ``thr`` makes the whole group take max(running, tile)."""
    g0 = (row // 16) * 16
    s = scores[g0:g0 + 16]
    m_run = torch.full((16,), -1e30)
    fired = []
    for t in range(s.shape[1] // KT):
        mt = s[:, t * KT:(t + 1) * KT].max(dim=1).values
        if ((mt - m_run) > thr).any():
            m_run = torch.maximum(m_run, mt)
            fired.append(t)
    return fired


def test_defer_max_staircase(extmod):
    """Rows 5, 21 and 130 see their tile maximum climb by ~6 per tile over
    the four tiles: no single step passes the defer threshold of 8, so the
    rescale has to fire on the growth accumulated since the last one (tile 2)
    with P as large as e^6 already summed in. Row 77 instead jumps by more
    than 8 in the last tile."""
    from comfyui_distributed_amd.ops import dispatch

    torch.manual_seed(64)
    bh, n, d = 2, 256, 64
    scale = 1.0 / math.sqrt(d)
    q = torch.randn(bh, n, d) / 4
    k = torch.randn(bh, n, d) / 4
    v = torch.randn(bh, n, d)
    stairs = {5: 3, 21: 9, 130: 40}  # row -> key column inside each tile
    for row in list(stairs) + [77]:
        q[:, row] = torch.randn(bh, d)  # long rows: little cross-talk
    for row, col in stairs.items():
        n2 = (q[:, row] ** 2).sum(-1, keepdim=True)
        for t in range(4):
            k[:, t * KT + col] = q[:, row] * (6.0 * (t + 1) / scale / n2)
    n2 = (q[:, 77] ** 2).sum(-1, keepdim=True)
    k[:, 3 * KT + 8] = q[:, 77] * (30.0 / scale / n2)
    q, k, v = _round(q), _round(k), _round(v)

    # the inputs do what the docstring says, in every batch-head
    s = torch.bmm(q, k.transpose(1, 2)) * scale
    for bi in range(bh):
        for row in stairs:
            tm = s[bi, row].reshape(4, KT).max(dim=1).values
            steps = tm[1:] - tm[:-1]
            assert (steps > 4).all() and (steps < 8).all(), (row, tm)
            assert _rescale_tiles(s[bi], row) == [0, 2], (bi, row)
        tm = s[bi, 77].reshape(4, KT).max(dim=1).values
        assert tm[3] - tm[:3].max() > 8, tm
        assert 3 in _rescale_tiles(s[bi], 77)

    ref = dispatch.attention(q, k, v, heads=1)
    out = dispatch.attention(_bf16(q).cuda(), _bf16(k).cuda(), _bf16(v).cuda(),
                             heads=1).float().cpu()
    err = (out - ref).abs().max().item()
    rows = list(stairs) + [77]
    err_rows = (out - ref)[:, rows].abs().max().item()
    print(f"staircase: max err {err:.5f}, forced rows {err_rows:.5f}")
    assert err < 0.05, f"defer-max staircase err {err}"
    ref64, bound = kb.attention_ref(q, k, v)
    kb.check(out, ref64, bound, "defer-max staircase")


def test_row_sums_uniform_v(extmod):
    """V of all ones returns the softmax row sum divided by itself: the
    lane-local partial sums must add up to exactly what went into PV."""
    from comfyui_distributed_amd.ops import dispatch

    torch.manual_seed(150)
    bh, nq, nk, d = 2, 100, 150, 40
    q = _bf16(torch.randn(bh, nq, d)).cuda()
    k = _bf16(torch.randn(bh, nk, d)).cuda()
    v = torch.ones(bh, nk, d, dtype=torch.bfloat16).cuda()
    out = dispatch.attention(q, k, v, heads=1).float()
    err = (out - 1.0).abs().max().item()
    print(f"row sums: max |out-1| {err:.5f}")
    assert err < 0.01, err
    ref64, bound = kb.attention_ref(q.float().cpu(), k.float().cpu(),
                                    v.float().cpu())
    kb.check(out, ref64, bound, "row sums, uniform V")
