"""VAEAttention as the autoencoder-KL block (one head over 512 channels, the
wide-head attention kernel) against a written-out fp64 reference:
module_refs.vae_attention_ref takes its head count from the channel count,
not from the module, so it is written out here from the same pieces. Metric
and limits of test_module_bounds_gpu.py on the branch y - x: e_rms <= 2 x,
e_max <= 3 x the bf16 yardstick.

head_dim = 64 runs the same weights and input as 8 heads: each module is
inside the limits of its own reference and outside them against the other's.
(fp64 reference against fp64 reference on the CPU: 8 heads sit at e_rms 11.8 x
and e_max 6.5 x the single-head yardstick.) Measured ratios:
profiles/r19_attention_wide.md.
"""

import copy

import pytest
import torch

import module_refs as mr
from comfyui_distributed_amd.models import vae as V

pytestmark = pytest.mark.gpu

RMS_LIMIT, MAX_LIMIT = 2.0, 3.0
C = 512


def attention_block_ref(P, x, heads, rnd):
    b, c, h, w = x.shape
    t = mr._gn(P, "norm", x, False, rnd).permute(0, 2, 3, 1).reshape(b, h * w, c)
    q, k, v = mr._linear(P, "qkv", t, rnd).chunk(3, dim=-1)
    o = mr._linear(P, "proj", mr._attention(q, k, v, heads, rnd), rnd)
    return rnd(x + o.reshape(b, h, w, c).permute(0, 3, 1, 2))


@pytest.fixture(scope="module")
def data():
    """Same seed, so both modules hold the same weights; references and
    yardsticks of both head counts, computed once."""
    x = mr.randn_bf16(5, 2, C, 9, 9)
    mods = {hd: mr.seeded(lambda: V.VAEAttention(C, head_dim=hd), 77)
            for hd in (512, 64)}
    P = mr.params_of(mods[512])
    with torch.no_grad():
        refs = {hd: (attention_block_ref(P, x.double(), C // hd, mr.ident),
                     attention_block_ref(P, x.double(), C // hd, mr.bf16))
                for hd in (512, 64)}
    return x, mods, refs


def ratios(y, x, ref, yard):
    x = x.double()
    e, ye = mr.errors(y.double().cpu() - x, ref - x), mr.errors(yard - x, ref - x)
    return e[0] / ye[0], e[1] / ye[1]


@pytest.mark.parametrize("head_dim", [512, 64])
def test_vae_attention_block(data, head_dim):
    x, mods, refs = data
    assert mods[head_dim].heads == C // head_dim
    m = copy.deepcopy(mods[head_dim]).to(mr.BF).cuda()
    xd = x.to(mr.BF).cuda().contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        y = m(xd)
    own = ratios(y, x, *refs[head_dim])
    other = ratios(y, x, *refs[576 - head_dim])
    print(f"VAE_ATTN head_dim {head_dim}: own e_rms {own[0]:.3f}x e_max "
          f"{own[1]:.3f}x; against the other architecture e_rms "
          f"{other[0]:.1f}x e_max {other[1]:.1f}x")
    assert own[0] <= RMS_LIMIT and own[1] <= MAX_LIMIT, own
    assert other[0] > RMS_LIMIT and other[1] > MAX_LIMIT, other
