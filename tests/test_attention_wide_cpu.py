"""Wide-head attention, the parts that need no GPU: the pad classes of
dispatch and the single-head (autoencoder-KL) VAE configuration."""

import pytest
import torch

import module_refs as mr
from comfyui_distributed_amd.models import create_diffusion_stack
from comfyui_distributed_amd.models import vae as V
from comfyui_distributed_amd.ops import dispatch
from test_vae_single_head_gpu import attention_block_ref


def test_dpad_classes():
    assert [dispatch._dpad_for(d) for d in (160, 168, 256, 264, 512)] == \
        [160, 256, 256, 512, 512]
    with pytest.raises(ValueError):
        dispatch._dpad_for(520)


def test_single_head_config():
    kl = V.VAE(V.VAEConfig(attn_head_dim=None))
    assert kl.encoder.mid[1].heads == kl.decoder.mid[1].heads == 1
    assert kl.decoder.mid[1].head_dim == 512
    sd = V.VAE(V.SD_VAE)
    assert sd.encoder.mid[1].heads == sd.decoder.mid[1].heads == 8
    assert V.SD_VAE_KL.attn_head_dim is None is V.SDXL_VAE_KL.attn_head_dim
    assert V.SDXL_VAE_KL.scale_factor == V.SDXL_VAE.scale_factor


def test_variant_selection():
    assert V.resolve_vae_variant("sdxl_kl", V.SD_VAE) is V.SDXL_VAE_KL
    assert create_diffusion_stack("tiny").vae.cfg.attn_head_dim == 64
    for name in ("tiny", "wan_tiny", "flux_tiny"):
        vae = create_diffusion_stack(name, vae_variant="kl").vae
        cfg = getattr(vae, "spatial", vae).cfg
        assert cfg.attn_head_dim is None and cfg.base_channels == 8
    with pytest.raises(ValueError):
        create_diffusion_stack("tiny", vae_variant="nope")


def test_single_head_forward_matches_reference():
    """128 mid channels: one head with attn_head_dim=None, two by default.
    fp32 forward against the written-out fp64 reference of each."""
    cfg = V.VAEConfig(base_channels=32, channel_mult=(1, 2, 4),
                      num_res_blocks=1, attn_head_dim=None)
    block = mr.seeded(lambda: V.VAE(cfg), 3).decoder.mid[1]
    assert block.heads == 1
    x = mr.randn_bf16(4, 2, 128, 5, 5)
    P = mr.params_of(block)
    with torch.no_grad():
        y = block(x).double()
        one, two = (attention_block_ref(P, x.double(), h, mr.ident)
                    for h in (1, 2))
    assert mr.errors(y - x, one - x)[1] < 1e-4
    assert mr.errors(y - x, two - x)[0] > 0.1
