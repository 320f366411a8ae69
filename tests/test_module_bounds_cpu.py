"""The module-level method of module_refs, shown on the CPU for every case of
its table:

(a) the module's own fp32 forward is within 1/50 of the yardstick's error of
    the written-out fp64 reference (fp32 has a 2^16 smaller unit roundoff than
    bf16, so a correct module passes by orders of magnitude and a wiring
    mistake on the CPU path does not);
(b) the module's own bf16 forward has an e_rms within [0.5, 1.5] x the
    yardstick's: the yardstick measures what a healthy bf16 chain does;
(c) every seeded defect, injected into the reference (never into the module),
    puts the bf16 forward at >= 4x the yardstick's e_rms, twice the limit the
    GPU tests assert. On the branch metric where the case has one.

The factors are fixed. Every defect clears 4x at the shapes of the table with
plain randn inputs (the smallest, SiLU for GELU in SpatialTransformer(128, 96,
2, 64), is 5.1x), so no input was changed to meet (c).
"""

import copy
import functools

import pytest
import torch

import module_refs as mr

NAMES = [c.name for c in mr.CASES]
PAIRS = [(c.name, d) for c in mr.CASES for d in c.defects]


@functools.lru_cache(maxsize=None)
def _forward(name, dtype):
    """The module's own CPU forward in ``dtype``, once per case."""
    cd = mr.case_data(name)
    module = copy.deepcopy(cd.module).to(dtype)
    inputs = tuple(t.to(dtype) if t.is_floating_point() else t
                   for t in cd.inputs)
    with torch.no_grad():
        return cd.forward(module, inputs)


@pytest.mark.parametrize("name", NAMES)
def test_fp32_forward_matches_reference(name):
    cd = mr.case_data(name)
    got = cd.metrics(_forward(name, torch.float32))
    yard = cd.yard_metrics()
    for key, (e_rms, e_max) in got.items():
        print(f"{name} {key}: fp32 e_rms {e_rms:.3e} e_max {e_max:.3e}; "
              f"yardstick {yard[key][0]:.3e} {yard[key][1]:.3e}")
        assert e_rms <= yard[key][0] / 50, (name, key, e_rms, yard[key])
        assert e_max <= yard[key][1] / 50, (name, key, e_max, yard[key])


@pytest.mark.parametrize("name", NAMES)
def test_bf16_forward_tracks_yardstick(name):
    cd = mr.case_data(name)
    got = cd.metrics(_forward(name, torch.bfloat16))
    yard = cd.yard_metrics()
    for key, (e_rms, e_max) in got.items():
        ratio = e_rms / yard[key][0]
        print(f"{name} {key}: bf16 e_rms {e_rms:.3e} = {ratio:.2f} x "
              f"yardstick; e_max {e_max / yard[key][1]:.2f} x")
        assert 0.5 <= ratio <= 1.5, (name, key, e_rms, yard[key])


@pytest.mark.parametrize("name,defect", PAIRS)
def test_seeded_defect_is_visible(name, defect):
    assert defect in mr.DEFECTS
    cd = mr.case_data(name)
    with torch.no_grad():
        bad, _ = cd.case.ref(cd.P, *mr.to64(cd.inputs), rnd=mr.ident,
                             defect=defect)
    assert bad.shape == cd.ref.shape
    y = _forward(name, torch.bfloat16).to(mr.F64)
    key = "branch" if cd.case.branch else "out"
    if cd.case.branch:
        x = cd.x64()
        e_rms, _ = mr.errors(y - x, bad - x)
    else:
        e_rms, _ = mr.errors(y, bad)
    yard = cd.yard_metrics()[key][0]
    print(f"{name} {defect} ({mr.DEFECTS[defect]}): {key} e_rms {e_rms:.4f} "
          f"= {e_rms / yard:.1f} x yardstick")
    assert e_rms >= 4 * yard, (name, defect, e_rms, yard)


def test_every_defect_is_seeded_somewhere():
    assert {d for _, d in PAIRS} == set(mr.DEFECTS)


def test_route_tables_of_the_compositions():
    """The extension-call counts the GPU tests expect of the two compositions
    are derived from the layout; spot values worked out by hand."""
    r = mr.CASE["unet"].routes
    # 1 stem; 8 ResBlocks (2 in, 2 mid, 4 out), 7 SpatialTransformers (2 in,
    # 1 mid, 4 out) and out_norm
    assert r["conv_smallc"] == 1 and r[mr.GN] == 2 * 8 + 7 + 1
    assert r["attn_fwd_qkv"] == r["attn_fwd_q_kv"] == r["act_mul"] == 7
    assert r["layer_norm"] == 21
    # level 1 runs at 9x10, M = 180: every conv there is the direct kernel
    # (input ResBlock 3 with its skip, two mid ResBlocks 2+2, two output
    # ResBlocks 3+3). The 256-tile kernel: level-0 input ResBlock 2,
    # Downsample 1, Upsample to (17, 19) 1, output ResBlocks 3+3, out_conv 1
    assert r[mr.CDIR] == 3 + 4 + 6
    assert r[mr.C256] == 2 + 1 + 1 + 3 + 3 + 1
    v = mr.CASE["vae_decoder"].routes
    assert v == {"conv_smallc": 1, mr.GN: 2 * 6 + 1 + 1, "attn_fwd_packed": 1,
                 mr.CDIR: 2 * 4, mr.C256: 1 + 3 + 2 + 1}
