"""The UNet and VAE modules on the GPU at widths where the HIP routes are
taken, against the written-out fp64 references of module_refs.

Each case builds the seeded module on the CPU, casts it to bf16, moves it to
the device, gives 4-D inputs channels_last (as UNetModel.forward and
VAE.decode do), runs one forward and measures e_rms and e_max against the
reference. The limits are relative to the yardstick (the same reference with
the model's bf16 roundings, computed on the CPU):

    e_rms <= 2 x yardstick        e_max <= 3 x yardstick

The kernels round where the yardstick rounds, or at fewer places; what they
add (fp32 instead of fp64 accumulation, the exp2-domain softmax, the v_rcp
SiLU) is a few fp32 ulps against 2^-9, so a healthy module sits near 1x. The
RMS over >= 10^4 outputs is stable; the maximum is an extreme-value statistic
and gets the wider factor. The smallest seeded wiring defect is 5.1x on e_rms
(test_module_bounds_cpu.py). Measured ratios: profiles/r14_module_bounds.md.

Route assertions: a case that falls back to MIOpen or eager proves nothing,
so each case wraps ``dispatch.ext.get_ext`` in a proxy that counts the
extension functions called (a Python-level call counter) and asserts the
expected multiset, and where the variant matters the launch-free
``conv256_plan`` / ``group_norm_nhwc_plan``.
"""

import copy
import dataclasses
from collections import Counter

import pytest
import torch

import module_refs as mr
from comfyui_distributed_amd.ops import dispatch

pytestmark = pytest.mark.gpu

RMS_LIMIT, MAX_LIMIT = 2.0, 3.0

PARAMS = [(c.name, f) for c in mr.CASES
          for f in ((False, True) if c.fuse_res else (None,))]


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


@pytest.fixture()
def calls(monkeypatch):
    """Counter of the extension functions called through dispatch."""
    counter = Counter()
    real = dispatch.ext.get_ext

    def get_ext(required=None):
        mod = real(required)
        return None if mod is None else _Proxy(mod, counter)

    monkeypatch.setattr(dispatch.ext, "get_ext", get_ext)
    return counter


def _to_device(module, inputs):
    m = copy.deepcopy(module).to(mr.BF).cuda()
    dev = []
    for t in inputs:
        t = t.to(mr.BF).cuda() if t.is_floating_point() else t.cuda()
        if t.dim() == 4:
            t = t.contiguous(memory_format=torch.channels_last)
        dev.append(t)
    return m, tuple(dev)


def _check(cd, module, inputs, y, label):
    got, yard = cd.metrics(y), cd.yard_metrics()
    bad = []
    for key, (e_rms, e_max) in got.items():
        r_rms, r_max = e_rms / yard[key][0], e_max / yard[key][1]
        print(f"MODULE_BOUNDS {label} {key} e_rms_ratio {r_rms:.3f} "
              f"e_max_ratio {r_max:.3f} (yardstick e_rms {yard[key][0]:.3e} "
              f"e_max {yard[key][1]:.3e})")
        if not (r_rms <= RMS_LIMIT and r_max <= MAX_LIMIT):
            bad.append((key, r_rms, r_max))
    if bad:
        with torch.no_grad():
            stages = mr.stage_errors(module, lambda: cd.forward(module, inputs),
                                     cd.inter_ref, cd.inter_yard)
        table = "\n".join(f"  {n}: e_rms {a:.2f}x e_max {b:.2f}x"
                          for n, a, b in stages)
        pytest.fail(f"{label}: (metric, e_rms ratio, e_max ratio) {bad} over "
                    f"the limits {RMS_LIMIT} / {MAX_LIMIT}; stages against "
                    f"their own yardstick:\n{table}")


@pytest.mark.parametrize("name,fuse", PARAMS)
def test_module_against_reference(name, fuse, calls, monkeypatch):
    cd = mr.case_data(name)
    case = cd.case
    if fuse is not None:
        monkeypatch.setattr(dispatch, "_FUSE_RES", fuse)
    module, inputs = _to_device(cd.module, cd.inputs)
    if name == "res_cat320_128":
        cat = torch.cat([inputs[0], inputs[1]], dim=1)
        assert cat.is_contiguous(memory_format=torch.channels_last)
        assert not cat.is_contiguous()
    calls.clear()
    with torch.no_grad():
        y = cd.forward(module, inputs)
    torch.cuda.synchronize()
    routes = dict(calls)
    assert y.dtype == mr.BF and y.shape == cd.ref.shape
    assert routes == case.routes, (name, routes, case.routes)
    ext = dispatch.ext.get_ext(True)
    for plan in case.plans:
        if plan[0] == "conv":
            assert tuple(ext.conv256_plan(*plan[1:4])) == plan[4], plan
        else:
            b, hw, c = plan[1:]
            threads, p, ns, bpi, ppb = ext.group_norm_nhwc_plan(b, hw, c)
            assert ns == 1 and ppb % p == 0 and bpi * ppb >= hw, plan
    label = name if fuse is None else f"{name}[fuse_res={fuse}]"
    _check(cd, module, inputs, y, label)


def _scaled_twin(cd, names):
    """CaseData of cd's module with the named parameters doubled (exact in
    bf16): reference and yardstick recomputed from the scaled values."""
    P = dict(cd.P)
    for n in names:
        P[n] = P[n] * 2
    with torch.no_grad():
        ref, inter_ref = cd.case.ref(P, *mr.to64(cd.inputs), rnd=mr.ident)
        yard, inter_yard = cd.case.ref(P, *mr.to64(cd.inputs), rnd=mr.bf16)
    return dataclasses.replace(cd, ref=ref, yard=yard, inter_ref=inter_ref,
                               inter_yard=inter_yard, P=P)


MUL_NAMES = {
    "res128": ("norm1.weight", "norm2.bias", "conv1.bias"),
    "st128": ("norm.weight", "blocks.0.norm1.weight", "blocks.0.norm2.bias"),
}


@pytest.mark.parametrize("how", ["load_state_dict", "copy_", "mul_"])
@pytest.mark.parametrize("name", ["res128", "st128"])
def test_module_follows_parameter_update(name, how, calls):
    """Stale caches on the device: a forward fills the fp32 parameter copies,
    the repacked conv weights and the fused QKV / KV weights; then the
    parameters are updated in place (load_state_dict of a differently seeded
    twin, copy_ from it parameter by parameter, or mul_(2) of norm and bias
    parameters) and the next forward is inside the limits of the reference of
    the new values."""
    first = mr.case_data(name)
    module, inputs = _to_device(first.module, first.inputs)
    with torch.no_grad():
        y0 = first.forward(module, inputs)
        if how == "mul_":
            twin = _scaled_twin(first, MUL_NAMES[name])
            params = dict(module.named_parameters())
            for n in MUL_NAMES[name]:
                params[n].mul_(2)
        else:
            twin = mr.case_data(name, seed=1)
            other, _ = _to_device(twin.module, ())
            if how == "load_state_dict":
                module.load_state_dict(other.state_dict())
            else:
                for p, q in zip(module.parameters(), other.parameters()):
                    p.copy_(q)
        calls.clear()
        y1 = first.forward(module, inputs)
    torch.cuda.synchronize()
    assert dict(calls) == first.case.routes
    assert not torch.equal(y0, y1)
    _check(twin, module, inputs, y1, f"{name}[after {how}]")
