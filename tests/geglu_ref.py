"""fp64 reference and bound of the GEGLU-fused Linear: a = x Wa^T + ba,
g = x Wg^T + bg, ref = a * gelu_tanh(g), |err| <= act(a, g) + (K + 1) * 2^-23 *
(A * |gelu(g)| + 1.13 * |a| * G) with A, G the sums of absolute terms of a, g:
kernel_bounds.act_mul_ref's bound plus the dot-product bound n * 2^-23 * mag
through the product rule (1.13 >= |gelu_tanh'|)."""

import torch.nn.functional as F

import kernel_bounds as kb


def geglu_ref(x, weight, bias=None):
    """x [M, K], weight [2*inner, K] (value, then gate rows) -> fp64."""
    inner, k = weight.shape[0] // 2, x.shape[1]
    xd, wd = x.double(), weight.double()
    pre, mag = xd @ wd.t(), xd.abs() @ wd.abs().t()
    if bias is not None:
        pre, mag = pre + bias.double(), mag + bias.double().abs()
    a, g = pre[:, :inner], pre[:, inner:]
    ref, act = kb.act_mul_ref(a, g, True)
    gelu = F.gelu(g, approximate="tanh").abs()
    return ref, act + (k + 1) * 2.0 ** -23 * (
        mag[:, :inner] * gelu + 1.13 * a.abs() * mag[:, inner:])
