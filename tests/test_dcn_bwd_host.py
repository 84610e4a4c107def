"""The DCNv2 backward, on the CPU: the gradient oracle is pinned, and the C ABI / Python surface of the new entry is checked
as far as that goes without a GPU.

The oracle of tests/test_gpu_dcn_bwd.py is torch.autograd.grad through tests/dcn_ref.py::dcn_ref with fp64 leaves (`g64`).
dcn_ref is a composition of differentiable torch operations (F.grid_sample, einsum); here its gradients are held to answers that
do not come from grid_sample's own backward:
  * for constant per-tap offsets the operation is linear in x and in the filters, so d/dx, d/dweight, d/dbias must equal autograd
    through the closed form shifted_conv_ref (zero-filled integer shifts and their dyadic combinations) to fp64 round-off;
  * d/doffset and d/dmask must equal central finite differences of dcn_ref itself (step 2^-20 — every perturbed sample point
    is still an exact fp32 number, so dcn_ref's fp32 point formation does not disturb the difference — and all points at least
    1/8 away from integer coordinates, where the bilinear form has a kink); within a cell the sample is linear in h and in w
    separately, so the central difference is the derivative up to round-off.
The deliberately wrong variants dcn_ref can build (align_corners=True, padding_mode='border', gate_min=0) are rejected by
these checks.
"""
import ctypes
import os
import subprocess

import pytest
import torch

from dcn_ref import const_offmask, dcn_ref, fractional_taps, integer_taps, out_hw, shifted_conv_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASKS = (0.25, 1.0, 0.5, 0.0, 1.0, 0.75, 0.5, 1.0, 0.25)
B, C, CO, H, W = 1, 3, 2, 5, 6                    # the tiny case
WRONG = ({'align_corners': True}, {'padding_mode': 'border'}, {'gate_min': 0})


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _err(a, b):
    return (a - b).abs().max().item() / b.abs().max().item()


def _case(stride, taps, seed):
    g = _g(seed)
    Ho, Wo = out_hw(H, W, stride, 1)
    x = torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(CO, C, 3, 3, generator=g, dtype=torch.float64)
    b = torch.randn(CO, generator=g, dtype=torch.float64)
    gy = torch.randn(B, CO, Ho, Wo, generator=g, dtype=torch.float64)
    off, m = const_offmask(B, Ho, Wo, taps, MASKS)
    return x, off.double(), m.double(), w, b, gy


def _g64(x, off, m, w, b, gy, stride, **variant):
    leaves = [t.clone().requires_grad_(True) for t in (x, off, m, w, b)]
    y = dcn_ref(*leaves, stride, 1, **variant)
    return torch.autograd.grad((y * gy).sum(), leaves)


def _closed_form_grads(x, taps, w, b, gy, stride):
    leaves = [t.clone().requires_grad_(True) for t in (x, w, b)]
    y = shifted_conv_ref(leaves[0], taps, leaves[1], leaves[2], stride, 1, MASKS)
    return torch.autograd.grad((y * gy).sum(), leaves)


def _off_center_taps():
    """fractional_taps moved by 1/8: every coordinate an odd multiple of 1/8, never closer than 1/8 to an integer."""
    return [(dh + 0.125, dw + 0.125) for dh, dw in fractional_taps()]


TAPS = {'integer': integer_taps(H, W), 'fractional': fractional_taps(), 'off_center': _off_center_taps()}


@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('kind', sorted(TAPS))
def test_oracle_linear_gradients_equal_closed_form(kind, stride):
    x, off, m, w, b, gy = _case(stride, TAPS[kind], 40 + stride)
    gx, _, _, gw, gb = _g64(x, off, m, w, b, gy, stride)
    cx, cw, cb = _closed_form_grads(x, TAPS[kind], w, b, gy, stride)
    assert _err(gx, cx) < 1e-12 and _err(gw, cw) < 1e-12 and _err(gb, cb) < 1e-12


def _finite_differences(x, off, m, w, b, gy, stride, which):
    """Central differences of sum(dcn_ref * gy) in every element of offset (which = 1) or mask (which = 2), step 2^-20."""
    eps = 2.0 ** -20
    args = [x, off, m, w, b]
    out = torch.zeros_like(args[which])
    flat = out.view(-1)
    for e in range(flat.numel()):
        vals = []
        for sgn in (1.0, -1.0):
            a = list(args)
            a[which] = args[which].clone()
            a[which].view(-1)[e] += sgn * eps
            vals.append((dcn_ref(*a, stride, 1) * gy).sum().item())
        flat[e] = (vals[0] - vals[1]) / (2 * eps)
    return out


_FD = {}


def _fd_case(stride):
    if stride not in _FD:
        case = _case(stride, TAPS['off_center'], 50 + stride)
        _FD[stride] = (case, _finite_differences(*case, stride, 1), _finite_differences(*case, stride, 2))
    return _FD[stride]


@pytest.mark.parametrize('stride', [1, 2])
def test_oracle_offset_and_mask_gradients_equal_finite_differences(stride):
    case, fd_off, fd_mask = _fd_case(stride)
    _, goff, gmask, _, _ = _g64(*case, stride)
    assert fd_off.abs().max().item() > 0.1 and fd_mask.abs().max().item() > 0.1
    # round-off of the difference quotient: ~ 2^-52 * |loss| / 2^-20 ~ 1e-9 relative
    assert _err(goff, fd_off) < 1e-7 and _err(gmask, fd_mask) < 1e-7


@pytest.mark.parametrize('variant', WRONG, ids=lambda v: next(iter(v)))
def test_the_checks_reject_wrong_variants(variant):
    """Each wrong variant of dcn_ref misses the closed form in d/dx AND the finite differences of the correct operation in
    d/doffset by orders of magnitude more than the bars above."""
    for stride in (1, 2):
        x, off, m, w, b, gy = _case(stride, TAPS['off_center'], 40 + stride)
        gx = _g64(x, off, m, w, b, gy, stride, **variant)[0]
        cx = _closed_form_grads(x, TAPS['off_center'], w, b, gy, stride)[0]
        assert _err(gx, cx) > 1e-3, (variant, stride)
        case, fd_off, _ = _fd_case(stride)
        goff = _g64(*case, stride, **variant)[1]
        assert _err(goff, fd_off) > 1e-3, (variant, stride)


# ---- the C ABI and the Python surface, without a GPU -----------------------------------------------------------------------

def test_backward_entry_is_exported_and_bound_at_abi_9():
    from yolact_amd import _lib as L
    lib = L.lib()
    assert lib.ymi_abi_version() == 9 and L.ABI_VERSION == 9
    assert any(name == 'ymi_dcn_v2_backward_f32' for name, _, _ in L.SYMBOLS)
    assert lib.ymi_dcn_v2_backward_f32.argtypes[0] == ctypes.POINTER(L.DcnBwdDesc)


def test_backward_descriptor_matches_c_compiler(tmp_path):
    from yolact_amd import _lib as L
    src = tmp_path / 'sz.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu %%zu %%zu %%zu %%zu\\n",'
                   'sizeof(ymi_dcn_bwd_desc),offsetof(ymi_dcn_bwd_desc,gx),offsetof(ymi_dcn_bwd_desc,B),'
                   'offsetof(ymi_dcn_bwd_desc,kh),offsetof(ymi_dcn_bwd_desc,om_layout));return 0;}'
                   % os.path.join(ROOT, 'include', 'yolact_amd.h'))
    exe = tmp_path / 'sz'
    subprocess.run(['gcc', str(src), '-o', str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    D = L.DcnBwdDesc
    assert got == [ctypes.sizeof(D), D.gx.offset, D.B.offset, D.kh.offset, D.om_layout.offset]
    assert ctypes.sizeof(D) == 9 * 8 + 18 * 4


def _desc(**over):
    from yolact_amd import _lib as L
    d = L.DcnBwdDesc()
    d.B, d.H, d.W, d.Cin, d.ldx, d.Ho, d.Wo, d.Cout = 1, 8, 8, 32, 32, 8, 8, 16
    d.kh, d.kw, d.stride, d.pad, d.dilation, d.deformable_groups = 3, 3, 1, 1, 1, 1
    d.ldo, d.mask_is_prob, d.om_layout = 27, 1, 0
    for k, v in over.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize('over,code', [
    ({'kh': 5, 'kw': 5, 'pad': 2}, -1), ({'pad': 0}, -1), ({'dilation': 2}, -1), ({'deformable_groups': 2}, -1),
    ({'stride': 3}, -1), ({'mask_is_prob': 0}, -1), ({'om_layout': 2}, -1),
    ({'Cin': 24, 'ldx': 24}, -1), ({'Cin': 48, 'ldx': 48}, -2), ({'ldx': 34}, -2), ({'ldo': 26}, -2), ({'Ho': 4}, -2),
    ({'stride': 2}, -2),                                 # Ho / Wo still those of stride 1
    ({'B': 1 << 20, 'H': 64, 'W': 64, 'Ho': 64, 'Wo': 64}, -2),
])
def test_backward_rejects_unsupported_descriptors_without_a_gpu(over, code):
    """Every gradient pointer is set (to an address nothing may touch): a launch would fault, a validation error returns."""
    from yolact_amd import _lib as L
    d = _desc(**over)
    for f in ('x', 'offmask', 'w', 'gy', 'gx', 'g_offset', 'g_mask', 'gw', 'gbias'):
        setattr(d, f, 16)
    assert L.lib().ymi_dcn_v2_backward_f32(ctypes.byref(d), None) == code


def test_backward_null_handling_without_a_gpu():
    from yolact_amd import _lib as L
    lib = L.lib()
    assert lib.ymi_dcn_v2_backward_f32(None, None) == -3
    assert lib.ymi_dcn_v2_backward_f32(ctypes.byref(_desc()), None) == 0       # no gradient wanted: nothing to do, no launch
    d = _desc(gx=16)                                                            # a gradient wanted, inputs missing
    assert lib.ymi_dcn_v2_backward_f32(ctypes.byref(d), None) == -3


def test_dcn_v2_conv_on_cpu_tensors_still_raises():
    from yolact_amd import dcn_v2
    x = torch.randn(1, 4, 5, 5, requires_grad=True)
    off, m = torch.zeros(1, 18, 5, 5, requires_grad=True), torch.full((1, 9, 5, 5), 0.5, requires_grad=True)
    w, b = torch.randn(4, 4, 3, 3, requires_grad=True), torch.zeros(4, requires_grad=True)
    with pytest.raises(RuntimeError):
        dcn_v2.dcn_v2_conv(x, off, m, w, b, 1, 1, 1, 1)
    with pytest.raises(RuntimeError):
        dcn_v2.DCN(4, 4, 3, stride=1, padding=1)(x)
    assert hasattr(dcn_v2, '_DCNv2Function') and issubclass(dcn_v2._DCNv2Function, torch.autograd.Function)
