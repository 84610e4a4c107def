"""The DCNv2 backward (csrc/dcn_bwd.hip, ymi_dcn_v2_backward_f32, yolact_amd/dcn_v2.py) against the fp64 gradient oracle.

Oracle: torch.autograd.grad through tests/dcn_ref.py::dcn_ref with fp64 leaves (`g64`; pinned by tests/test_dcn_bwd_host.py).
Bar: per case and per gradient tensor, max(4 * rel_err(g32, g64), EXACT_BAR) where g32 is the same grid_sample formulation with
fp32 leaves and fp32 arithmetic on the CPU and EXACT_BAR = 8e-6 is what tests/test_gpu_dcn_kat.py holds the exact-fp32 forward
tiles to.  The factor 4 covers what legitimately differs from a CPU fp32 run: atomics and MFMA accumulate in another order
(both errors grow like eps * sqrt(terms)).

Offsets are N(0, 2^2) (external/DCNv2/test.py:74) and then CONSTRUCTED off the bilinear kinks: any sample coordinate whose
fractional part is within 1/16 of an integer is moved to the nearest of {1/16, 15/16} of its cell, so the derivative is defined
everywhere and no element is excluded from any comparison.

The largest rel_err per case and gradient is printed at the end of the module (the table of DESIGN.md 5.1).
"""
import ctypes as C
import itertools
import math
import os
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dcn_ref import dcn_ref, out_hw, sample_points  # noqa: E402
from gpu_utils import rel_err  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EXACT_BAR = 8e-6
NAMES = ('input', 'offset', 'mask', 'weight', 'bias')
_MAX = {}


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    print('\nDCNv2 backward: rel_err against g64 (bar)')
    for case in sorted(_MAX):
        print('  %-28s ' % case + '  '.join('%s %.2e (%.1e)' % (n, e, b) for n, (e, b) in _MAX[case].items()))


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _base(H, W, stride):
    Ho, Wo = out_hw(H, W, stride, 1)
    ki = torch.arange(9)
    bh = (torch.arange(Ho) * stride - 1).view(1, 1, Ho, 1) + (ki // 3).view(1, 9, 1, 1)
    bw = (torch.arange(Wo) * stride - 1).view(1, 1, 1, Wo) + (ki % 3).view(1, 9, 1, 1)
    return bh.expand(1, 9, Ho, Wo).float(), bw.expand(1, 9, Ho, Wo).float()


def off_kink_offsets(off, H, W, stride):
    """Move every sample coordinate whose fraction is within 1/16 of an integer to 1/16 or 15/16 of its cell."""
    Bn, _, Ho, Wo = off.shape
    h, w = sample_points(H, W, off, stride, 1)
    bh, bw = _base(H, W, stride)
    out = []
    for c, base, old in ((h, bh, off[:, 0::2]), (w, bw, off[:, 1::2])):
        cell = torch.floor(c)
        fr = c - cell
        tgt = torch.where(fr < 1 / 16, cell + 1 / 16, torch.where(fr > 15 / 16, cell + 15 / 16, c))
        out.append(torch.where(tgt == c, old, tgt - base))      # untouched: as drawn; moved: cell + k/16 - integer, exact in fp32
    new = torch.stack(out, 2).reshape(Bn, 18, Ho, Wo).float()
    h2, w2 = sample_points(H, W, new, stride, 1)
    for c2 in (h2, w2):
        fr = c2 - torch.floor(c2)
        assert fr.min().item() >= 1 / 16 - 1e-6 and fr.max().item() <= 15 / 16 + 1e-6
    # fp32 and fp64 sample points fall in the same cell, for every element
    h64, w64 = bh.double() + new[:, 0::2].double(), bw.double() + new[:, 1::2].double()
    assert torch.equal(torch.floor(h2).double(), torch.floor(h64)) and torch.equal(torch.floor(w2).double(), torch.floor(w64))
    return new


def make_case(B, Cin, Cout, H, W, stride, bias, seed, spread=2.0):
    g = _g(seed)
    Ho, Wo = out_hw(H, W, stride, 1)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * math.sqrt(2.0 / (9 * Cin))
    b = torch.randn(Cout, generator=g) if bias else None
    mask = torch.sigmoid(torch.randn(B, 9, Ho, Wo, generator=g))
    off = off_kink_offsets(torch.randn(B, 18, Ho, Wo, generator=g) * spread, H, W, stride)
    gy = torch.randn(B, Cout, Ho, Wo, generator=g)
    return x, off, mask, w, b, gy, stride


def dcn_f32(x, offset, mask, weight, bias, stride):
    """dcn_ref's formulation with fp32 arithmetic throughout (the yardstick of the bar, not an oracle)."""
    Bn, Cc, H, W = x.shape
    h, w = sample_points(H, W, offset, stride, 1)
    out = 0
    for k in range(9):
        i, j = divmod(k, 3)
        grid = torch.stack([(2 * w[:, k] + 1) / W - 1, (2 * h[:, k] + 1) / H - 1], -1)
        s = F.grid_sample(x, grid, mode='bilinear', padding_mode='zeros', align_corners=False) * mask[:, k].unsqueeze(1)
        out = out + torch.einsum('oc,bchw->bohw', weight[:, :, i, j], s)
    return out if bias is None else out + bias.view(1, -1, 1, 1)


def cpu_grads(case, dtype):
    x, off, mask, w, b, gy, stride = case
    leaves = [t.detach().to(dtype).requires_grad_(True) for t in (x, off, mask, w) + ((b,) if b is not None else ())]
    bb = leaves[4] if b is not None else None
    y = dcn_ref(leaves[0], leaves[1], leaves[2], leaves[3], bb, stride, 1) if dtype == torch.float64 else \
        dcn_f32(leaves[0], leaves[1], leaves[2], leaves[3], bb, stride)
    g = list(torch.autograd.grad((y * gy.to(dtype)).sum(), leaves))
    return g + [None] * (5 - len(g))


def gpu_grads(case, needs=(True,) * 5):
    from yolact_amd import dcn_v2
    x, off, mask, w, b, gy, stride = case
    ts = [None if t is None else t.to(DEV).requires_grad_(n) for t, n in zip((x, off, mask, w, b), needs)]
    y = dcn_v2.dcn_v2_conv(ts[0], ts[1], ts[2], ts[3], ts[4], stride, 1, 1, 1)
    y.backward(gy.to(DEV))
    torch.cuda.synchronize()
    return y.detach().cpu(), [None if t is None or t.grad is None else t.grad.cpu() for t in ts]


def check_against_oracle(name, case, got, skip=()):
    g64, g32 = cpu_grads(case, torch.float64), cpu_grads(case, torch.float32)
    row = _MAX.setdefault(name, {})
    bad = []
    for n, a, r64, r32 in zip(NAMES, got, g64, g32):
        if r64 is None or n in skip:
            continue
        assert a is not None and a.shape == r64.shape and a.dtype == torch.float32, n
        bar = max(4 * rel_err(r32.double(), r64), EXACT_BAR)
        e = rel_err(a.double(), r64)
        row[n] = (e, bar)
        print('%s %s: rel_err %.3e bar %.3e' % (name, n, e, bar))
        if not e <= bar:
            bad.append((n, e, bar))
    assert not bad, (name, bad)
    return g64


# every distinct YOLACT++ DCN shape (data/config.py:250-266 at 550 x 550): (Cin = Cout, input size, stride), batch 2
YOLACT = [(128, 138, 2), (128, 69, 1), (256, 69, 2), (256, 35, 1), (512, 35, 2), (512, 18, 1)]
#         B, Cin, Cout, H, W, stride, bias
AWKWARD = {'cin24': (2, 24, 32, 9, 11, 1, True), 'cout20': (2, 32, 20, 9, 11, 1, True), 'h13w17': (2, 32, 32, 13, 17, 1, True),
           's2_even': (2, 32, 36, 12, 10, 2, True), 's2_odd': (2, 64, 32, 13, 17, 2, True), 'nobias': (2, 32, 32, 9, 11, 1, False),
           'batch1': (1, 64, 40, 11, 9, 1, True), 'cin24_cout20_s2': (1, 24, 20, 13, 17, 2, False)}


@pytest.mark.parametrize('shape', YOLACT, ids=lambda s: 'c%d_%d_s%d' % s)
def test_gradients_yolact_shapes(shape):
    Cc, size, stride = shape
    case = make_case(2, Cc, Cc, size, size, stride, True, 1000 + Cc + size)
    _, got = gpu_grads(case)
    check_against_oracle('yolact c%d %d^2 s%d' % shape, case, got)


@pytest.mark.parametrize('name', sorted(AWKWARD))
def test_gradients_awkward_shapes(name):
    Bn, Cin, Cout, H, W, stride, bias = AWKWARD[name]
    case = make_case(Bn, Cin, Cout, H, W, stride, bias, 2000 + sum(map(ord, name)))
    _, got = gpu_grads(case)
    assert (got[4] is None) == (not bias)
    check_against_oracle(name, case, got)


@pytest.mark.parametrize('stride', [1, 2])
def test_exact_zeros_outside_the_image(stride):
    """Taps 0 / 4 / 7 of EVERY pixel sit at h = -1, h = H and h = H + 2.5 (wholly outside: their d/ddh, d/ddw, d/dmu are exactly
    0.0); tap 2 sits at h = -0.5 (half outside: a non-zero, correct gradient).  gx and the other taps against g64 as usual."""
    Bn, Cin, Cout, H, W = 2, 64, 32, 11, 14
    x, off, mask, w, b, gy, _ = make_case(Bn, Cin, Cout, H, W, stride, True, 3000 + stride, spread=1.0)
    bh, bw = _base(H, W, stride)
    for k, hval in ((0, -1.0), (4, float(H)), (7, H + 2.5), (2, -0.5)):
        off[:, 2 * k] = hval - bh[:, k]
    off[:, 2 * 2 + 1] = (W // 2 + 0.3125) - bw[:, 2]            # tap 2: w well inside, off the kinks
    case = (x, off, mask, w, b, gy, stride)
    _, got = gpu_grads(case)
    goff, gmask = got[1], got[2]
    for k in (0, 4, 7):
        assert torch.equal(goff[:, 2 * k], torch.zeros_like(goff[:, 2 * k])), k
        assert torch.equal(goff[:, 2 * k + 1], torch.zeros_like(goff[:, 2 * k + 1])), k
        assert torch.equal(gmask[:, k], torch.zeros_like(gmask[:, k])), k
    # h = -1 exactly is a kink of the bilinear form (one-sided derivative; the operation's gate makes it 0): the oracle is
    # compared on the other taps for offset / mask, and on everything for input / weight / bias
    g64 = check_against_oracle('zeros s%d' % stride, case, got, skip=('offset', 'mask'))
    keep = [k for k in range(9) if k not in (0, 4, 7)]
    ko = [c for k in keep for c in (2 * k, 2 * k + 1)]
    g32 = cpu_grads(case, torch.float32)
    for n, a, r64, r32, idx in (('offset', goff, g64[1], g32[1], ko), ('mask', gmask, g64[2], g32[2], keep)):
        bar = max(4 * rel_err(r32[:, idx].double(), r64[:, idx]), EXACT_BAR)
        e = rel_err(a[:, idx].double(), r64[:, idx])
        _MAX['zeros s%d' % stride][n] = (e, bar)
        assert e <= bar, (n, e, bar)
    assert goff[:, 4].abs().max().item() > 1e-3                                            # tap 2's d/ddh is alive
    assert rel_err(goff[:, 4].double(), g64[1][:, 4]) <= max(4 * rel_err(g32[1][:, 4].double(), g64[1][:, 4]), EXACT_BAR)


SMALL = (2, 32, 36, 9, 11, 1, True)


def test_forward_value_does_not_depend_on_grad_mode():
    from yolact_amd import dcn_v2
    x, off, mask, w, b, gy, stride = make_case(*SMALL, 4000)
    ts = [t.to(DEV) for t in (x, off, mask, w, b)]
    with torch.no_grad():
        y0 = dcn_v2.dcn_v2_conv(*ts, stride, 1, 1, 1)
    y1 = dcn_v2.dcn_v2_conv(*[t.clone().requires_grad_(True) for t in ts], stride, 1, 1, 1)
    assert y1.requires_grad and y1.grad_fn is not None and not y0.requires_grad and torch.equal(y0, y1.detach())
    y2 = dcn_v2.dcn_v2_conv(*ts, stride, 1, 1, 1)            # grad mode on, nothing requires grad: today's path
    assert not y2.requires_grad and torch.equal(y0, y2)
    m = dcn_v2.DCNv2(32, 36, 3, stride=1, padding=1).to(DEV)
    with torch.no_grad():
        z0 = m(ts[0], ts[1], ts[2])
    z1 = m(ts[0], ts[1], ts[2])
    assert z1.requires_grad and torch.equal(z0, z1.detach())
    d = dcn_v2.DCN(32, 36, 3, stride=2, padding=1).to(DEV)
    with torch.no_grad():
        d.conv_offset_mask.weight.copy_(torch.randn(27, 32, 3, 3, generator=_g(1)) * 0.05)
        d.conv_offset_mask.bias.copy_(torch.randn(27, generator=_g(2)) * 0.5)
        u0 = d(ts[0])
    u1 = d(ts[0])
    assert u1.requires_grad and torch.equal(u0, u1.detach())


def _close(a, b, tol=2e-5):
    return rel_err(a.double(), b.double()) <= tol


def test_every_requires_grad_subset():
    """The gradients a subset returns equal those of the full call (to the order of the atomics); the rest are None."""
    case = make_case(*SMALL, 4100)
    _, full = gpu_grads(case)
    for needs in itertools.product((False, True), repeat=5):
        if not any(needs):
            continue
        _, got = gpu_grads(case, needs)
        for n, want, g, f in zip(NAMES, needs, got, full):
            assert (g is not None) == want, (needs, n)
            if want:
                assert _close(g, f), (needs, n, rel_err(g, f))


def _abi_call(case, om_layout=0, want=(True,) * 5):
    """ymi_dcn_v2_backward_f32 directly: NHWC tensors, the descriptor's null pointers for what is not wanted."""
    from yolact_amd import _lib as L
    x, off, mask, w, b, gy, stride = case
    Bn, Cin, H, W = x.shape
    Cout = w.shape[0]
    Ho, Wo = out_hw(H, W, stride, 1)
    assert Cin % 32 == 0
    om = torch.cat([off, mask], 1)
    if om_layout:
        om = torch.stack([off[:, 0::2], off[:, 1::2], mask], 2).reshape(Bn, 27, Ho, Wo)      # [dh_k, dw_k, mask_k] per tap
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(DEV)
    xd, omd, wd, gyd = nhwc(x), nhwc(om), nhwc(w), nhwc(gy)
    shapes = ((Bn, H, W, Cin), (Bn, Ho, Wo, 18), (Bn, Ho, Wo, 9), (Cout, 3, 3, Cin), (Cout,))
    outs = [torch.full(s, float('nan'), device=DEV) if n else None for s, n in zip(shapes, want)]
    d = L.DcnBwdDesc()
    d.x, d.offmask, d.w, d.gy = xd.data_ptr(), omd.data_ptr(), wd.data_ptr(), gyd.data_ptr()
    for f, t in zip(('gx', 'g_offset', 'g_mask', 'gw', 'gbias'), outs):
        setattr(d, f, None if t is None else t.data_ptr())
    d.B, d.H, d.W, d.Cin, d.ldx, d.Ho, d.Wo, d.Cout = Bn, H, W, Cin, Cin, Ho, Wo, Cout
    d.kh, d.kw, d.stride, d.pad, d.dilation, d.deformable_groups = 3, 3, stride, 1, 1, 1
    d.ldo, d.mask_is_prob, d.om_layout = 27, 1, om_layout
    L.check(L.lib().ymi_dcn_v2_backward_f32(C.byref(d), L.stream_ptr()), 'ymi_dcn_v2_backward_f32')
    torch.cuda.synchronize()
    nchw = lambda t: t.permute(0, 3, 1, 2).contiguous().cpu()
    return [None if t is None else (t.cpu() if t.dim() == 1 else nchw(t)) for t in outs]


def test_c_abi_null_pointers_and_layouts():
    case = make_case(*SMALL, 4200)
    _, full = gpu_grads(case)
    a0 = _abi_call(case, 0)
    a1 = _abi_call(case, 1)
    for n, p, q, f in zip(NAMES, a0, a1, full):
        assert not torch.isnan(p).any() and _close(p, f) and _close(q, p), n
    for want in ((True, False, False, False, False), (False, True, False, False, False), (False, False, True, False, False),
                 (False, False, False, True, False), (False, False, False, False, True), (False, True, True, False, True)):
        got = _abi_call(case, 0, want)
        for n, wnt, g, f in zip(NAMES, want, got, a0):
            if wnt:
                assert not torch.isnan(g).any() and _close(g, f), (want, n)


def test_dcn_module_backward_fills_every_grad():
    """DCN: one loss.backward() fills weight / bias / conv_offset_mask.weight / .bias / input gradients; against the same module
    restated on the CPU in fp64 (nn.Conv2d + dcn_ref), bar rule as above with the fp32 CPU restatement."""
    from yolact_amd import dcn_v2
    Cin, Cout, stride = 32, 36, 1
    g = _g(4300)
    d = dcn_v2.DCN(Cin, Cout, 3, stride=stride, padding=1).to(DEV)
    with torch.no_grad():
        d.conv_offset_mask.weight.copy_(torch.randn(27, Cin, 3, 3, generator=g) * 0.05)
        d.conv_offset_mask.bias.copy_(torch.randn(27, generator=g) * 0.5)
        d.bias.copy_(torch.randn(Cout, generator=g) * 0.1)
    x = torch.randn(2, Cin, 10, 9, generator=g)
    gy = torch.randn(2, Cout, 10, 9, generator=g)
    xg = x.to(DEV).requires_grad_(True)
    d(xg).backward(gy.to(DEV))
    params = (d.weight, d.bias, d.conv_offset_mask.weight, d.conv_offset_mask.bias)
    got = [xg.grad.cpu()] + [p.grad.cpu() for p in params]

    def restated(dtype):
        conv = nn.Conv2d(Cin, 27, 3, stride=stride, padding=1).to(dtype)
        with torch.no_grad():
            conv.weight.copy_(d.conv_offset_mask.weight.detach().cpu()); conv.bias.copy_(d.conv_offset_mask.bias.detach().cpu())
        xl = x.to(dtype).requires_grad_(True)
        wl, bl = d.weight.detach().cpu().to(dtype).requires_grad_(True), d.bias.detach().cpu().to(dtype).requires_grad_(True)
        out = conv(xl)
        o1, o2, m = torch.chunk(out, 3, dim=1)
        off, m = torch.cat((o1, o2), 1), torch.sigmoid(m)
        if dtype == torch.float64:
            y = dcn_ref(xl, off, m, wl, bl, stride, 1)
        else:
            y = dcn_f32(xl, off, m, wl, bl, stride)
        return torch.autograd.grad((y * gy.to(dtype)).sum(), [xl, wl, bl, conv.weight, conv.bias])

    g64, g32 = restated(torch.float64), restated(torch.float32)
    row = _MAX.setdefault('DCN module', {})
    for n, a, r64, r32 in zip(('input', 'weight', 'bias', 'om.weight', 'om.bias'), got, g64, g32):
        bar = max(4 * rel_err(r32.double(), r64), EXACT_BAR)
        e = rel_err(a.double(), r64)
        row[n] = (e, bar)
        print('DCN module %s: rel_err %.3e bar %.3e' % (n, e, bar))
        assert e <= bar, (n, e, bar)


def test_two_backwards_accumulate():
    from yolact_amd import dcn_v2
    x, off, mask, w, b, gy, stride = make_case(*SMALL, 4400)
    ts = [t.to(DEV).requires_grad_(True) for t in (x, off, mask, w, b)]
    dcn_v2.dcn_v2_conv(*ts, stride, 1, 1, 1).backward(gy.to(DEV))
    once = [t.grad.clone() for t in ts]
    dcn_v2.dcn_v2_conv(*ts, stride, 1, 1, 1).backward(gy.to(DEV))
    for n, t, o in zip(NAMES, ts, once):
        assert _close(t.grad.cpu(), 2 * o.cpu()), n


def test_side_stream_and_non_contiguous_gy():
    from yolact_amd import dcn_v2
    case = make_case(*SMALL, 4500)
    x, off, mask, w, b, gy, stride = case
    _, want = gpu_grads(case)
    ts = [t.to(DEV).requires_grad_(True) for t in (x, off, mask, w, b)]
    gy_nc = gy.permute(0, 2, 3, 1).contiguous().to(DEV).permute(0, 3, 1, 2)       # NCHW view of NHWC memory
    assert not gy_nc.is_contiguous()
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        y = dcn_v2.dcn_v2_conv(*ts, stride, 1, 1, 1)
        y.backward(gy_nc)
    s.synchronize()
    torch.cuda.synchronize()
    for n, t, f in zip(NAMES, ts, want):
        assert _close(t.grad.cpu(), f), n


def test_reference_gradcheck_recorded_not_gated():
    """external/DCNv2/test.py:69-97 restated with its sizes: an fp32 finite-difference check (eps 1e-3, atol 1e-4, rtol 1e-2),
    flaky by construction (kinks within eps of a sample point).  Run once with a fixed seed; the outcome is printed and recorded
    in DESIGN.md, not asserted — test_gradients_* are the gate."""
    from torch.autograd import gradcheck
    from yolact_amd import dcn_v2
    g = _g(5000)
    N, inC, inH, inW, outC = 2, 2, 4, 4, 2
    inp = (torch.rand(N, inC, inH, inW, generator=g) * 0.01).to(DEV).requires_grad_(True)
    offset = (torch.randn(N, 18, inH, inW, generator=g) * 2).to(DEV).requires_grad_(True)
    mask = torch.sigmoid(torch.rand(N, 9, inH, inW, generator=g).to(DEV).requires_grad_(True))
    weight = torch.randn(outC, inC, 3, 3, generator=g).to(DEV).requires_grad_(True)
    bias = torch.rand(outC, generator=g).to(DEV).requires_grad_(True)
    try:
        ok = gradcheck(dcn_v2.dcn_v2_conv, (inp, offset, mask, weight, bias, 1, 1, 1, 1), eps=1e-3, atol=1e-4, rtol=1e-2,
                       raise_exception=False, nondet_tol=1e-5)
    except Exception as e:      # (fp32 inputs: gradcheck may refuse outright on some torch versions)
        ok = 'error: %s' % type(e).__name__
    print('reference gradcheck (fp32, eps 1e-3, atol 1e-4, rtol 1e-2): %s' % ok)
