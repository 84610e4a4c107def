"""The fp64 oracle of the train path's deformable convolution (yolact_amd/layers/train_ops.py deform_conv, dcn_bottleneck) and the
cases tests/test_gpu_dcn_train.py runs, built here so that tests/test_dcn_train_host.py can certify them on the CPU.

    deform_conv_ref(x, om, w, b, stride)   tests/dcn_ref.py::dcn_ref on om's 18 offset channels and the sigmoid of its 9 mask logits
                                            (NCHW; gradients from torch autograd on fp64 leaves: tests/test_dcn_bwd_host.py pins that)
    deform_conv_f32(..)                     the same formulation in fp32 arithmetic (test_gpu_dcn_bwd.dcn_f32): the yardstick of the
                                            bar max(4 * rel_err(g32, g64), 8e-6), never an oracle
    dcn_bottleneck_ref(..)                  backbone.py:37-57 with a DCN as conv2, from conv_plain_ref and bn_ref of
                                            tests/backbone_train_ref.py
Everything is NCHW on the CPU; om is [B,27,Ho,Wo].  `wrong` selects a deliberately wrong variant (the host test shows that the bars
reject them): 'no_sigmoid_grad' keeps the values and drops the sigmoid's derivative, 'swapped_offsets' reads dw where dh belongs.
"""
import math

import torch
import torch.nn.functional as F

import backbone_train_ref as R
import helpers
from dcn_ref import dcn_ref, out_hw, sample_points
from test_gpu_dcn_bwd import _base, dcn_f32, off_kink_offsets

EXACT_BAR = 8e-6
OP_NAMES = ('y', 'x', 'om', 'weight', 'bias')


def _split(om, wrong=None):
    off, logit = om[:, :18], om[:, 18:]
    mask = torch.sigmoid(logit)
    if wrong == 'no_sigmoid_grad':
        mask = mask.detach() + (logit - logit.detach())
    elif wrong == 'swapped_offsets':
        off = torch.stack([off[:, 1::2], off[:, 0::2]], 2).reshape(off.shape)
    else:
        assert wrong is None
    return off, mask


def deform_conv_ref(x, om, w, b, stride, wrong=None):
    off, mask = _split(om, wrong)
    return dcn_ref(x, off, mask, w, b, stride, 1)


def deform_conv_f32(x, om, w, b, stride):
    off, mask = _split(om)
    return dcn_f32(x, off, mask, w, b, stride)


def op_grads(case, dtype, wrong=None):
    """case = (x, om, w, b or None, gy, stride) -> dict y, x, om, weight, bias (the last absent without a bias): the output and the
    gradients of <y, gy>."""
    x, om, w, b, gy, stride = case
    leaves = [t.detach().to(dtype).requires_grad_(True) for t in (x, om, w) + ((b,) if b is not None else ())]
    bb = leaves[3] if b is not None else None
    with helpers.oracle_threads():
        y = deform_conv_ref(leaves[0], leaves[1], leaves[2], bb, stride, wrong) if dtype == torch.float64 else \
            deform_conv_f32(leaves[0], leaves[1], leaves[2], bb, stride)
        g = torch.autograd.grad((y * gy.to(dtype)).sum(), leaves)
    out = dict(y=y.detach(), x=g[0], om=g[1], weight=g[2])
    if b is not None:
        out['bias'] = g[3]
    return out


def bars(g64, g32):
    return {k: max(4 * helpers.rel_err(g32[k], g64[k]), EXACT_BAR) for k in g64}


# ---- the cases of the op ------------------------------------------------------------------------------------------------------------------
#            B, Cin, Cout, H, W, stride, bias
OP_CASES = {'c32_o20_9x11_s1_b2': (2, 32, 20, 9, 11, 1, True), 'c64_o32_13x17_s1_b1_nobias': (1, 64, 32, 13, 17, 1, False),
            'c32_o32_12x10_s2_b1': (1, 32, 32, 12, 10, 2, True), 'c64_o20_13x17_s2_b2_nobias': (2, 64, 20, 13, 17, 2, False),
            'c128_35_s2': (2, 128, 128, 35, 35, 2, True), 'c512_18_s1': (2, 512, 512, 18, 18, 1, True)}
SMALL = 'c32_o20_9x11_s1_b2'


def make_op_case(B, Cin, Cout, H, W, stride, bias, seed, spread=2.0):
    """x ~ N(0, 1), w ~ N(0, 2 / fan_in), offsets ~ N(0, spread^2) moved off the bilinear kinks (off_kink_offsets), logits ~ N(0, 1),
    gy ~ N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    Ho, Wo = out_hw(H, W, stride, 1)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * math.sqrt(2.0 / (9 * Cin))
    b = torch.randn(Cout, generator=g) if bias else None
    logit = torch.randn(B, 9, Ho, Wo, generator=g)
    off = off_kink_offsets(torch.randn(B, 18, Ho, Wo, generator=g) * spread, H, W, stride)
    gy = torch.randn(B, Cout, Ho, Wo, generator=g)
    return x, torch.cat([off, logit], 1), w, b, gy, stride


def op_case(name):
    return make_op_case(*OP_CASES[name], seed=7000 + sum(map(ord, name)))


def aim_offsets(H, W, stride, B, th, tw):
    """Offsets [B,18,Ho,Wo] that put tap k of every output pixel at (th, tw)[..., k, oy, ox] (tensors broadcastable to [B,9,Ho,Wo])."""
    Ho, Wo = out_hw(H, W, stride, 1)
    bh, bw = _base(H, W, stride)
    dh = (torch.as_tensor(th, dtype=torch.float32) - bh).expand(B, 9, Ho, Wo)
    dw = (torch.as_tensor(tw, dtype=torch.float32) - bw).expand(B, 9, Ho, Wo)
    return torch.stack([dh, dw], 2).reshape(B, 18, Ho, Wo).contiguous()


def adversarial_case(seed=7100):
    """B = 1, 9 x 9, Cin = 32: every sample point of every tap lies in the one cell [4, 5] x [4, 5], at (4.5, 4.5) + multiples of 1/16
    up to +- 3/8.  The four pixels around it hold 9 * 81 entries each; every other pixel of gx holds none."""
    B, Cin, Cout, H, W, stride = 1, 32, 32, 9, 9, 1
    x, om, w, b, gy, _ = make_op_case(B, Cin, Cout, H, W, stride, True, seed)
    g = torch.Generator().manual_seed(seed + 1)
    jit = lambda: torch.randint(-6, 7, (B, 9, H, W), generator=g).float() / 16
    om = torch.cat([aim_offsets(H, W, stride, B, 4.5 + jit(), 4.5 + jit()), om[:, 18:]], 1)
    return x, om, w, b, gy, stride


def outside_case(seed=7200):
    """Every point outside the image: h in [-6, -2] (dyadic), any w."""
    B, Cin, Cout, H, W, stride = 2, 32, 20, 9, 11, 1
    x, om, w, b, gy, _ = make_op_case(B, Cin, Cout, H, W, stride, True, seed)
    g = torch.Generator().manual_seed(seed + 1)
    th = -2.0 - torch.randint(0, 65, (B, 9, H, W), generator=g).float() / 16
    h, wc = sample_points(H, W, om[:, :18], stride, 1)
    return x, torch.cat([aim_offsets(H, W, stride, B, th, wc), om[:, 18:]], 1), w, b, gy, stride


BAND = (4, 7)                     # the input rows band_case samples (inclusive)


def band_case(seed=7300):
    """13 x 17: every point's h lies in [4 + 1/16, 7 - 1/16], so only the rows 4 .. 7 of x are read; w as drawn."""
    B, Cin, Cout, H, W, stride = 2, 32, 20, 13, 17, 1
    x, om, w, b, gy, _ = make_op_case(B, Cin, Cout, H, W, stride, True, seed)
    g = torch.Generator().manual_seed(seed + 1)
    th = 4.0 + (1 + torch.randint(0, 47, (B, 9, H, W), generator=g).float()) / 16
    th = torch.where((th - th.floor()) == 0, th + 1 / 16, th)
    h, wc = sample_points(H, W, om[:, :18], stride, 1)
    off = off_kink_offsets(aim_offsets(H, W, stride, B, th, wc), H, W, stride)
    return x, torch.cat([off, om[:, 18:]], 1), w, b, gy, stride


def zero_om_case(seed=7400):
    """om = 0 (a DCN's initial state): every point on a kink, every modulation 1/2."""
    B, Cin, Cout, H, W, stride = 2, 32, 32, 9, 11, 1
    x, om, w, b, gy, _ = make_op_case(B, Cin, Cout, H, W, stride, True, seed)
    return x, torch.zeros_like(om), w, b, gy, stride


def point_fractions(case):
    """(smallest, largest) fraction of any fp32 sample coordinate of the case, and whether every fp32 point lies in its fp64 point's
    cell."""
    x, om, _, _, _, stride = case
    H, W = x.shape[2:]
    h, w = sample_points(H, W, om[:, :18], stride, 1)
    bh, bw = _base(H, W, stride)
    h64, w64 = bh.double() + om[:, 0:18:2].double(), bw.double() + om[:, 1:18:2].double()
    fr = torch.cat([(h - h.floor()).reshape(-1), (w - w.floor()).reshape(-1)])
    same = torch.equal(h.floor().double(), h64.floor()) and torch.equal(w.floor().double(), w64.floor())
    return fr.min().item(), fr.max().item(), same


# ---- the DCN bottleneck -------------------------------------------------------------------------------------------------------------------
DCN_NAMES = ('conv2.bias', 'conv2.conv_offset_mask.weight', 'conv2.conv_offset_mask.bias')
#              inplanes, planes, stride, projection   (a block without projection needs inplanes = 4 planes)
BLOCK_SPECS = {'identity_s1': (128, 32, 1, False), 'proj_s2': (64, 32, 2, True)}
BLOCK_X = (9, 7)
# per (variant, batch statistics): find_block_seed on the CPU (32 times the fp32 deviation at every ReLU, fractions in [1/8, 7/8]; the
# host test asserts 16 times)
BLOCK_SEEDS = {('identity_s1', False): 1, ('identity_s1', True): 5, ('proj_s2', False): 1, ('proj_s2', True): 3}
OM_TAP_FRACTIONS = (0.25, 0.375, 0.5, 0.625, 0.75)


def dcn_block_params(g, inplanes, planes, projection):
    """random_block_params plus the DCN's own: conv2.bias ~ N(0, 0.1); conv_offset_mask.weight ~ N(0, 0.02^2 / fan_in) (small: the
    offsets move by a few hundredths around their biases); its bias per offset channel an integer in -2 .. 2 plus a fraction of
    OM_TAP_FRACTIONS, per logit channel N(0, 1)."""
    P = R.random_block_params(g, inplanes, planes, projection)
    P['conv2.bias'] = R.grid((torch.randn(planes, generator=g) * 0.1).clamp(-0.9, 0.9), R.PARAM_GRID)
    P['conv2.conv_offset_mask.weight'] = torch.randn(27, planes, 3, 3, generator=g) * (0.02 / math.sqrt(9 * planes))
    whole = torch.randint(-2, 3, (18,), generator=g).float()
    frac = torch.tensor(OM_TAP_FRACTIONS)[torch.randint(0, len(OM_TAP_FRACTIONS), (18,), generator=g)]
    P['conv2.conv_offset_mask.bias'] = torch.cat([whole + frac, torch.randn(9, generator=g)])
    return P


def dcn_bottleneck_ref(x, P, stride, batch_stats, keep=None, new_stats=None, oms=None, wrong=None):
    """backbone.py:37-57 with conv2 a DCN (dcn_v2.py:118-128).  keep / new_stats as bottleneck_ref; oms receives conv_offset_mask's
    output.  The arithmetic follows x's dtype: dcn_ref (fp64) or dcn_f32."""
    def bn(z, name):
        y, nm, nv, _, _ = R.bn_ref(z, P[name + '.weight'], P[name + '.bias'], P[name + '.running_mean'], P[name + '.running_var'],
                                   batch_stats)
        if new_stats is not None:
            new_stats[name + '.running_mean'], new_stats[name + '.running_var'] = nm, nv
        return y

    def relu(z, name):
        a = F.relu(z)
        if keep is not None:
            keep.append((name, z, a))
        return a
    out = relu(bn(R.conv_plain_ref(x, P['conv1.weight']), 'bn1'), 'relu1')
    om = F.conv2d(out, P['conv2.conv_offset_mask.weight'], P['conv2.conv_offset_mask.bias'], stride=stride, padding=1)
    if oms is not None:
        oms.append(om)
    if x.dtype == torch.float64:
        out = deform_conv_ref(out, om, P['conv2.weight'], P['conv2.bias'], stride, wrong)
    else:
        out = deform_conv_f32(out, om, P['conv2.weight'], P['conv2.bias'], stride)
    out = relu(bn(out, 'bn2'), 'relu2')
    out = bn(R.conv_plain_ref(out, P['conv3.weight']), 'bn3')
    res = x
    if 'downsample.0.weight' in P:
        res = bn(R.conv_plain_ref(x, P['downsample.0.weight'], stride), 'downsample.1')
    return relu(out + res, 'relu3')


def run_block_ref(x, params, stride, up, batch_stats, dtype, keep=None, oms=None, wrong=None):
    """-> dict y, d_x, d_<name> per parameter that takes a gradient, new_<name> per running statistic (R.run_ref's layout)."""
    leaf = x.detach().to(dtype).requires_grad_(True)
    names = [n for n in params if R.is_leaf_name(n)]
    P = {n: params[n].detach().to(dtype) for n in params}
    for n in names:
        P[n].requires_grad_(True)
    new_stats = {}
    with helpers.oracle_threads():
        y = dcn_bottleneck_ref(leaf, P, stride, batch_stats, keep, new_stats, oms, wrong)
        total = (y * up.to(dtype)).sum()
        g = torch.autograd.grad(total, [leaf] + [P[n] for n in names], retain_graph=keep is not None)
    res = {'y': y.detach(), 'd_x': g[0]}
    res.update({'d_' + n: t for n, t in zip(names, g[1:])})
    res.update({'new_' + n: t.detach() for n, t in new_stats.items()})
    res['_total'] = total
    return res


def block_margins(x, params, stride, up, batch_stats):
    """(ReLU margins as R.relu_margins gives them, (smallest, largest) fraction of a sample coordinate over both oracles, every
    fp32 point in its fp64 point's cell)."""
    res, pts = {}, {}
    with helpers.oracle_threads():
        for dtype in (torch.float64, torch.float32):
            keep, oms = [], []
            r = run_block_ref(x, params, stride, up, batch_stats, dtype, keep, oms)
            ga = torch.autograd.grad(r['_total'], [a for _, _, a in keep], allow_unused=True)
            res[dtype] = [(n, z.detach(), torch.zeros_like(a) if g is None else g) for (n, z, a), g in zip(keep, ga)]
            om = oms[0].detach()
            H, W = keep[0][1].shape[2:]
            pts[dtype] = sample_points(H, W, om[:, :18], stride, 1)          # (fp32 points of each oracle's own offsets)
    relus = []
    for (n, z64, g), (_, z32, _) in zip(res[torch.float64], res[torch.float32]):
        hit = g != 0
        relus.append((n, z64[hit].abs().min().item() if hit.any() else float('inf'), (z32.double() - z64).abs().max().item()))
    fr = torch.cat([(c - c.floor()).reshape(-1) for dt in pts for c in pts[dt]])
    same = all(torch.equal(a.floor(), b.floor()) for a, b in zip(pts[torch.float64], pts[torch.float32]))
    return relus, (fr.min().item(), fr.max().item()), same


def block_case(variant, batch_stats, seed=None):
    """-> (spec, x, params, up)."""
    spec = BLOCK_SPECS[variant]
    inplanes, planes, stride, projection = spec
    seed = BLOCK_SEEDS[(variant, batch_stats)] if seed is None else seed
    g = torch.Generator().manual_seed(8000 + seed)
    x = R.grid(torch.randn(2, inplanes, *BLOCK_X, generator=g).clamp(-4, 4), 256)
    params = dcn_block_params(g, inplanes, planes, projection)
    up = torch.randint(-2, 3, R.out_shape(tuple(x.shape), [spec]), generator=g).float() / 2
    return spec, x, params, up


def block_ok(variant, batch_stats, seed, factor=16, lo=1 / 8):
    spec, x, params, up = block_case(variant, batch_stats, seed)
    relus, (fmin, fmax), same = block_margins(x, params, spec[2], up, batch_stats)
    return same and fmin >= lo and fmax <= 1 - lo and all(m >= factor * dev for _, m, dev in relus)


def find_block_seed(variant, batch_stats, last=40, factor=32):
    """The search that chose BLOCK_SEEDS (twice the margin the host test asserts)."""
    for seed in range(1, last + 1):
        if block_ok(variant, batch_stats, seed, factor):
            return seed
    raise AssertionError('no seed keeps the margins')
