"""The train-mode ResNet stages (backbone.py:13-57) in plain torch, written from the semantics: the bias-free convolution, BatchNorm
in both modes (batch statistics with the running update, or the running statistics as they are: the reference's freeze_bn()) and the
bottleneck.  The oracle of tests/test_backbone_train_host.py (pinned there to what the reference's own Bottleneck class computed:
tests/golden/backbone_train.npz, tools/make_golden_backbone_train.py) and of tests/test_gpu_backbone_train.py.

Everything works in the dtype given (fp32 or fp64) on the CPU, NCHW.  A block's parameters are a dict under its state-dict names
(conv1.weight, bn1.weight, bn1.bias, bn1.running_mean, bn1.running_var, .., downsample.0.weight, downsample.1.*); a chain of blocks
prefixes them with '<index>.'.
"""
import numpy as np
import torch
import torch.nn.functional as F

import helpers
from heads_train_ref import PARAM_GRID, assert_margins, grid, rel_err, tightest  # noqa: F401

EPS, MOMENTUM = 1e-5, 0.1
GOLDEN_BLOCKS = ((64, 32, 2, True), (128, 32, 1, False))         # (inplanes, planes, stride, projection)
GOLDEN_X = (2, 64, 9, 7)


def conv_plain_ref(x, w, stride=1):
    return F.conv2d(x, w, None, stride=stride, padding=w.shape[2] // 2)


def bn_ref(x, gamma, beta, rmean, rvar, batch_stats, eps=EPS, momentum=MOMENTUM, unbiased_running=True, xhat_term=True):
    """-> (y, new running_mean, new running_var, mean, invstd).  batch_stats: the statistics of x over (N, H, W), biased variance
    for the normalisation and the unbiased one in the running update; else the running statistics, which stay.  xhat_term=False is a
    deliberately WRONG variant: the same values, but the backward loses its mean(dy * xhat) * xhat term (the variance is a constant)."""
    dims = [d for d in range(x.dim()) if d != 1]
    shape = [1, -1] + [1] * (x.dim() - 2)
    if batch_stats:
        n = x.numel() // x.shape[1]
        mean = x.mean(dims)
        var = ((x - mean.view(shape)) ** 2).mean(dims)
        with torch.no_grad():
            new_mean = (1 - momentum) * rmean + momentum * mean.detach()
            new_var = (1 - momentum) * rvar + momentum * var.detach() * ((n / (n - 1)) if unbiased_running else 1.0)
    else:
        mean, var, new_mean, new_var = rmean, rvar, rmean, rvar
    invstd = 1 / torch.sqrt((var if xhat_term else var.detach()) + eps)
    y = gamma.view(shape) * ((x - mean.view(shape)) * invstd.view(shape)) + beta.view(shape)
    return y, new_mean, new_var, mean, invstd


def block_param_names(projection):
    names = []
    for i in (1, 2, 3):
        names += ['conv%d.weight' % i] + ['bn%d.%s' % (i, s) for s in ('weight', 'bias', 'running_mean', 'running_var')]
    if projection:
        names += ['downsample.0.weight'] + ['downsample.1.%s' % s for s in ('weight', 'bias', 'running_mean', 'running_var')]
    return names


def block_param_shapes(inplanes, planes, projection):
    shapes = {'conv1.weight': (planes, inplanes, 1, 1), 'conv2.weight': (planes, planes, 3, 3), 'conv3.weight': (4 * planes, planes, 1, 1)}
    for i, c in ((1, planes), (2, planes), (3, 4 * planes)):
        for s in ('weight', 'bias', 'running_mean', 'running_var'):
            shapes['bn%d.%s' % (i, s)] = (c,)
    if projection:
        shapes['downsample.0.weight'] = (4 * planes, inplanes, 1, 1)
        for s in ('weight', 'bias', 'running_mean', 'running_var'):
            shapes['downsample.1.%s' % s] = (4 * planes,)
    return {n: shapes[n] for n in block_param_names(projection)}


def is_leaf_name(n):
    """The parameters that take a gradient: everything but the running statistics."""
    return 'running' not in n


def bottleneck_ref(x, P, stride, batch_stats, prefix='', keep=None, new_stats=None, stride_on_conv1=False, **bn_kw):
    """backbone.py:37-57.  keep receives (name, pre-activation, activation) of every ReLU; new_stats the updated running statistics;
    bn_kw goes to bn_ref (unbiased_running, momentum, xhat_term)."""
    def bn(z, name):
        y, nm, nv, _, _ = bn_ref(z, P[prefix + name + '.weight'], P[prefix + name + '.bias'], P[prefix + name + '.running_mean'],
                                 P[prefix + name + '.running_var'], batch_stats, **bn_kw)
        if new_stats is not None:
            new_stats[prefix + name + '.running_mean'], new_stats[prefix + name + '.running_var'] = nm, nv
        return y

    def relu(z, name):
        a = F.relu(z)
        if keep is not None:
            keep.append((prefix + name, z, a))
        return a
    s1, s2 = (stride, 1) if stride_on_conv1 else (1, stride)
    out = relu(bn(conv_plain_ref(x, P[prefix + 'conv1.weight'], s1), 'bn1'), 'relu1')
    out = relu(bn(conv_plain_ref(out, P[prefix + 'conv2.weight'], s2), 'bn2'), 'relu2')
    out = bn(conv_plain_ref(out, P[prefix + 'conv3.weight']), 'bn3')
    res = x
    if prefix + 'downsample.0.weight' in P:
        res = bn(conv_plain_ref(x, P[prefix + 'downsample.0.weight'], stride), 'downsample.1')
    return relu(out + res, 'relu3')


def chain_ref(x, P, blocks, batch_stats, keep=None, new_stats=None, **kw):
    """blocks: [(prefix, stride), ..] -> the output of every block."""
    outs = []
    for prefix, stride in blocks:
        x = bottleneck_ref(x, P, stride, batch_stats, prefix, keep, new_stats, **kw)
        outs.append(x)
    return outs


def run_ref(x, params, blocks, up, batch_stats, dtype, keep=None, ups=None, **kw):
    """Forward of the chain and the gradients of <last output, up> -> dict('y' -> output, 'd_x', 'd_<name>' per parameter that takes a
    gradient, 'new_<name>' per running statistic).  ups (one upstream gradient per block output, `up` is then None): the gradients of
    sum_i <output i, ups[i]>, every block output with two consumers but the last, and 'out<i>' per block in place of 'y'."""
    leaf = x.detach().to(dtype).requires_grad_(True)
    names = [n for n in params if is_leaf_name(n)]
    P = {n: params[n].detach().to(dtype) for n in params}
    for n in names:
        P[n].requires_grad_(True)
    new_stats = {}
    with helpers.oracle_threads():                       # torch's CPU summation order depends on the thread count
        outs = chain_ref(leaf, P, blocks, batch_stats, keep, new_stats, **kw)
        if ups is None:
            total = (outs[-1] * up.to(dtype)).sum()
        else:
            assert up is None and len(ups) == len(outs)
            total = sum((o * u.to(dtype)).sum() for o, u in zip(outs, ups))
        g = torch.autograd.grad(total, [leaf] + [P[n] for n in names], retain_graph=keep is not None)
    res = {'y': outs[-1].detach()} if ups is None else {'out%d' % i: o.detach() for i, o in enumerate(outs)}
    res['d_x'] = g[0]
    res.update({'d_' + n: t for n, t in zip(names, g[1:])})
    res.update({'new_' + n: t.detach() for n, t in new_stats.items()})
    res['_total'], res['_outs'] = total, outs
    return res


def relu_margins(x, params, blocks, up, batch_stats, ups=None):
    """Per ReLU: (name, the smallest |pre-activation| whose activation receives gradient, in fp64; the largest fp32-versus-fp64
    deviation of that tensor)."""
    res = {}
    with helpers.oracle_threads():
        for dtype in (torch.float64, torch.float32):
            keep = []
            r = run_ref(x, params, blocks, up, batch_stats, dtype, keep, ups=ups)
            ga = torch.autograd.grad(r['_total'], [a for _, _, a in keep], allow_unused=True)
            res[dtype] = [(n, z.detach(), torch.zeros_like(a) if g is None else g) for (n, z, a), g in zip(keep, ga)]
    out = []
    for (n, z64, g), (_, z32, _) in zip(res[torch.float64], res[torch.float32]):
        hit = g != 0
        out.append((n, z64[hit].abs().min().item() if hit.any() else float('inf'), (z32.double() - z64).abs().max().item()))
    return out


def random_block_params(g, inplanes, planes, projection, prefix=''):
    """On fp16-exact grids: weights ~ N(0, 2 / fan_in) in 1/2048, gamma in [0.5, 1.5], beta ~ N(0, 0.1), running_mean ~ N(0, 0.25),
    running_var in [0.5, 1.5] (these two in 1/1024), the rest in 1/2048: non-trivial running statistics."""
    params = {}
    for n, shp in block_param_shapes(inplanes, planes, projection).items():
        wide = n.endswith('running_var') or (n.endswith('weight') and len(shp) == 1)     # up to 1.5: fp16 holds 1/1024 there
        if n.endswith('running_var') or (n.endswith('weight') and len(shp) == 1):
            t = 0.5 + torch.rand(*shp, generator=g)
        elif n.endswith('running_mean'):
            t = (torch.randn(*shp, generator=g) * 0.25).clamp(-0.9, 0.9)
        elif len(shp) == 1:
            t = (torch.randn(*shp, generator=g) * 0.1).clamp(-0.9, 0.9)
        else:
            t = (torch.randn(*shp, generator=g) * (2.0 / (shp[1] * shp[2] * shp[3])) ** 0.5).clamp(-0.9, 0.9)
        params[prefix + n] = grid(t, 1024 if wide else PARAM_GRID)
    return params


def out_shape(xshape, specs):
    B, _, H, W = xshape
    for _, planes, stride, _ in specs:
        if stride == 2:
            H, W = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return (B, 4 * specs[-1][1], H, W)


def random_case(seed, xshape, specs):
    """specs: [(inplanes, planes, stride, projection), ..] -> (x, params, blocks, up): x ~ N(0, 1) in 1/256, the upstream gradient of
    the last output in {-1, -1/2, 0, 1/2, 1}."""
    g = torch.Generator().manual_seed(seed)
    x = grid(torch.randn(*xshape, generator=g).clamp(-4, 4), 256)
    params, blocks = {}, []
    for i, (inplanes, planes, stride, projection) in enumerate(specs):
        prefix = '%d.' % i if len(specs) > 1 else ''
        params.update(random_block_params(g, inplanes, planes, projection, prefix))
        blocks.append((prefix, stride))
    up = torch.randint(-2, 3, out_shape(xshape, specs), generator=g).float() / 2
    return x, params, blocks, up


def find_seed(xshape, specs, modes=(False, True), first=1, last=200, factor=16, ups=None):
    """The first seed whose case keeps `factor` times the fp32 deviation at every ReLU in every mode -> (seed, tried).  ups: as in
    run_ref, the same for every seed (the case's own `up` is then not used)."""
    for seed in range(first, last + 1):
        x, params, blocks, up = random_case(seed, xshape, specs)
        if all(all(lo >= factor * dev for _, lo, dev in relu_margins(x, params, blocks, None if ups else up, m, ups)) for m in modes):
            return seed, seed - first + 1
    raise AssertionError('no seed in %d .. %d keeps the margin' % (first, last))


# ---- the stored reference results ---------------------------------------------------------------------------------------------------
def load_golden():
    """tests/golden/backbone_train.npz -> (meta, x, params {name: fp32}, blocks, up, want {'eval' / 'train': {name: fp32}})."""
    meta, z = helpers.load_golden('backbone_train')
    x = torch.from_numpy(z['x'].astype(np.float32))
    params = {n: torch.from_numpy(z['p_' + n].astype(np.float32)) for n in meta['params']}
    up = torch.from_numpy(z['up'].astype(np.float32))
    want = {mode: {k[len(mode) + 1:]: torch.from_numpy(z[k]) for k in z if k.startswith(mode + '_')} for mode in ('eval', 'train')}
    blocks = [(p, s) for p, s in meta['blocks']]
    return meta, x, params, blocks, up, want
