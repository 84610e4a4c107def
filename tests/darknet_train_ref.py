"""The train-mode DarkNet53 backbone (backbone.py:222-294) in plain torch, written from the layout of yolact_amd/modules.py: the unit
(a bias-free convolution with padding k // 2, BatchNorm2d in both modes, LeakyReLU(0.1)), the DarkNetBlock (conv2(conv1(x)) + x: the
residual is added BEHIND conv2's activation) and the whole backbone (_preconv, then five stages of a stride-2 unit and its blocks).
The oracle of tests/test_darknet_train_host.py (pinned there to what the reference's own darknetconvlayer / DarkNetBlock computed:
tests/golden/darknet_train.npz, tools/make_golden_darknet_train.py) and of tests/test_gpu_darknet_train.py.

Everything works in the dtype given (fp32 or fp64) on the CPU, NCHW.  Parameters are a dict under the state-dict names of the
Sequentials: '<unit>0.weight', '<unit>1.weight', '<unit>1.bias', '<unit>1.running_mean', '<unit>1.running_var'; a block's units are
'conv1.' and 'conv2.'; the backbone's are '_preconv.', 'layers.<i>.0.' and 'layers.<i>.<j>.conv1.' / '.conv2.'.

A case is a `net`: a list of steps, each ('unit', prefix, stride) or ('block', prefix), and `taps`: the indices of the steps whose
outputs are returned (the last one alone when None).

Kink condition.  LeakyReLU has two slopes, so every pre-activation z decides which one its gradient takes.  A case is decidable when
the smallest |z| whose activation receives gradient is at least `factor` times the fp32-versus-fp64 deviation of that tensor.
"""
import numpy as np
import torch
import torch.nn.functional as F

import helpers
from backbone_train_ref import EPS, MOMENTUM, bn_ref, conv_plain_ref, is_leaf_name  # noqa: F401
from heads_train_ref import PARAM_GRID, assert_margins, grid, rel_err, tightest  # noqa: F401

SLOPE = 0.1
BN_SUFFIXES = ('weight', 'bias', 'running_mean', 'running_var')
# the golden cases (tools/make_golden_darknet_train.py): name -> (net, input shape, unit shapes {prefix: (cin, cout, k)})
GOLDEN_CASES = {
    'pre': ([('unit', '', 1)], (2, 3, 9, 7), {'': (3, 32, 3)}),
    'down': ([('unit', '', 2)], (2, 32, 9, 7), {'': (32, 64, 3)}),
    'block': ([('block', '')], (2, 64, 9, 7), {'conv1.': (64, 32, 1), 'conv2.': (32, 64, 3)}),
}


def leaky(z, slope=SLOPE):
    """nn.LeakyReLU(slope): z > 0 ? z : slope * z."""
    return torch.where(z > 0, z, z * slope)


def unit_ref(x, P, prefix, stride, batch_stats, keep=None, new_stats=None, residual=None, slope=SLOPE, residual_first=False, **bn_kw):
    """conv, BatchNorm2d, LeakyReLU (+ residual).  keep receives (name, pre-activation, activation); new_stats the updated running
    statistics; bn_kw goes to bn_ref.  slope and residual_first = True (the sum BEFORE the activation, the bottleneck's form) are the
    deliberately WRONG variants."""
    c = conv_plain_ref(x, P[prefix + '0.weight'], stride)
    z, nm, nv, _, _ = bn_ref(c, *(P[prefix + '1.' + s] for s in BN_SUFFIXES), batch_stats, **bn_kw)
    if new_stats is not None:
        new_stats[prefix + '1.running_mean'], new_stats[prefix + '1.running_var'] = nm, nv
    if residual is not None and residual_first:
        z = z + residual
    a = leaky(z, slope)
    if keep is not None:
        keep.append((prefix + 'leaky', z, a))
    return a + residual if (residual is not None and not residual_first) else a


def block_ref(x, P, prefix, batch_stats, keep=None, new_stats=None, **kw):
    """backbone.py:246-247: conv2(conv1(x)) + x."""
    h = unit_ref(x, P, prefix + 'conv1.', 1, batch_stats, keep, new_stats, **kw)
    return unit_ref(h, P, prefix + 'conv2.', 1, batch_stats, keep, new_stats, residual=x, **kw)


def net_ref(x, P, net, batch_stats, keep=None, new_stats=None, **kw):
    """-> the output of every step."""
    outs = []
    for step in net:
        if step[0] == 'unit':
            x = unit_ref(x, P, step[1], step[2], batch_stats, keep, new_stats, **kw)
        else:
            x = block_ref(x, P, step[1], batch_stats, keep, new_stats, **kw)
        outs.append(x)
    return outs


def backbone_net(layers):
    """A DarkNetBackbone(layers) as (net, taps, unit shapes): one tap behind the last block of every stage."""
    net, taps, shapes = [('unit', '_preconv.', 1)], [], {'_preconv.': (3, 32, 3)}
    cin = 32
    for i, (ch, n) in enumerate(zip((32, 64, 128, 256, 512), layers)):
        net.append(('unit', 'layers.%d.0.' % i, 2))
        shapes['layers.%d.0.' % i] = (cin, 2 * ch, 3)
        cin = 2 * ch
        for j in range(1, n + 1):
            net.append(('block', 'layers.%d.%d.' % (i, j)))
            shapes['layers.%d.%d.conv1.' % (i, j)] = (cin, ch, 1)
            shapes['layers.%d.%d.conv2.' % (i, j)] = (ch, cin, 3)
        taps.append(len(net) - 1)
    return net, taps, shapes


def run_ref(x, params, net, ups, batch_stats, dtype, keep=None, taps=None, x_grad=True, **kw):
    """Forward and the gradients of sum_i <tapped output i, ups[i]> -> dict('y' (one tap) or 'out<i>', 'd_x' when x_grad, 'd_<name>' per
    parameter that takes a gradient, 'new_<name>' per running statistic).  ups: one tensor, or one per tap."""
    ups = list(ups) if isinstance(ups, (list, tuple)) else [ups]
    taps = [len(net) - 1] if taps is None else list(taps)
    assert len(ups) == len(taps)
    leaf = x.detach().to(dtype).requires_grad_(bool(x_grad))
    names = [n for n in params if is_leaf_name(n)]
    P = {n: params[n].detach().to(dtype) for n in params}
    for n in names:
        P[n].requires_grad_(True)
    new_stats = {}
    with helpers.oracle_threads():                       # torch's CPU summation order depends on the thread count
        outs = net_ref(leaf, P, net, batch_stats, keep, new_stats, **kw)
        outs = [outs[t] for t in taps]
        total = sum((o * u.to(dtype)).sum() for o, u in zip(outs, ups))
        g = torch.autograd.grad(total, ([leaf] if x_grad else []) + [P[n] for n in names], retain_graph=keep is not None)
    res = {'y': outs[0].detach()} if len(outs) == 1 else {'out%d' % i: o.detach() for i, o in enumerate(outs)}
    if x_grad:
        res['d_x'], g = g[0], g[1:]
    res.update({'d_' + n: t for n, t in zip(names, g)})
    res.update({'new_' + n: t.detach() for n, t in new_stats.items()})
    res['_total'] = total
    return res


def leaky_margins(x, params, net, ups, batch_stats, taps=None, x_grad=True):
    """Per LeakyReLU: (name, the smallest |pre-activation| whose activation receives gradient, in fp64; the largest fp32-versus-fp64
    deviation of that tensor)."""
    res = {}
    with helpers.oracle_threads():
        for dtype in (torch.float64, torch.float32):
            keep = []
            r = run_ref(x, params, net, ups, batch_stats, dtype, keep, taps, x_grad)
            ga = torch.autograd.grad(r['_total'], [a for _, _, a in keep], allow_unused=True)
            res[dtype] = [(n, z.detach(), torch.zeros_like(a) if g is None else g) for (n, z, a), g in zip(keep, ga)]
    out = []
    for (n, z64, g), (_, z32, _) in zip(res[torch.float64], res[torch.float32]):
        hit = g != 0
        out.append((n, z64[hit].abs().min().item() if hit.any() else float('inf'), (z32.double() - z64).abs().max().item()))
    return out


def random_unit_params(g, cin, cout, k, prefix=''):
    """On fp16-exact grids: the weight ~ N(0, 2 / fan_in) in 1/2048, gamma and running_var in [0.5, 1.5] in 1/1024, beta ~ N(0, 0.1)
    and running_mean ~ N(0, 0.25) in 1/2048: non-trivial running statistics."""
    return {prefix + '0.weight': grid((torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5).clamp(-0.9, 0.9), PARAM_GRID),
            prefix + '1.weight': grid(0.5 + torch.rand(cout, generator=g), 1024),
            prefix + '1.bias': grid((torch.randn(cout, generator=g) * 0.1).clamp(-0.9, 0.9), PARAM_GRID),
            prefix + '1.running_mean': grid((torch.randn(cout, generator=g) * 0.25).clamp(-0.9, 0.9), PARAM_GRID),
            prefix + '1.running_var': grid(0.5 + torch.rand(cout, generator=g), 1024)}


def out_shapes(xshape, net, shapes):
    """The shape of every step's output."""
    B, _, H, W = xshape
    res = []
    for step in net:
        if step[0] == 'unit':
            if step[2] == 2:
                H, W = (H - 1) // 2 + 1, (W - 1) // 2 + 1
            c = shapes[step[1]][1]
        else:
            c = shapes[step[1] + 'conv2.'][1]
        res.append((B, c, H, W))
    return res


def random_case(seed, xshape, net, shapes, taps=None):
    """-> (x, params, ups): x ~ N(0, 1) in 1/256, the upstream gradient of every tapped output in {-1, -1/2, 0, 1/2, 1}."""
    g = torch.Generator().manual_seed(seed)
    x = grid(torch.randn(*xshape, generator=g).clamp(-4, 4), 256)
    params = {}
    for prefix, (cin, cout, k) in shapes.items():
        params.update(random_unit_params(g, cin, cout, k, prefix))
    osh = out_shapes(xshape, net, shapes)
    taps = [len(net) - 1] if taps is None else taps
    ups = [torch.randint(-2, 3, osh[t], generator=g).float() / 2 for t in taps]
    return x, params, ups


def one_sided_case(seed, xshape, net, shapes, taps=None):
    """random_case for a net too large for it.  A whole backbone has some 2 * 10^5 pre-activations that all receive gradient; drawn as
    in random_case some of them always lie within 16 fp32 deviations of 0 (of the seeds 1 .. 40 on a [2,3,33,29] image the best keeps
    2.6 times the deviation), so no seed meets the kink condition.  Here every channel stays on ONE side of 0: gamma in [1/16, 1/8] and
    beta = +-[3/4, 1], at least six standard deviations of the normalised input, the sign drawn per channel (both slopes are used, a
    channel at a time); and the running statistics are the batch's own (fp64, rounded to 1/256, the variance at least 1/4), as a
    trained network's are, so that the frozen mode normalises too."""
    x, params, ups = random_case(seed, xshape, net, shapes, taps)
    g = torch.Generator().manual_seed(100000 + seed)
    for prefix, (_, cout, _) in shapes.items():
        params[prefix + '1.weight'] = grid(1.0 / 16 + torch.rand(cout, generator=g) / 16, 1024)
        sign = torch.randint(0, 2, (cout,), generator=g).float() * 2 - 1
        params[prefix + '1.bias'] = sign * grid(0.75 + torch.rand(cout, generator=g) / 4, 1024)
    stats = {}
    with helpers.oracle_threads():
        net_ref(x.double(), {n: t.double() for n, t in params.items()}, net, True, None, stats, momentum=1.0)
    for n, t in stats.items():
        t = torch.round(t * 256) / 256
        params[n] = (t.clamp_min(0.25) if n.endswith('running_var') else t).float()
    return x, params, ups


def find_seed(xshape, net, shapes, taps=None, modes=(False, True), first=1, last=200, factor=16, x_grad=True, case=None):
    """The first seed whose case keeps `factor` times the fp32 deviation at every LeakyReLU in every mode -> (seed, tried)."""
    for seed in range(first, last + 1):
        x, params, ups = (case or random_case)(seed, xshape, net, shapes, taps)
        if all(all(lo >= factor * dev for _, lo, dev in leaky_margins(x, params, net, ups, m, taps, x_grad)) for m in modes):
            return seed, seed - first + 1
    raise AssertionError('no seed in %d .. %d keeps the margin' % (first, last))


def bn_case(seed, npos, Cc, residual):
    """The leaky BatchNorm alone on x [npos, C]: -> (x, gamma, beta, running_mean, running_var, res or None, dy): x and res ~ N(0, 1) in
    1/256, the parameters on random_unit_params' grids, dy in {-1, -1/2, 0, 1/2, 1}."""
    g = torch.Generator().manual_seed(seed)
    x = grid(torch.randn(npos, Cc, generator=g).clamp(-4, 4), 256)
    gamma, beta = grid(0.5 + torch.rand(Cc, generator=g), 1024), grid(torch.randn(Cc, generator=g) * 0.1, PARAM_GRID)
    rmean = grid((torch.randn(Cc, generator=g) * 0.25).clamp(-0.9, 0.9), PARAM_GRID)
    rvar = grid(0.5 + torch.rand(Cc, generator=g), 1024)
    res = grid(torch.randn(npos, Cc, generator=g).clamp(-4, 4), 256) if residual else None
    dy = torch.randint(-2, 3, (npos, Cc), generator=g).float() / 2
    return x, gamma, beta, rmean, rvar, res, dy


def bn_leaky_ref(x, gamma, beta, rmean, rvar, res, dy, batch_stats, dtype, keep=None):
    """[npos, C] tensors -> dict(y, mean, invstd, dx, dgamma, dbeta, new_running_mean, new_running_var)."""
    xl, gl, bl = (t.detach().to(dtype).requires_grad_(True) for t in (x, gamma, beta))
    with helpers.oracle_threads():
        z, nm, nv, mean, invstd = bn_ref(xl.t().unsqueeze(0), gl, bl, rmean.to(dtype), rvar.to(dtype), batch_stats)
        z = z.squeeze(0).t()
        a = leaky(z)
        y = a if res is None else a + res.to(dtype)
        dx, dg, db = torch.autograd.grad((y * dy.to(dtype)).sum(), [xl, gl, bl])
    if keep is not None:
        keep['z'] = z.detach()
    return dict(y=y.detach(), mean=mean.detach(), invstd=invstd.detach(), dx=dx, dgamma=dg, dbeta=db, new_running_mean=nm.detach(),
                new_running_var=nv.detach())


def bn_margin(case, batch_stats):
    """(smallest |z| in fp64 of an element whose dy is not 0, largest fp32-versus-fp64 deviation of z)."""
    k64, k32 = {}, {}
    bn_leaky_ref(*case, batch_stats, torch.float64, k64)
    bn_leaky_ref(*case, batch_stats, torch.float32, k32)
    hit = case[6] != 0
    return k64['z'][hit].abs().min().item(), (k32['z'].double() - k64['z']).abs().max().item()


def find_bn_seed(npos, Cc, residual, modes=(False, True), first=1, last=200, factor=16):
    for seed in range(first, last + 1):
        case = bn_case(seed, npos, Cc, residual)
        if all(lo >= factor * dev for lo, dev in (bn_margin(case, m) for m in modes)):
            return seed, seed - first + 1
    raise AssertionError('no seed in %d .. %d keeps the margin' % (first, last))


# ---- the stored reference results ---------------------------------------------------------------------------------------------------
def load_golden():
    """tests/golden/darknet_train.npz -> (meta, {case: (x, params {name: fp32}, up, want {'eval' / 'train': {name: fp32}})})."""
    meta, z = helpers.load_golden('darknet_train')
    cases = {}
    for case in meta['cases']:
        pre = case + '_'
        x = torch.from_numpy(z[pre + 'x'].astype(np.float32))
        up = torch.from_numpy(z[pre + 'up'].astype(np.float32))
        params = {n: torch.from_numpy(z[pre + 'p_' + n].astype(np.float32)) for n in meta['params'][case]}
        want = {mode: {k[len(pre + mode) + 1:]: torch.from_numpy(z[k]) for k in z if k.startswith(pre + mode + '_')}
                for mode in ('eval', 'train')}
        cases[case] = (x, params, up, want)
    return meta, cases
