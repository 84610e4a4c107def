"""The FPN of Yolact (yolact.py:311-360) in plain torch, written from the semantics, for the variant every shipped config uses:
1x1 laterals, the top-down sum through a size-form bilinear interpolation, 3x3 / pad 1 pred layers followed by a ReLU, and 3x3 /
stride 2 / pad 1 downsample layers without one.  The oracle of tests/test_fpn_train_host.py (pinned there to what the reference's own
FPN class computed: tests/golden/fpn_train.npz, tools/make_golden_fpn_train.py) and of tests/test_gpu_fpn_train.py.

Everything works in the dtype given (fp32 or fp64) on the CPU.  Parameters are a dict under the state-dict names
(fpn.lat_layers.N.weight, fpn.pred_layers.N.weight, fpn.downsample_layers.N.weight and the biases); lat_layers and pred_layers are
stored DEEPEST level first, the maps come finest first.
"""
import numpy as np
import torch
import torch.nn.functional as F

import helpers
from packed_fixture import QBITS  # noqa: F401
from heads_train_ref import (PARAM_GRID, assert_margins, grid, ints_of, pack, pack5, planes_of, rel_err, tightest, unpack,  # noqa: F401
                             unpack5)

GOLDEN_SIZES, GOLDEN_IN, GOLDEN_B, GOLDEN_NF, GOLDEN_DOWN = ((13, 10), (7, 5), (4, 3)), (64, 96, 128), 2, 32, 2


def param_names(n_in, n_down):
    """The state-dict names of the FPN, in module order."""
    names = []
    for kind, n in (('lat_layers', n_in), ('pred_layers', n_in), ('downsample_layers', n_down)):
        for i in range(n):
            names += ['fpn.%s.%d.weight' % (kind, i), 'fpn.%s.%d.bias' % (kind, i)]
    return names


def param_shapes(in_channels, nf, n_down):
    shapes = {}
    for i, c in enumerate(reversed(list(in_channels))):                      # deepest level first
        shapes['fpn.lat_layers.%d.weight' % i], shapes['fpn.lat_layers.%d.bias' % i] = (nf, c, 1, 1), (nf,)
    for kind, n in (('pred_layers', len(in_channels)), ('downsample_layers', n_down)):
        for i in range(n):
            shapes['fpn.%s.%d.weight' % (kind, i)], shapes['fpn.%s.%d.bias' % (kind, i)] = (nf, nf, 3, 3), (nf,)
    return {n: shapes[n] for n in param_names(len(in_channels), n_down)}


def fpn_ref(convouts, params, n_down, keep=None, detach_down=False):
    """convouts: [B,C_j,h_j,w_j], finest first -> the len(convouts) + n_down maps [B,nf,h,w].  keep receives (name, pre-activation,
    activation) of every pred layer.  detach_down=True is a deliberately WRONG variant: the same values, but nothing comes back from the
    downsample layers into the deepest pred layer's map."""
    n = len(convouts)
    sums, x = [None] * n, None
    for i in range(n):                                                       # layer i works on level n - 1 - i
        j = n - 1 - i
        lat = F.conv2d(convouts[j], params['fpn.lat_layers.%d.weight' % i], params['fpn.lat_layers.%d.bias' % i])
        if x is not None:
            lat = F.interpolate(x, size=tuple(lat.shape[2:]), mode='bilinear', align_corners=False) + lat
        sums[j] = x = lat
    out = [None] * n
    for i in range(n):
        j = n - 1 - i
        z = F.conv2d(sums[j], params['fpn.pred_layers.%d.weight' % i], params['fpn.pred_layers.%d.bias' % i], padding=1)
        out[j] = F.relu(z)
        if keep is not None:
            keep.append(('fpn.pred_layers.%d' % i, z, out[j]))
    for i in range(n_down):
        out.append(F.conv2d(out[-1].detach() if (detach_down and i == 0) else out[-1], params['fpn.downsample_layers.%d.weight' % i], params['fpn.downsample_layers.%d.bias' % i],
                            stride=2, padding=1))
    return out


def run_ref(convouts, params, n_down, ups, dtype, keep=None):
    """Forward and the gradients of sum_k <out_k, ups_k> -> dict('out%d' -> map, 'd_c%d' -> d convout, 'd_' + name -> d param)."""
    leaves = [c.detach().to(dtype).requires_grad_(True) for c in convouts]
    names = param_names(len(convouts), n_down)
    P = {n: params[n].detach().to(dtype).requires_grad_(True) for n in names}
    with helpers.oracle_threads():                       # torch's CPU summation order depends on the thread count
        outs = fpn_ref(leaves, P, n_down, keep)
        total = sum((o * u.to(dtype)).sum() for o, u in zip(outs, ups))
        g = torch.autograd.grad(total, leaves + [P[n] for n in names], retain_graph=keep is not None)
    res = {'out%d' % i: o.detach() for i, o in enumerate(outs)}
    res.update({'d_c%d' % i: t for i, t in enumerate(g[:len(leaves)])})
    res.update({'d_' + n: t for n, t in zip(names, g[len(leaves):])})
    res['_total'], res['_outs'] = total, outs
    return res


def relu_margins(convouts, params, n_down, ups):
    """Per pred layer: (name, the smallest |pre-activation| whose activation receives gradient, in fp64; the largest
    fp32-versus-fp64 deviation of that tensor)."""
    res = {}
    with helpers.oracle_threads():
        for dtype in (torch.float64, torch.float32):
            keep = []
            r = run_ref(convouts, params, n_down, ups, dtype, keep)
            ga = torch.autograd.grad(r['_total'], [a for _, _, a in keep], allow_unused=True)
            res[dtype] = [(n, z.detach(), torch.zeros_like(a) if g is None else g) for (n, z, a), g in zip(keep, ga)]
    out = []
    for (n, z64, g), (_, z32, _) in zip(res[torch.float64], res[torch.float32]):
        hit = g != 0
        out.append((n, z64[hit].abs().min().item() if hit.any() else float('inf'), (z32.double() - z64).abs().max().item()))
    return out


def out_sizes(sizes, n_down):
    sizes = [tuple(s) for s in sizes]
    for _ in range(n_down):
        sizes.append(((sizes[-1][0] - 1) // 2 + 1, (sizes[-1][1] - 1) // 2 + 1))
    return sizes


def random_case(seed, in_channels, nf, sizes, B, n_down):
    """(convouts, params, ups) on fp16-exact grids: maps ~ N(0, 1) in 1/256, weights ~ N(0, 2 / fan_in) in 1/2048, biases in 1/2048,
    one upstream gradient per output with values in {-1, -1/2, 0, 1/2, 1}."""
    g = torch.Generator().manual_seed(seed)
    convouts = [grid(torch.randn(B, c, h, w, generator=g).clamp(-4, 4), 256) for c, (h, w) in zip(in_channels, sizes)]
    params = {}
    for n, shp in param_shapes(in_channels, nf, n_down).items():
        if n.endswith('weight'):
            params[n] = grid((torch.randn(*shp, generator=g) * (2.0 / (shp[1] * shp[2] * shp[3])) ** 0.5).clamp(-0.9, 0.9), PARAM_GRID)
        else:
            params[n] = grid((torch.randn(*shp, generator=g) * 0.1).clamp(-0.9, 0.9), PARAM_GRID)
    ups = [torch.randint(-2, 3, (B, nf, h, w), generator=g).float() / 2 for h, w in out_sizes(sizes, n_down)]
    return convouts, params, ups


# ---- the stored reference results ---------------------------------------------------------------------------------------------------
def load_golden():
    """tests/golden/fpn_train.npz -> (meta, convouts [3 fp32 NCHW], params {name: fp32}, ups [5 fp32], want {name: fp64})."""
    meta, z = helpers.load_golden('fpn_train')
    convouts = [torch.from_numpy(z['c%d' % i].astype(np.float32)) for i in range(len(meta['sizes']))]
    params = {n: torch.from_numpy((ints_of(z['p_' + n]).astype(np.float32) / PARAM_GRID).reshape(meta['param_shapes'][n]))
              for n in meta['params']}
    ups = [unpack5(z['up_out%d' % i], meta['shapes']['out%d' % i]) for i in range(len(meta['sizes']) + meta['num_downsample'])]
    want = {k: unpack(z['q_' + k], meta['steps'][k], meta['shapes'][k]) for k in meta['steps']}
    return meta, convouts, params, ups, want
