"""The train-mode ResNet stages on the GPU (csrc/conv_dgrad.hip: ymi_conv_dgrad_s2_nhwc_f32; csrc/bn_train.hip: ymi_bn_fwd_nhwc_f32,
ymi_bn_bwd_nhwc_f32; yolact_amd/layers/train_ops.py: conv2d_plain, batch_norm_act, bottleneck; Yolact.forward_backbone) against the
oracle of tests/backbone_train_ref.py, which tests/test_backbone_train_host.py pins to the reference's own Bottleneck results.

Bar, for every output and every gradient, every element compared: rel_err(gpu, fp64 oracle) <= max(4 * rel_err(fp32 oracle, fp64
oracle), EXACT_BAR = 8e-6), the bar of tests/test_gpu_fpn_train.py, printed per quantity.  Against the STORED reference results the bar
is that plus 1e-6, the distance tests/test_backbone_train_host.py allows between the fp64 oracle and the stored values.  Every case with
a ReLU first asserts on the oracle that the smallest |pre-activation| that receives gradient is at least 16 times the measured
fp32-versus-fp64 deviation of that tensor; the seeds below were chosen on the CPU so that this holds (the golden's is in its meta).
Every case runs twice on the same inputs and must give the same bits.  Where an entry is called directly its outputs go into NaN-filled
buffers with a NaN guard band behind them.

The real widths.  The whole real backbone's gradients cannot be compared with fp64: among its several hundred thousand ReLU elements
some pre-activation sits inside the fp32 deviation for every seed.  So every distinct piece is pinned on its own, on the smallest map on
which all of its paths still run:
  DG_WIDE      ymi_conv_dgrad_s2_nhwc_f32 at 3x3 512 -> 512 and 1x1 1024 -> 2048 on 5 x 4 (8 and 16 blocks of 64 input channels,
               Cout / 8 = 64 and 256 steps per tap, the masked last odd column), and at Cin = 160: the half block behind full ones
  BN_SHAPES    C = 2048, 1024, 512 at npos = 18 (below one chunk), 40 (a chunk and a ragged one) and 2 (the smallest training takes)
  conv2d_plain 3x3 512 -> 512 and 1x1 2048 -> 512: the stride-1 data gradient on the engine at K = 4608 and 2048
  REAL_SPECS   the seven bottlenecks of ResNet-50 / 101 beside 'entry', planes 64 .. 512, on [2, inplanes, 5, 4]: behind a stride the
               map is 3 x 2, 12 positions for the batch statistics; wgrad_k<4, 1> and wgrad_k<4, 2> with gz up to 4
  the seam     train_net.backbone itself on four one-block stages whose outputs ALL take a gradient of their own: each map's gradient
               is the sum of two consumers', added at the view_as alias; every other compared case has one consumer per map
The stride-2 and stride-1 weight gradients alone at these widths are in tests/test_gpu_fpn_train.py and tests/test_gpu_heads_train.py.
Each wide data-gradient and weight-gradient case also shows that it can fail: against an fp64 oracle that drops one block of 32 output
channels of g the GPU result misses the bar.
"""
import ctypes as C
import functools
import os
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import backbone_train_ref as R  # noqa: E402
import heads_train_ref as H  # noqa: E402
import helpers  # noqa: E402
import train_helpers  # noqa: E402
from helpers import rel_err, same_bits  # noqa: E402
from train_helpers import DEV, EXACT_BAR, STORED_SLACK, down, guarded, nan_padded, twice, unguard, zero_insert_gpu  # noqa: E402
import yolact_amd  # noqa: E402
from yolact_amd import _lib as L  # noqa: E402
from yolact_amd import modules as M  # noqa: E402
from yolact_amd.layers import train_ops as TO  # noqa: E402
from yolact_amd.layers.modules import MultiBoxLoss  # noqa: E402

pytestmark = pytest.mark.gpu
# (kernel, B, H, W, Cin, Cout): odd extents with every window at a border; even extents (the masked last row and column); 1x1 on odd
# and on even extents; 2 * 37 * 41 pixels: many tiles with a ragged last one in every phase
DG_SHAPES = [(3, 2, 5, 7, 32, 32), (3, 1, 8, 6, 64, 96), (1, 2, 7, 9, 64, 32), (1, 1, 8, 6, 32, 64), (3, 2, 37, 41, 96, 32)]
# the widths of the real stages on a 5 x 4 map (odd H, even W: the last odd column has a masked tap, every pixel at a border; 2 or 6
# pixels per phase, so three waves of every block leave at once): stage 3's conv2 (8 channel blocks of 64, Cout / 8 = 64 steps per tap),
# stage 4's projection (16 channel blocks, 256 steps, three phases of exact zeros); Cin = 160 = 2.5 blocks: a half block (one row tile
# live) BEHIND two full ones.  On the exact grids the largest |sum| is 2048 * 32 units of 1/32, below 2^24.
DG_WIDE = [(3, 2, 5, 4, 512, 512), (1, 2, 5, 4, 1024, 2048), (3, 1, 4, 5, 160, 128)]
DG_SHAPES += DG_WIDE
DG_RANDOM = [DG_SHAPES[4]] + DG_WIDE                      # also run on N(0, 1) values against the fp64 oracle, under the bar
BN_SHAPES = [(2, 32), (70, 32), (70, 256), (3034, 64)]
# channel counts past 256 (bn_delta_k / bn_fin_k: 512 blocks of 4 waves; the chunk kernels: several blocks per chunk) at the position
# counts of a 3 x 3 map (18: below one chunk of 32), of a 5 x 4 one (40: a full chunk and a ragged one of 8) and at the smallest npos
# the training mode takes
BN_SHAPES += [(18, 2048), (40, 1024), (2, 512)]
# the ReLU cases' seeds, per (npos, C, training, residual): the first seed of 1 .. 40 with 64 times the deviation as margin, or the widest
# of them (chosen on the CPU, bn_find_seed; the test asserts 16 times)
BN_SEEDS = {(npos, Cc, training, residual): 1 for npos, Cc in BN_SHAPES for training in (True, False) for residual in (False, True)}
BN_SEEDS.update({(70, 32, True, False): 2, (70, 256, True, False): 2, (70, 256, True, True): 2, (3034, 64, True, False): 4,
                 (3034, 64, True, True): 39, (3034, 64, False, True): 3, (18, 2048, True, False): 5, (18, 2048, False, False): 2,
                 (40, 1024, True, False): 5, (40, 1024, True, True): 2, (40, 1024, False, False): 6})
# (inplanes, planes, stride, projection): identity; stride 1 with a projection; stride 2 with a projection; a layers[0]-style entry
BLOCK_SPECS = {'identity': (128, 32, 1, False), 'proj_s1': (64, 32, 1, True), 'proj_s2': (64, 32, 2, True), 'entry': (64, 64, 1, True)}
BLOCK_SEEDS = {(v, bs): 1 for v in BLOCK_SPECS for bs in (False, True)}      # chosen likewise (at least 77 times)
BLOCK_SEEDS.update({('identity', True): 5, ('proj_s1', True): 2, ('proj_s2', True): 2, ('entry', True): 7})
# every other distinct bottleneck of ResNet-50 / 101 at its real width ('entry' above is stage 1's first), on a 2 x 5 x 4 map
REAL_SPECS = {'s1_id': (256, 64, 1, False), 's2_entry': (256, 128, 2, True), 's2_id': (512, 128, 1, False),
              's3_entry': (512, 256, 2, True), 's3_id': (1024, 256, 1, False), 's4_entry': (1024, 512, 2, True),
              's4_id': (2048, 512, 1, False)}
REAL_X = (5, 4)
# per (shape, batch statistics): R.find_seed(xshape, [spec], modes=(batch_stats,), last=40, factor=16) on the CPU
# (the tightest: s4_id with batch statistics, 17 times; the fp32 oracle's largest rel_err over all quantities is 1.1e-6: the bar is
# EXACT_BAR everywhere)
REAL_SEEDS = {(v, bs): 1 for v in REAL_SPECS for bs in (False, True)}
REAL_SEEDS.update({('s1_id', True): 2, ('s2_entry', True): 2, ('s3_id', False): 3, ('s4_id', False): 8, ('s4_id', True): 9})
# the two-consumer seam: four stages of one block each; every stage output feeds the next stage AND takes a gradient of its own
SEAM_SPECS = [(64, 32, 1, True), (128, 32, 2, True), (128, 32, 2, True), (128, 32, 2, True)]
SEAM_X = (2, 64, 9, 7)
SEAM_SEEDS = {False: 1, True: 3}                          # per batch statistics: R.find_seed(SEAM_X, SEAM_SPECS, (mode,), ups=seam_ups())
_MAX = {}
compare = functools.partial(train_helpers.compare, _MAX)


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    print('\ntrain-mode backbone: rel_err against the fp64 oracle (bar)')
    for case in _MAX:
        worst = max(_MAX[case].items(), key=lambda kv: kv[1][0] / kv[1][1])
        print('  %-28s largest %.2e   closest to its bar: %s %.2e (%.1e)' % (case, max(e for e, _ in _MAX[case].values()), worst[0],
                                                                          worst[1][0], worst[1][1]))


@pytest.fixture(autouse=True)
def _restore_cfg():
    yield
    yolact_amd.set_cfg('yolact_base_config')


# ---- 1. the stride-2 data gradient alone --------------------------------------------------------------------------------------------------
def dgrad_gpu(gpad, w, Hh, W):
    """ymi_conv_dgrad_s2_nhwc_f32 on gpad [B,Ho,Wo,ldg] (device) and the weight [Cout,Cin,k,k] -> dx [B,H,W,Cin] on the CPU."""
    Cout, Cin, k, _ = w.shape
    B = gpad.shape[0]
    wpk = TO._pack_dgrad_s2(w.to(DEV), Cout)
    assert tuple(wpk.shape) == (k, k, Cout // 4, Cin, 4)
    buf = guarded(B * Hh * W * Cin)
    d = L.ConvDgradDesc()
    d.g, d.w, d.dx = gpad.data_ptr(), wpk.data_ptr(), buf.data_ptr()
    d.B, d.H, d.W, d.Cin, d.Cout, d.ldg, d.kh, d.kw, d.pad, d.stride = B, Hh, W, Cin, Cout, gpad.shape[3], k, k, k // 2, 2
    L.check(L.lib().ymi_conv_dgrad_s2_nhwc_f32(C.byref(d), L.stream_ptr()), 'dgrad s2')
    torch.cuda.synchronize()
    return unguard(buf, (B, Hh, W, Cin))


def dgrad_oracle(g, w, Hh, W, dtype):
    B, Cin, k = g.shape[0], w.shape[1], w.shape[2]
    leaf = torch.zeros(B, Cin, Hh, W, dtype=dtype, requires_grad=True)
    y = F.conv2d(leaf, w.to(dtype), None, stride=2, padding=k // 2)
    assert y.shape[2:] == g.shape[1:3]
    (dx,) = torch.autograd.grad((y * g.to(dtype).permute(0, 3, 1, 2)).sum(), [leaf])
    return dx.permute(0, 2, 3, 1)


@pytest.mark.parametrize('shape', DG_SHAPES, ids=lambda s: '%dx%d_b%d_%dx%d_%dto%d' % (s[0], s[0], s[1], s[2], s[3], s[4], s[5]))
def test_stride_2_data_gradient_alone(shape):
    k, B, Hh, W, Cin, Cout = shape
    gen = torch.Generator().manual_seed(11)
    # exact grids: g in 1/4, w in 1/8, every partial sum a small multiple of 1/32: any summation order gives the same fp32 bits
    g = torch.randint(-8, 9, (B, down(Hh), down(W), Cout), generator=gen).float() / 4
    w = torch.randint(-4, 5, (Cout, Cin, k, k), generator=gen).float() / 8
    want = dgrad_oracle(g, w, Hh, W, torch.float64)
    gd = nan_padded(g)
    got = twice(lambda: dict(dx=dgrad_gpu(gd, w, Hh, W)))['dx']
    assert got.shape == want.shape and rel_err(got, want) == 0.0
    assert bool(got.ne(0).any())
    same_bits(got, zero_insert_gpu(g, w, Hh, W), 'the zero-insert route')
    if k == 1:      # the pixels no window reads: an exact +0.0
        unread = torch.ones(Hh, W, dtype=torch.bool)
        unread[::2, ::2] = False
        assert (got[:, unread].view(torch.int32) == 0).all() and bool(got[:, ~unread].ne(0).any())
    if shape in DG_RANDOM:
        g = torch.randn(B, down(Hh), down(W), Cout, generator=gen)
        w = torch.randn(Cout, Cin, k, k, generator=gen) * (2.0 / (Cout * k * k)) ** 0.5
        gd = nan_padded(g)
        got = twice(lambda: dict(dx=dgrad_gpu(gd, w, Hh, W)))
        name = 'dgrad_s2_random_%dx%d' % (Hh, W) + ('_%d_%d' % (Cin, Cout) if shape in DG_WIDE else '')
        want = dict(dx=dgrad_oracle(g, w, Hh, W, torch.float64))
        compare(name, got, want, dict(dx=dgrad_oracle(g, w, Hh, W, torch.float32)))
        if shape in DG_WIDE:      # the comparison can fail: an oracle that drops one block of 32 output channels of g is not met
            lost = g.clone()
            lost[..., Cout - 64:Cout - 32] = 0
            e, bar = rel_err(got['dx'], dgrad_oracle(lost, w, Hh, W, torch.float64)), _MAX[name]['dx'][1]
            print('%s against an oracle without the channels %d .. %d of g: rel_err %.3e (bar %.3e)' % (name, Cout - 64, Cout - 33, e, bar))
            assert e > bar


# ---- 2. the BatchNorm kernels alone -------------------------------------------------------------------------------------------------------
def bn_case(seed, npos, Cc, residual, offset=None):
    gen = torch.Generator().manual_seed(seed)
    if offset is None:
        x = H.grid(torch.randn(npos, Cc, generator=gen).clamp(-4, 4), 256)
    else:
        x = offset + 0.01 * torch.randn(npos, Cc, generator=gen)
    p = dict(gamma=H.grid(0.5 + torch.rand(Cc, generator=gen), 1024), beta=H.grid(torch.randn(Cc, generator=gen) * 0.1, 2048),
             rmean=H.grid((torch.randn(Cc, generator=gen) * 0.25).clamp(-0.9, 0.9), 2048) + (0.0 if offset is None else offset),
             rvar=H.grid(0.5 + torch.rand(Cc, generator=gen), 1024))
    res = H.grid(torch.randn(npos, Cc, generator=gen).clamp(-4, 4), 256) if residual else None
    up = torch.randint(-2, 3, (npos, Cc), generator=gen).float() / 2
    return x, p, res, up


def bn_oracle(x, p, res, up, training, relu, dtype):
    """-> (results, pre-activation)."""
    leaves = [t.to(dtype).requires_grad_(True) for t in (x, p['gamma'], p['beta'])]
    rl = None if res is None else res.to(dtype).requires_grad_(True)
    with helpers.oracle_threads():                       # torch's CPU summation order depends on the thread count
        y, nm, nv, mean, invstd = R.bn_ref(leaves[0], leaves[1], leaves[2], p['rmean'].to(dtype), p['rvar'].to(dtype), training)
        z = y if rl is None else y + rl
        out = F.relu(z) if relu else z
        gr = torch.autograd.grad((out * up.to(dtype)).sum(), leaves + ([] if rl is None else [rl]))
    r = dict(y=out.detach(), mean=mean.detach(), invstd=invstd.detach(), new_rmean=nm.detach(), new_rvar=nv.detach(),
             dx=gr[0], dgamma=gr[1], dbeta=gr[2])
    if rl is not None:
        r['d_res'] = gr[3]
    return r, z.detach()


def bn_margin(x, p, res, up, training):
    (_, z64), (_, z32) = (bn_oracle(x, p, res, up, training, True, dt) for dt in (torch.float64, torch.float32))
    hit = up != 0
    return z64[hit].abs().min().item(), (z32.double() - z64).abs().max().item()


def bn_find_seed(npos, Cc, training, residual, last=40, factor=48):
    """The search that chose BN_SEEDS: well above the margin the test asserts, so that another host's fp32 oracle keeps it too."""
    for seed in range(1, last + 1):
        x, p, res, up = bn_case(seed, npos, Cc, residual)
        lo, dev = bn_margin(x, p, res, up, training)
        if lo >= factor * dev:
            return seed
    raise AssertionError('no seed keeps the margin')


def bn_gpu(x, p, res, up, training, relu):
    """Both entries, called directly -> dict of CPU tensors."""
    npos, Cc = x.shape
    lib, s = L.lib(), L.stream_ptr()
    dev = lambda t: t.to(DEV).contiguous()
    xd, gd, bd, ud = dev(x), dev(p['gamma']), dev(p['beta']), dev(up)
    rm, rv = dev(p['rmean']).clone(), dev(p['rvar']).clone()
    rd = None if res is None else dev(res)
    y, mean, invstd = guarded(npos * Cc), guarded(Cc), guarded(Cc)
    d = L.BnDesc()
    d.x, d.res, d.gamma, d.beta = xd.data_ptr(), (None if rd is None else rd.data_ptr()), gd.data_ptr(), bd.data_ptr()
    d.running_mean, d.running_var, d.y, d.mean, d.invstd = rm.data_ptr(), rv.data_ptr(), y.data_ptr(), mean.data_ptr(), invstd.data_ptr()
    d.npos, d.C, d.training, d.relu, d.eps, d.momentum = npos, Cc, int(training), int(relu), R.EPS, R.MOMENTUM
    nbytes = lib.ymi_workspace_bytes(L.WS_BN, C.byref(d))
    assert nbytes > 0
    ws = torch.full((nbytes // 4,), float('nan'), device=DEV)
    d.ws, d.ws_bytes = ws.data_ptr(), nbytes
    L.check(lib.ymi_bn_fwd_nhwc_f32(C.byref(d), s), 'bn fwd')
    dx, dres, dg, db = guarded(npos * Cc), guarded(npos * Cc), guarded(Cc), guarded(Cc)
    d.dy, d.dx, d.dgamma, d.dbeta = ud.data_ptr(), dx.data_ptr(), dg.data_ptr(), db.data_ptr()
    d.d_res = None if res is None else dres.data_ptr()
    ws.fill_(float('nan'))
    L.check(lib.ymi_bn_bwd_nhwc_f32(C.byref(d), s), 'bn bwd')
    torch.cuda.synchronize()
    out = dict(y=unguard(y, (npos, Cc)), mean=unguard(mean, (Cc,)), invstd=unguard(invstd, (Cc,)), new_rmean=rm.cpu(), new_rvar=rv.cpu(),
               dx=unguard(dx, (npos, Cc)), dgamma=unguard(dg, (Cc,)), dbeta=unguard(db, (Cc,)))
    if res is not None:
        out['d_res'] = unguard(dres, (npos, Cc))
    else:
        assert torch.isnan(dres).all()
    return out


@pytest.mark.parametrize('training', [True, False], ids=['batch_stats', 'frozen'])
@pytest.mark.parametrize('shape', BN_SHAPES, ids=lambda s: '%dx%d' % s)
def test_batchnorm_kernels_alone(shape, training):
    npos, Cc = shape
    for residual in (False, True):
        for relu in (False, True):
            seed = BN_SEEDS[(npos, Cc, training, residual)] if relu else 1
            x, p, res, up = bn_case(seed, npos, Cc, residual)
            if relu:
                m = bn_margin(x, p, res, up, training)
                print('margin (smallest |pre-activation| with gradient, fp32 deviation):', m)
                H.assert_margins(m)
            (o64, _), (o32, _) = (bn_oracle(x, p, res, up, training, relu, dt) for dt in (torch.float64, torch.float32))
            got = twice(lambda: bn_gpu(x, p, res, up, training, relu))
            compare('bn_%dx%d_%s%s%s' % (npos, Cc, 'stats' if training else 'frozen', '_res' if residual else '', '_relu' if relu else ''),
                    got, o64, o32)
            if not training:
                same_bits(got['new_rmean'], p['rmean'], 'frozen: nothing is updated')
                same_bits(got['new_rvar'], p['rvar'], 'frozen: nothing is updated')
                same_bits(got['mean'], p['rmean'])
            if residual and not relu:
                same_bits(got['d_res'], up, 'd_res without a ReLU is dy')


def test_batchnorm_variance_comes_from_deviations():
    """x = 100 + 0.01 randn: E[x^2] - E[x]^2 in fp32 cancels to nothing here (1e4 against 1e-4); deviations about the mean do not."""
    npos, Cc = 3034, 32
    x, p, res, up = bn_case(5, npos, Cc, False, offset=100.0)
    (o64, _), (o32, _) = (bn_oracle(x, p, None, up, True, False, dt) for dt in (torch.float64, torch.float32))
    one_pass = 1 / torch.sqrt(((x * x).mean(0) - x.mean(0) ** 2).clamp_min(0) + R.EPS)
    bar = max(4 * rel_err(o32['invstd'], o64['invstd']), EXACT_BAR)
    print('one-pass fp32 invstd: rel_err %.3e (bar %.3e)' % (rel_err(one_pass, o64['invstd']), bar))
    assert rel_err(one_pass, o64['invstd']) > bar
    got = twice(lambda: bn_gpu(x, p, None, up, True, False))
    compare('bn_offset_100', got, o64, o32)


# ---- 3. conv2d_plain, batch_norm_act and bottleneck through autograd ----------------------------------------------------------------------
# the last two: stage 4's conv2 and conv1 (in stage 4's identity blocks) at their real widths: the stride-1 data gradient on the inference
# engine with K = 9 * 512 = 4608 and K = 2048, the weight gradient with gridDim.x = 144 and 64
@pytest.mark.parametrize('geo', [(3, 1, 32, 40), (1, 1, 64, 32), (3, 2, 32, 32), (1, 2, 64, 96), (3, 2, 64, 40), (3, 1, 512, 512),
                                 (1, 1, 2048, 512)],
                         ids=lambda g: '%dx%d_s%d_%dto%d' % (g[0], g[0], g[1], g[2], g[3]))
def test_conv2d_plain_through_autograd(geo):
    k, stride, Cin, Cout = geo
    gen = torch.Generator().manual_seed(5)
    B, Hh, W = 2, 9, 7
    x = H.grid(torch.randn(B, Hh, W, Cin, generator=gen).clamp(-4, 4), 256)
    w = H.grid((torch.randn(Cout, Cin, k, k, generator=gen) * (2.0 / (Cin * k * k)) ** 0.5).clamp(-0.9, 0.9), 2048)
    Ho, Wo = (down(Hh), down(W)) if stride == 2 else (Hh, W)
    up = torch.randint(-2, 3, (B, Ho, Wo, Cout), generator=gen).float() / 2
    want = {}
    for dtype in (torch.float64, torch.float32):
        leaves = [t.to(dtype).requires_grad_(True) for t in (x, w)]
        y = R.conv_plain_ref(leaves[0].permute(0, 3, 1, 2), leaves[1], stride).permute(0, 2, 3, 1)
        gr = torch.autograd.grad((y * up.to(dtype)).sum(), leaves)
        want[dtype] = dict(y=y.detach(), dx=gr[0], dw=gr[1])

    def run():
        leaves = [t.to(DEV).requires_grad_(True) for t in (x, w)]
        y = TO.conv2d_plain(leaves[0], leaves[1], stride)
        gr = torch.autograd.grad((y * up.to(DEV)).sum(), leaves)
        torch.cuda.synchronize()
        return dict(y=y.detach().cpu(), dx=gr[0].cpu(), dw=gr[1].cpu())
    compare('plain_%dx%d_s%d_%d_%d' % (k, k, stride, Cin, Cout), twice(run), want[torch.float64], want[torch.float32])
    with pytest.raises(NotImplementedError, match='bias = None'):
        TO.conv2d_act(x.to(DEV), w.to(DEV), None, k // 2)


def make_blocks(specs, params, blocks):
    """modules.Bottleneck containers on the GPU holding `params` (names prefixed as backbone_train_ref.random_case prefixes them)."""
    mods = []
    for (inplanes, planes, stride, projection), (prefix, _) in zip(specs, blocks):
        ds = nn.Sequential(nn.Conv2d(inplanes, 4 * planes, 1, stride=stride, bias=False), nn.BatchNorm2d(4 * planes)) if projection else None
        blk = M.Bottleneck(inplanes, planes, stride, ds)
        sd = blk.state_dict()
        with torch.no_grad():
            for n in sd:
                if 'num_batches' not in n:
                    assert sd[n].shape == params[prefix + n].shape, n
                    sd[n].copy_(params[prefix + n])
        mods.append(blk.to(DEV).eval())
    return mods


def restore_stats(mods, params, blocks):
    with torch.no_grad():
        for blk, (prefix, _) in zip(mods, blocks):
            for n, t in blk.state_dict().items():
                if 'running' in n:
                    t.copy_(params[prefix + n])


def run_blocks(mods, params, blocks, x, up, batch_stats):
    """The chain of TO.bottleneck calls -> y, d_x, the gradient of every parameter, the running statistics afterwards."""
    restore_stats(mods, params, blocks)
    leaf = x.permute(0, 2, 3, 1).contiguous().to(DEV).requires_grad_(True)
    out = leaf
    for blk in mods:
        out = TO.bottleneck(out, blk, batch_stats)
    names, plist = [], []
    for blk, (prefix, _) in zip(mods, blocks):
        for n, p in blk.named_parameters():
            names.append(prefix + n)
            plist.append(p)
    gr = torch.autograd.grad((out * up.permute(0, 2, 3, 1).to(DEV)).sum(), [leaf] + plist)
    torch.cuda.synchronize()
    got = {'y': out.detach().permute(0, 3, 1, 2).cpu(), 'd_x': gr[0].permute(0, 3, 1, 2).cpu()}
    got.update({'d_' + n: t.cpu() for n, t in zip(names, gr[1:])})
    for blk, (prefix, _) in zip(mods, blocks):
        for n, t in blk.state_dict().items():
            if 'running' in n:
                got['new_' + prefix + n] = t.detach().cpu().clone()
    return got


def check_blocks(name, specs, x, params, blocks, up, batch_stats, stored=None):
    m = R.relu_margins(x, params, blocks, up, batch_stats)
    print(name, 'tightest ReLU margin: %s %.3e, fp32 deviation %.3e' % R.tightest(m))
    R.assert_margins(m)
    r64, r32 = (R.run_ref(x, params, blocks, up, batch_stats, dt) for dt in (torch.float64, torch.float32))
    keys = [k for k in r64 if not k.startswith('_')]
    mods = make_blocks(specs, params, blocks)
    before = [int(b.bn1.num_batches_tracked) for b in mods]
    got = twice(lambda: run_blocks(mods, params, blocks, x, up, batch_stats))
    assert [int(b.bn1.num_batches_tracked) for b in mods] == [n + (2 if batch_stats else 0) for n in before]
    compare(name, got, {k: r64[k] for k in keys}, {k: r32[k] for k in keys})
    if not batch_stats:
        for n in params:
            if 'running' in n:
                same_bits(got['new_' + n], params[n], n)
    if stored is not None:
        sk = sorted(stored)
        assert set(sk) <= set(keys)
        compare(name + '_stored', {k: got[k] for k in sk}, {k: r64[k] for k in sk}, {k: r32[k] for k in sk}, against=stored,
                slack=STORED_SLACK)
    return mods, got


@pytest.mark.parametrize('batch_stats', [False, True], ids=['frozen', 'batch_stats'])
@pytest.mark.parametrize('variant', list(BLOCK_SPECS))
def test_bottleneck_through_autograd(variant, batch_stats):
    spec = BLOCK_SPECS[variant]
    xshape = (2, spec[0], 9, 7)
    x, params, blocks, up = R.random_case(BLOCK_SEEDS[(variant, batch_stats)], xshape, [spec])
    check_blocks('%s_%s' % (variant, 'stats' if batch_stats else 'frozen'), [spec], x, params, blocks, up, batch_stats)


@pytest.mark.parametrize('batch_stats', [False, True], ids=['frozen', 'batch_stats'])
@pytest.mark.parametrize('variant', list(REAL_SPECS))
def test_bottleneck_at_the_real_widths(variant, batch_stats):
    """Every distinct bottleneck of ResNet-50 / 101 the toy widths leave out, on x [2, inplanes, 5, 4]: odd H and even W (the stride-2
    blocks meet the masked last column), every pixel at a border, and behind the stride a 3 x 2 map: 12 positions for the batch
    statistics, below one BatchNorm chunk.  Output, d_x, every parameter gradient and the new running statistics."""
    spec = REAL_SPECS[variant]
    xshape = (2, spec[0]) + REAL_X
    x, params, blocks, up = R.random_case(REAL_SEEDS[(variant, batch_stats)], xshape, [spec])
    check_blocks('%s_%s' % (variant, 'stats' if batch_stats else 'frozen'), [spec], x, params, blocks, up, batch_stats)


def seam_ups():
    """One upstream gradient per stage output of the seam case, in {-1, -1/2, 0, 1/2, 1}: the same for every seed."""
    gen = torch.Generator().manual_seed(6)
    return [torch.randint(-2, 3, R.out_shape(SEAM_X, SEAM_SPECS[:i + 1]), generator=gen).float() / 2 for i in range(len(SEAM_SPECS))]


class _Stages:
    """What train_net.backbone reads of a Yolact: .backbone.layers, a ModuleList (the stages) of ModuleLists of Bottlenecks."""

    def __init__(self, mods):
        self.backbone = nn.Module()
        self.backbone.layers = nn.ModuleList(nn.ModuleList([m]) for m in mods)


def run_seam(mods, params, blocks, x, ups, batch_stats, through_backbone):
    """sum_i <stage output i, ups[i]> through train_net.backbone (the view_as alias per stage and its node order) or through the
    hand-composed chain of TO.bottleneck calls -> the stage outputs, d_x and the gradient of every parameter."""
    from yolact_amd import train_net as TN
    restore_stats(mods, params, blocks)
    leaf = x.permute(0, 2, 3, 1).contiguous().to(DEV).requires_grad_(True)
    if through_backbone:
        outs = [o.permute(0, 3, 1, 2) for o in TN.backbone(_Stages(mods), leaf, batch_stats)]      # as Yolact.forward_backbone does
    else:
        # as manual() of test_forward_backbone_on_the_real_model: the view of a stage's output is made before the next stage runs, so
        # that what arrives through it is added to the map's gradient last, behind the next stage's conv1 and shortcut (three addends:
        # their order decides the bits)
        h, outs = leaf, []
        for blk in mods:
            h = TO.bottleneck(h, blk, batch_stats)
            outs.append(h.permute(0, 3, 1, 2))
    assert len(outs) == len(mods)
    names, plist = [], []
    for blk, (prefix, _) in zip(mods, blocks):
        for n, p in blk.named_parameters():
            names.append(prefix + n)
            plist.append(p)
    total = sum((o * u.to(DEV)).sum() for o, u in zip(outs, ups))
    gr = torch.autograd.grad(total, [leaf] + plist)
    torch.cuda.synchronize()
    got = {'out%d' % i: o.detach().cpu() for i, o in enumerate(outs)}
    got['d_x'] = gr[0].permute(0, 3, 1, 2).cpu()
    got.update({'d_' + n: t.cpu() for n, t in zip(names, gr[1:])})
    return got


@pytest.mark.parametrize('batch_stats', [False, True], ids=['frozen', 'batch_stats'])
def test_every_stage_output_has_two_consumers(batch_stats):
    """train_net.backbone on four stages of one block each (reduced planes, where the ReLU margins hold), with a gradient arriving at
    EVERY stage output as well as through the next stage: autograd adds the two at the view_as alias.  A backward that wrote into its
    incoming gradient, or reused it, would be wrong only here, where that buffer has a second reader.  Against the fp64 oracle (the four
    outputs, d_x, every parameter gradient), the bits of the hand-composed chain, and each extra consumer shown to contribute."""
    x, params, blocks, _ = R.random_case(SEAM_SEEDS[batch_stats], SEAM_X, SEAM_SPECS)
    ups = seam_ups()
    name = 'seam_%s' % ('stats' if batch_stats else 'frozen')
    m = R.relu_margins(x, params, blocks, None, batch_stats, ups)
    print(name, 'tightest ReLU margin: %s %.3e, fp32 deviation %.3e' % R.tightest(m))
    assert len(m) == 12 and all(lo < float('inf') for _, lo, _ in m)
    R.assert_margins(m)
    r64, r32 = (R.run_ref(x, params, blocks, None, batch_stats, dt, ups=ups) for dt in (torch.float64, torch.float32))
    keys = [k for k in r64 if not k.startswith('_') and not k.startswith('new_')]
    assert len(keys) == 4 + 1 + 4 * 12
    mods = make_blocks(SEAM_SPECS, params, blocks)
    got = twice(lambda: run_seam(mods, params, blocks, x, ups, batch_stats, True))
    assert [tuple(got['out%d' % i].shape) for i in range(4)] == [(2, 128, 9, 7), (2, 128, 5, 4), (2, 128, 3, 2), (2, 128, 2, 1)]
    compare(name, got, {k: r64[k] for k in keys}, {k: r32[k] for k in keys})
    same_bits(got, run_seam(mods, params, blocks, x, ups, batch_stats, False))
    for i in range(3):      # without the gradient of its own at stage output i, d_x is another one: the extra consumer counts
        less = [torch.zeros_like(u) if j == i else u for j, u in enumerate(ups)]
        other = run_seam(mods, params, blocks, x, less, batch_stats, True)
        same_bits(other['out%d' % i], got['out%d' % i])
        assert not torch.equal(other['d_x'], got['d_x']), i
        want = R.run_ref(x, params, blocks, None, batch_stats, torch.float64, ups=less)['d_x']
        assert rel_err(got['d_x'], want) > _MAX[name]['d_x'][1], i


def test_needs_input_grad_is_honoured_and_an_edited_parameter_is_refused():
    spec = BLOCK_SPECS['proj_s2']
    x, params, blocks, up = R.random_case(BLOCK_SEEDS[('proj_s2', False)], (2, spec[0], 9, 7), [spec])
    (blk,) = make_blocks([spec], params, blocks)
    full = run_blocks([blk], params, blocks, x, up, False)
    for m in blk.modules():                              # the reference's freeze_bn(): the affine parameters take no gradient
        if isinstance(m, nn.BatchNorm2d):
            m.weight.requires_grad_(False)
            m.bias.requires_grad_(False)
    leaf = x.permute(0, 2, 3, 1).contiguous().to(DEV).requires_grad_(True)
    y = TO.bottleneck(leaf, blk, False)
    (y * up.permute(0, 2, 3, 1).to(DEV)).sum().backward()
    for n, p in blk.named_parameters():
        if p.requires_grad:
            same_bits(p.grad, full['d_' + n], n)
        else:
            assert p.grad is None, n
    same_bits(leaf.grad.permute(0, 3, 1, 2), full['d_x'])
    # batch_norm_act on its own: no gradient asked for -> none recorded
    bn = blk.bn1
    assert not TO.batch_norm_act(torch.zeros(2, 3, 3, 32, device=DEV), bn, False).requires_grad
    # a backward after an in-place edit of a parameter or of the input is refused by autograd's version check
    for victim in ('conv2', 'bn3', 'x'):
        leaf = x.permute(0, 2, 3, 1).contiguous().to(DEV).requires_grad_(True)
        src = leaf * 1.0
        blk.bn3.weight.requires_grad_(True)
        y = TO.bottleneck(src, blk, False)
        with torch.no_grad():
            {'conv2': blk.conv2.weight, 'bn3': blk.bn3.weight, 'x': src}[victim].mul_(1.0)
        with pytest.raises(RuntimeError, match='modified by an inplace operation'):
            y.sum().backward()
    # the running statistics are edited in place by the kernel, and autograd's version counters say so
    before = (bn.running_mean._version, bn.running_var._version, int(bn.num_batches_tracked))
    TO.batch_norm_act(torch.zeros(2, 3, 3, 32, device=DEV), bn, False)
    assert (bn.running_mean._version, bn.running_var._version, int(bn.num_batches_tracked)) == before
    TO.batch_norm_act(torch.ones(2, 3, 3, 32, device=DEV), bn, True)
    assert bn.running_mean._version > before[0] and bn.running_var._version > before[1] and int(bn.num_batches_tracked) == before[2] + 1


# ---- 4. the golden blocks -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', [('eval', False), ('train', True)], ids=['eval', 'train'])
def test_bottlenecks_on_the_golden_case(mode):
    name, batch_stats = mode
    meta, x, params, blocks, up, want = R.load_golden()
    mods, got = check_blocks('golden_' + name, [tuple(s) for s in meta['specs']], x, params, blocks, up, batch_stats, stored=want[name])
    assert tuple(got['y'].shape) == (2, 128, 5, 4)
    assert len(want[name]) == (2 + 21 + 14 if batch_stats else 2 + 21)


# ---- 5. Yolact.forward_backbone -----------------------------------------------------------------------------------------------------------
def seeded_backbone(config, seed=1):
    """A Yolact of `config` whose backbone stages hold seeded values (weights ~ N(0, 2 / fan_in), non-trivial BatchNorm)."""
    yolact_amd.set_cfg(config)
    from yolact_amd.yolact import Yolact
    torch.manual_seed(seed)
    net = Yolact()
    gen = torch.Generator().manual_seed(seed)
    params, blocks = {}, []
    with torch.no_grad():
        for si, layer in enumerate(net.backbone.layers):
            for bi, blk in enumerate(layer):
                prefix = 'layers.%d.%d.' % (si, bi)
                vals = R.random_block_params(gen, blk.conv1.in_channels, blk.conv1.out_channels, blk.downsample is not None, prefix)
                sd = blk.state_dict()
                for n in sd:
                    if 'num_batches' not in n:
                        sd[n].copy_(vals[prefix + n])
                params.update(vals)
                blocks.append((prefix, blk.stride))
    net.backbone.to(DEV)
    return net, params, blocks


def backbone_params(net):
    return [(n, p) for n, p in net.backbone.layers.named_parameters()]


def restore_backbone(net, params):
    with torch.no_grad():
        for n, t in net.backbone.state_dict().items():
            if 'running' in n and n in params:
                t.copy_(params[n])


@pytest.mark.parametrize('config', ['yolact_base_config', 'yolact_resnet50_config'])
def test_forward_backbone_on_the_real_model(config):
    net, params, blocks = seeded_backbone(config)
    depth = [len(l) for l in net.backbone.layers]
    assert depth == ([3, 4, 23, 3] if config == 'yolact_base_config' else [3, 4, 6, 3])
    gen = torch.Generator().manual_seed(2)
    x = H.grid(torch.randn(2, 64, 9, 9, generator=gen).clamp(-4, 4), 256)
    ends = [sum(depth[:i + 1]) - 1 for i in range(4)]
    ups = [torch.randint(-2, 3, (2, c, s, s), generator=gen).float() / 2 for c, s in zip((256, 512, 1024, 2048), (9, 5, 3, 2))]
    named = backbone_params(net)
    for batch_stats in (False, True):
        want = {}
        for dtype in (torch.float64, torch.float32):
            with torch.no_grad(), helpers.oracle_threads():
                outs = R.chain_ref(x.to(dtype), {n: p.to(dtype) for n, p in params.items()}, blocks, batch_stats)
            want[dtype] = {'out%d' % i: outs[e] for i, e in enumerate(ends)}

        def run():
            restore_backbone(net, params)
            net.zero_grad()
            leaf = x.to(DEV).requires_grad_(True)
            outs = net.forward_backbone(leaf, batch_stats)
            assert len(outs) == 4
            for o in outs:      # a permuted view of NHWC storage: forward_fpn's layout change copies nothing
                nhwc = o.permute(0, 2, 3, 1)
                assert nhwc.is_contiguous() and nhwc.contiguous().data_ptr() == o.data_ptr()
            sum((o * u.to(DEV)).sum() for o, u in zip(outs, ups)).backward()
            torch.cuda.synchronize()
            got = {'out%d' % i: o.detach().cpu() for i, o in enumerate(outs)}
            grads = {'d_x': leaf.grad.cpu()}
            grads.update({'d_' + n: p.grad.cpu() for n, p in named})
            return got, grads

        def manual():
            restore_backbone(net, params)
            net.zero_grad()
            leaf = x.to(DEV).requires_grad_(True)
            h, outs = leaf.permute(0, 2, 3, 1).contiguous(), []
            for layer in net.backbone.layers:
                for blk in layer:
                    h = TO.bottleneck(h, blk, batch_stats)
                outs.append(h.permute(0, 3, 1, 2))
            sum((o * u.to(DEV)).sum() for o, u in zip(outs, ups)).backward()
            torch.cuda.synchronize()
            got = {'out%d' % i: o.detach().cpu() for i, o in enumerate(outs)}
            grads = {'d_x': leaf.grad.cpu()}
            grads.update({'d_' + n: p.grad.cpu() for n, p in named})
            return got, grads
        (got, grads), (got2, grads2) = run(), run()
        same_bits(got, got2)
        same_bits(grads, grads2)
        mgot, mgrads = manual()
        same_bits(got, mgot)
        same_bits(grads, mgrads)
        assert [tuple(got['out%d' % i].shape) for i in range(4)] == [(2, c, s, s) for c, s in zip((256, 512, 1024, 2048), (9, 5, 3, 2))]
        assert len(grads) == 1 + len(named) and all(bool(torch.isfinite(g).all()) for g in grads.values())
        compare('%s_%s' % (config.replace('yolact_', '').replace('_config', ''), 'stats' if batch_stats else 'frozen'), got,
                want[torch.float64], want[torch.float32])
    assert not net.training
    with pytest.raises(NotImplementedError):
        net.train()


def test_forward_backbone_refuses_a_dcn_block_naming_it():
    yolact_amd.set_cfg('yolact_plus_base_config')
    from yolact_amd.yolact import Yolact
    net = Yolact()
    with pytest.raises(NotImplementedError, match=r'backbone\.layers\.\d+\.\d+ is a DCN block'):
        net.forward_backbone(torch.zeros(2, 64, 9, 9, device=DEV))


# ---- 6. end to end ------------------------------------------------------------------------------------------------------------------------
def test_multibox_loss_through_heads_fpn_and_backbone():
    """MultiBoxLoss(forward_heads(forward_fpn(selected(forward_backbone(stem))))) on the golden-sized config of
    tests/test_gpu_fpn_train.py (96 x 96 images: a 24 x 24 stem map, stages of 24, 12, 6 and 3 squared, a pyramid of 12, 6, 3, 2, 1)."""
    net, params, _ = seeded_backbone('yolact_resnet50_config', seed=3)
    cfg = yolact_amd.config.cfg
    o = H.golden_cfg_overrides()
    cfg.fpn = cfg.fpn.copy({'num_features': o.pop('num_features')})
    cfg.update(o)
    from yolact_amd.yolact import Yolact
    torch.manual_seed(3)
    head = Yolact()                                    # the FPN and the heads at 32 features, on the seeded backbone
    head.backbone = net.backbone
    net = head
    for m in (net.fpn, net.proto_net, net.prediction_layers, net.semantic_seg_conv):
        m.to(DEV)
    assert cfg.fpn.num_features == 32 and list(cfg.backbone.selected_layers) == [1, 2, 3]
    gen = torch.Generator().manual_seed(4)
    stem = H.grid(torch.randn(2, 64, 24, 24, generator=gen).clamp(-4, 4), 256).abs()      # behind a ReLU and a max-pool
    targets = [torch.tensor([[0.11, 0.13, 0.42, 0.41, 2.0], [0.52, 0.31, 0.93, 0.79, 0.0], [0.21, 0.56, 0.44, 0.81, 4.0],
                             [0.03, 0.03, 0.97, 0.96, 1.0]]),
               torch.tensor([[0.31, 0.22, 0.79, 0.71, 1.0], [0.06, 0.61, 0.29, 0.84, 3.0]])]
    masks = []
    for t in targets:
        m = torch.zeros(t.size(0), 48, 48)
        for j, (x1, y1, x2, y2) in enumerate((t[:, :4] * 48).round().long().tolist()):
            m[j, y1:y2, x1:x2] = 1
        masks.append(m)
    convs = [(n, p) for n, p in net.backbone.layers.named_parameters() if p.dim() == 4]
    assert len(convs) == 3 * 16 + 4

    def run():
        net.zero_grad()
        leaf = stem.to(DEV).requires_grad_(True)
        outs = net.forward_backbone(leaf)
        assert [tuple(t.shape[1:]) for t in outs] == [(256, 24, 24), (512, 12, 12), (1024, 6, 6), (2048, 3, 3)]
        pred = net.forward_heads(net.forward_fpn([outs[i] for i in cfg.backbone.selected_layers]))
        torch.manual_seed(3)
        losses = MultiBoxLoss(cfg.num_classes, 0.5, 0.4, 3)(None, pred, [t.to(DEV) for t in targets], [m.to(DEV) for m in masks], [0, 0])
        assert sorted(losses) == ['B', 'C', 'M', 'S']
        sum(losses.values()).backward()
        torch.cuda.synchronize()
        got = {k: v.detach().cpu().view(1) for k, v in losses.items()}
        got['d_stem'] = leaf.grad.cpu()
        got.update({'d_' + n: p.grad.cpu() for n, p in convs})
        return got
    got = twice(run)
    for k in 'BCMS':
        assert bool(torch.isfinite(got[k]).all()), (k, got[k])
    for n, _ in convs:
        g = got['d_' + n]
        assert bool(torch.isfinite(g).all()) and bool(g.ne(0).any()), n
    assert bool(torch.isfinite(got['d_stem']).all()) and bool(got['d_stem'].ne(0).any())
    for n, t in net.backbone.state_dict().items():      # eval mode: the frozen statistics stayed
        if 'running' in n and n in params:
            same_bits(t, params[n], n)
    assert not net.training
    with pytest.raises(NotImplementedError):
        net.train()
