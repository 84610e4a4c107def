"""The train-mode heads and protonet on the GPU (csrc/conv_train.hip, yolact_amd/layers/train_ops.py, Yolact.forward_heads) against
the oracle of tests/heads_train_ref.py, which tests/test_heads_train_host.py pins to the reference's own train-mode results.

Bar, for every output and every gradient: rel_err(gpu, fp64 oracle) <= max(4 * rel_err(fp32 oracle, fp64 oracle), EXACT_BAR = 8e-6),
the project's bar (tests/test_gpu_multibox.py), printed per quantity.  Against the STORED reference results (fp32 on the CPU) the bar
is that plus 1e-6, the distance tests/test_heads_train_host.py allows between the fp64 oracle and the stored values.  Every case with
a ReLU first asserts on the oracle, per ReLU input, that the smallest |pre-activation| that receives gradient is at least 16 times
the measured fp32-versus-fp64 deviation of that tensor (the rule of tests/test_gpu_maskiou_loss.py); the ReLU behind the upsample inside
the protonet is exempt (its input is a sum of non-negatives).  The seeds below were chosen on the CPU so that this holds.  The
single-layer cases take their inputs from grids on which the pre-activations are exact in fp32 (maps in 1/256, weights in 1/2048):
their deviation is 0 and the margin is the smallest non-zero |pre-activation|.  Nothing is left out of a comparison.

WG_WIDE holds the stride-1 weight gradients of the backbone's last stage at their real widths, all wgrad_k<4, 1> (nt = 4): 1x1 2048 -> 512
(gridDim.x = 64), 1x1 512 -> 2048 (gz = 4 full z-blocks) and 3x3 512 -> 512 (gridDim.x = 144), on 18 positions.  Each also shows that it
can fail: against an fp64 oracle that drops one block of 32 output channels of g the GPU result misses the bar, in dw and in db.
"""
import ctypes as C
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heads_train_ref as H  # noqa: E402
import train_helpers  # noqa: E402
from helpers import rel_err, same_bits  # noqa: E402
from train_helpers import DEV, EXACT_BAR, STORED_SLACK, grid_randn  # noqa: E402
import yolact_amd  # noqa: E402
from yolact_amd import _lib as L  # noqa: E402
from yolact_amd.layers import train_ops as TO  # noqa: E402
from yolact_amd.layers.modules import MultiBoxLoss  # noqa: E402

pytestmark = pytest.mark.gpu
SEEDS = dict(real=37, wgrad=3, conv=5, up=7)         # chosen on the CPU: see the module docstring (the golden's is in its meta)
SMALL_PYRAMID = [(5, 5), (3, 3), (2, 2), (1, 1), (1, 1)]
# (kernel, B, H, W, Cin, Cout): a map smaller than a tile with every pixel at a border and Cout < 32; an odd Cout over several column
# tiles and two channel chunks; 1x1; 3 034 positions: several chunks with a ragged last one and the ordered second pass
WG_SHAPES = [(3, 2, 5, 7, 32, 12), (3, 1, 9, 9, 64, 243), (1, 3, 6, 6, 256, 32), (3, 2, 37, 41, 32, 96)]
# The backbone's stride-1 convolutions at the widths of stage 4, on its 3 x 3 map at batch 2 (18 positions: one ragged chunk, every pixel
# at a border).  The heads reach Cout = 1053 only with Cin = 256 (gridDim.x = 72).  conv1: Cin = 2048, gridDim.x = 64 blocks of 32 input
# channels, nt = 4, gz = 1; conv3: Cout = 2048 = 4 full z-blocks of 512 channels with nothing ragged, gridDim.x = 16; conv2: gridDim.x =
# 9 * 16 = 144 (tap, channel block) pairs, the largest gradient of the backbone (9 x 512 x 512).
WG_WIDE = [(1, 2, 3, 3, 2048, 512), (1, 2, 3, 3, 512, 2048), (3, 2, 3, 3, 512, 512)]
WG_SHAPES += WG_WIDE
_MAX = {}
compare = functools.partial(train_helpers.compare, _MAX)


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    print('\ntrain-mode heads: rel_err against the fp64 oracle (bar)')
    for case in _MAX:
        worst = max(_MAX[case].items(), key=lambda kv: kv[1][0] / kv[1][1])
        print('  %-14s largest %.2e   closest to its bar: %s %.2e (%.1e)' % (case, max(e for e, _ in _MAX[case].values()), worst[0],
                                                                          worst[1][0], worst[1][1]))


@pytest.fixture(autouse=True)
def _restore_cfg():
    yield
    yolact_amd.set_cfg('yolact_base_config')


# ---- the weight gradient alone ----------------------------------------------------------------------------------------------------------
def wgrad_gpu(x, gpad, Cout, k):
    """ymi_conv_wgrad_nhwc_f32 on x [B,H,W,Cin], gpad [B,H,W,ldg] -> (dw [Cout,Cin,k,k], db [Cout])."""
    B, Hh, W, Cin = x.shape
    d = L.ConvWgradDesc()
    dw = torch.full((k * k * Cin, Cout), float('nan'), device=DEV)
    db = torch.full((Cout,), float('nan'), device=DEV)
    d.x, d.g, d.dw, d.db = x.data_ptr(), gpad.data_ptr(), dw.data_ptr(), db.data_ptr()
    d.B, d.H, d.W, d.Cin, d.Cout, d.ldg, d.kh, d.kw, d.pad = B, Hh, W, Cin, Cout, gpad.shape[3], k, k, k // 2
    nbytes = L.lib().ymi_workspace_bytes(L.WS_CONV_WGRAD, C.byref(d))
    ws = torch.full((nbytes // 4,), float('nan'), device=DEV)
    d.ws, d.ws_bytes = ws.data_ptr(), nbytes
    L.check(L.lib().ymi_conv_wgrad_nhwc_f32(C.byref(d), L.stream_ptr()), 'wgrad')
    torch.cuda.synchronize()
    return dw.reshape(k, k, Cin, Cout).permute(3, 2, 0, 1).contiguous().cpu(), db.cpu()


@pytest.mark.parametrize('shape', WG_SHAPES, ids=lambda s: '%dx%d_b%d_%dx%d_%dto%d' % (s[0], s[0], s[1], s[2], s[3], s[4], s[5]))
def test_weight_gradient_alone(shape):
    k, B, Hh, W, Cin, Cout = shape
    g = torch.Generator().manual_seed(SEEDS['wgrad'])
    x = torch.randn(B, Hh, W, Cin, generator=g)
    dy = torch.randn(B, Hh, W, Cout, generator=g)
    def oracle(dy, dtype):
        w = torch.zeros(Cout, Cin, k, k, dtype=dtype, requires_grad=True)
        b = torch.zeros(Cout, dtype=dtype, requires_grad=True)
        y = F.conv2d(x.to(dtype).permute(0, 3, 1, 2), w, b, padding=k // 2)
        dw, db = torch.autograd.grad((y * dy.to(dtype).permute(0, 3, 1, 2)).sum(), [w, b])
        return dict(dw=dw, db=db)
    want = {dtype: oracle(dy, dtype) for dtype in (torch.float64, torch.float32)}
    ldg = (Cout + 31) // 32 * 32
    gpad = torch.full((B, Hh, W, ldg), float('nan'))           # the padding channels are never read
    gpad[..., :Cout] = dy
    dw, db = wgrad_gpu(x.to(DEV), gpad.to(DEV), Cout, k)
    name = 'wgrad_%dx%d_%d_%d' % (k, k, Cin, Cout)
    compare(name, dict(dw=dw, db=db), want[torch.float64], want[torch.float32])
    dw2, db2 = wgrad_gpu(x.to(DEV), gpad.to(DEV), Cout, k)
    same_bits(dw, dw2, 'dw')
    same_bits(db, db2, 'db')
    if shape in WG_WIDE:      # the comparison can fail: an oracle that drops one block of 32 output channels of g is not met
        lost = dy.clone()
        lost[..., Cout - 64:Cout - 32] = 0
        off = oracle(lost, torch.float64)
        for q, t in (('dw', dw), ('db', db)):
            e, bar = rel_err(t, off[q]), _MAX[name][q][1]
            print('%s %s against an oracle without the channels %d .. %d of g: rel_err %.3e (bar %.3e)'
                  % (name, q, Cout - 64, Cout - 33, e, bar))
            assert e > bar


# ---- the activation backward alone ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('act', [L.ACT_NONE, L.ACT_RELU, L.ACT_TANH], ids=['none', 'relu', 'tanh'])
def test_act_bwd_writes_exact_zeros_into_the_padding_channels(act):
    """Three outputs side by side in one NaN-filled buffer of stride 64 (5 | 18 | 12 columns, then padding up to 64):
    every real column holds dy * act'(y), every padding column an exact +0.0, and nothing outside [0, cpad) is touched."""
    g_ = torch.Generator().manual_seed(SEEDS['up'])
    npos, widths, ldg = 70, (5, 18, 12), 64
    buf = torch.full((npos, ldg + 3), float('nan'), device=DEV)          # rows of stride 67: three floats past cpad stay NaN
    n0, want = 0, []
    for i, Cc in enumerate(widths):
        y = torch.randn(npos, Cc, generator=g_).clamp(-0.99, 0.99)
        dy = torch.randn(npos, Cc, generator=g_)
        cpad = Cc + (ldg - sum(widths) if i == len(widths) - 1 else 0)
        yd, dyd = y.to(DEV), dy.to(DEV)
        L.check(L.lib().ymi_act_bwd_f32(yd.data_ptr(), dyd.data_ptr(), buf.data_ptr() + 4 * n0, npos, Cc, cpad, Cc, Cc, ldg + 3, act,
                                        L.stream_ptr()), 'ymi_act_bwd_f32')
        want.append({L.ACT_NONE: dy, L.ACT_RELU: dy * (y > 0), L.ACT_TANH: dy * (1 - y * y)}[act].double())
        n0 += Cc
    torch.cuda.synchronize()
    got = buf.cpu()
    assert rel_err(got[:, :sum(widths)], torch.cat(want, 1)) <= EXACT_BAR
    assert (got[:, sum(widths):ldg].view(torch.int32) == 0).all()          # exact +0.0, not NaN, not -0.0
    assert torch.isnan(got[:, ldg:]).all()


# ---- conv2d_act and upsample2x through autograd -----------------------------------------------------------------------------------------
def conv_case(shape, seed):
    k, B, Hh, W, Cin, Cout = shape
    g = torch.Generator().manual_seed(seed)
    x = grid_randn(g, (B, Hh, W, Cin), 256)
    w = grid_randn(g, (Cout, Cin, k, k), 2048, std=(2.0 / (Cin * k * k)) ** 0.5, lim=0.9)
    b = grid_randn(g, (Cout,), 2048, std=0.1, lim=0.9)
    up = torch.randint(-2, 3, (B, Hh, W, Cout), generator=g).float() / 2
    return x, w, b, up


def conv_oracle(x, w, b, up, k, act, dtype):
    leaves = [t.to(dtype).requires_grad_(True) for t in (x, w, b)]
    z = F.conv2d(leaves[0].permute(0, 3, 1, 2), leaves[1], leaves[2], padding=k // 2).permute(0, 2, 3, 1)
    y = {None: z, 'relu': F.relu(z), 'tanh': torch.tanh(z)}[act]
    gr = torch.autograd.grad((y * up.to(dtype)).sum(), leaves)
    return dict(y=y.detach(), dx=gr[0], dw=gr[1], db=gr[2]), z.detach()


@pytest.mark.parametrize('act', ['relu', 'tanh'])
@pytest.mark.parametrize('shape', [WG_SHAPES[0], WG_SHAPES[3]], ids=['5x7_32to12', '37x41_32to96'])
def test_conv2d_act_through_autograd(shape, act):
    k = shape[0]
    x, w, b, up = conv_case(shape, SEEDS['conv'])
    (o64, z64), (o32, z32) = (conv_oracle(x, w, b, up, k, act, dt) for dt in (torch.float64, torch.float32))
    if act == 'relu':
        hit = up != 0
        m = (z64[hit].abs().min().item(), (z32.double() - z64).abs().max().item())
        print('margin (smallest |pre-activation| with gradient, fp32 deviation):', m)
        assert m[0] > 0
        H.assert_margins(m)
    leaves = [t.to(DEV).requires_grad_(True) for t in (x, w, b)]
    y = TO.conv2d_act(leaves[0], leaves[1], leaves[2], k // 2, act)
    assert y.shape == up.shape
    gr = torch.autograd.grad((y * up.to(DEV)).sum(), leaves)
    torch.cuda.synchronize()
    got = dict(y=y.detach().cpu(), dx=gr[0].cpu(), dw=gr[1].cpu(), db=gr[2].cpu())
    compare('conv_%s_%dto%d_%dx%d' % (act, shape[4], shape[5], shape[2], shape[3]), got, o64, o32)


def test_conv2d_act_with_only_the_bias_requiring_grad():
    shape = WG_SHAPES[0]
    x, w, b, up = conv_case(shape, SEEDS['conv'])
    bg = b.to(DEV).requires_grad_(True)
    y = TO.conv2d_act(x.to(DEV), w.to(DEV), bg, 1, None)
    (db,) = torch.autograd.grad((y * up.to(DEV)).sum(), [bg])
    want = up.double().sum((0, 1, 2))
    assert rel_err(db.cpu(), want) <= EXACT_BAR
    # nobody asked for anything: no gradient function at all
    assert not TO.conv2d_act(x.to(DEV), w.to(DEV), b.to(DEV), 1, 'relu').requires_grad


@pytest.mark.parametrize('relu', [False, True])
def test_upsample2x(relu):
    g = torch.Generator().manual_seed(SEEDS['up'])
    x = grid_randn(g, (2, 5, 7, 32), 256)
    up = torch.randn(2, 10, 14, 32, generator=g)
    want, zs = {}, {}
    for dtype in (torch.float64, torch.float32):
        leaf = x.to(dtype).requires_grad_(True)
        z = F.interpolate(leaf.permute(0, 3, 1, 2), scale_factor=2, mode='bilinear', align_corners=False).permute(0, 2, 3, 1)
        y = F.relu(z) if relu else z
        (dx,) = torch.autograd.grad((y * up.to(dtype)).sum(), [leaf])
        want[dtype], zs[dtype] = dict(y=y.detach(), dx=dx), z.detach()
    if relu:      # a map of both signs, unlike the protonet's: the decisions are exact on this grid (weights 1/16 .. 9/16)
        m = (zs[torch.float64][zs[torch.float64] != 0].abs().min().item(), (zs[torch.float32].double() - zs[torch.float64]).abs().max().item())
        print('margin:', m)
        H.assert_margins(m)
    xg = x.to(DEV).requires_grad_(True)
    y = TO.upsample2x(xg, relu)
    assert y.shape == (2, 10, 14, 32)
    (dx,) = torch.autograd.grad((y * up.to(DEV)).sum(), [xg])
    compare('up2x_relu%d' % relu, dict(y=y.detach().cpu(), dx=dx.cpu()), want[torch.float64], want[torch.float32])
    with pytest.raises(RuntimeError, match='shape'):      # YMI_ESHAPE for other ratios
        L.check(L.lib().ymi_bilinear_bwd_nhwc_f32(y.data_ptr(), None, dx.data_ptr(), 2, 5, 7, 32, 15, 21, 0, L.stream_ptr()))


# ---- Yolact.forward_heads ---------------------------------------------------------------------------------------------------------------
def build_net(config, params, golden=False):
    """A Yolact of `config` (with the golden replacements) whose head side holds `params`, head side on the GPU."""
    yolact_amd.set_cfg(config)
    cfg = yolact_amd.config.cfg
    if golden:
        o = H.golden_cfg_overrides()
        cfg.fpn = cfg.fpn.copy({'num_features': o.pop('num_features')})
        cfg.update(o)
    from yolact_amd.yolact import Yolact
    net = Yolact()
    named = dict(net.named_parameters())
    with torch.no_grad():
        for n, p in params.items():
            assert named[n].shape == p.shape, n
            named[n].copy_(p)
    for m in (net.proto_net, net.prediction_layers, net.semantic_seg_conv):
        m.to(DEV)
    return net, [named[n] for n in params], H.spec_of(cfg)


def run_heads(net, plist, outs, ups):
    leaves = [o.to(DEV).requires_grad_(True) for o in outs]
    pred = net.forward_heads(leaves)
    total = sum((pred[k] * ups[k].to(DEV)).sum() for k in H.OUT_NAMES)
    gr = torch.autograd.grad(total, leaves + plist)
    torch.cuda.synchronize()
    got = {k: pred[k].detach().cpu() for k in H.OUT_NAMES}
    got.update({'d_out%d' % i: t.cpu() for i, t in enumerate(gr[:len(leaves)])})
    return got, gr[len(leaves):], pred


def check_heads(name, net, plist, spec, outs, params, ups, stored=None):
    m = H.relu_margins(outs, params, spec, ups)
    print(name, 'tightest ReLU margin: %s %.3e, fp32 deviation %.3e' % H.tightest(m))
    H.assert_margins(m)
    r64, r32 = (H.run_ref(outs, params, spec, ups, dt) for dt in (torch.float64, torch.float32))
    got, gp, pred = run_heads(net, plist, outs, ups)
    got.update({'d_' + n: t.cpu() for n, t in zip(params, gp)})
    keys = [k for k in r64 if not k.startswith('_') and k != 'priors']
    assert sorted(keys) == sorted(got)
    assert torch.equal(pred['priors'].cpu(), r64['priors']) and not pred['priors'].requires_grad
    assert pred['segm'].shape == r64['segm'].shape and pred['proto'].shape == r64['proto'].shape
    compare(name, got, {k: r64[k] for k in keys}, {k: r32[k] for k in keys})
    if stored is not None:
        assert torch.equal(pred['priors'].cpu(), stored['priors'])
        compare(name + '_stored', got, {k: r64[k] for k in keys}, {k: r32[k] for k in keys}, against=stored, slack=STORED_SLACK)
    return got


@pytest.fixture(scope='module')
def golden():
    meta, outs, params, ups, want = H.load_golden()
    net, plist, spec = build_net('yolact_resnet50_config', params, golden=True)
    return dict(net=net, plist=plist, spec=spec, outs=outs, params=params, ups=ups, want=want)


def use_golden_cfg():
    yolact_amd.set_cfg('yolact_resnet50_config')
    cfg = yolact_amd.config.cfg
    o = H.golden_cfg_overrides()
    cfg.fpn = cfg.fpn.copy({'num_features': o.pop('num_features')})
    cfg.update(o)
    cfg.mask_dim, cfg.num_heads = 32, 5
    return cfg


def test_the_golden_case(golden):
    use_golden_cfg()
    G = golden
    assert len(G['plist']) == 20
    check_heads('golden', G['net'], G['plist'], G['spec'], G['outs'], G['params'], G['ups'], stored=G['want'])


@pytest.mark.parametrize('config', ['yolact_base_config', 'yolact_plus_base_config'])
def test_real_channel_counts_on_the_smallest_pyramid(config):
    cfg = yolact_amd.CONFIGS[config].copy()
    spec = H.spec_of(cfg)
    outs, params, ups = H.random_case(SEEDS['real'], spec, 256, SMALL_PYRAMID, 1)
    net, plist, spec = build_net(config, params)
    A = 3 if config == 'yolact_base_config' else 9
    assert params['prediction_layers.0.conf_layer.weight'].shape[0] == A * 81 and params['semantic_seg_conv.weight'].shape[0] == 80
    got = check_heads(config.replace('yolact_', '').replace('_config', ''), net, plist, spec, outs, params, ups)
    assert got['conf'].shape == (1, 40 * A, 81) and got['mask'].shape == (1, 40 * A, 32) and got['proto'].shape == (1, 10, 10, 32)
    with pytest.raises(NotImplementedError):
        net.train()


def test_bit_reproducibility(golden):
    use_golden_cfg()
    G = golden
    a, ga, _ = run_heads(G['net'], G['plist'], G['outs'], G['ups'])
    b, gb, _ = run_heads(G['net'], G['plist'], G['outs'], G['ups'])
    same_bits(a, b)
    for n, x, y in zip(G['params'], ga, gb):
        same_bits(x, y, n)


def test_freshness_and_the_version_check(golden):
    use_golden_cfg()
    G = golden
    net, spec = G['net'], G['spec']
    w = net.proto_net[0].weight
    leaves = [o.to(DEV).requires_grad_(True) for o in G['outs']]
    before = net.forward_heads(leaves)
    try:
        with torch.no_grad():
            w.mul_(2)
        after = net.forward_heads(leaves)
        params2 = dict(G['params'])
        params2['proto_net.0.weight'] = G['params']['proto_net.0.weight'] * 2
        want = H.run_ref(G['outs'], params2, spec, G['ups'], torch.float64)
        assert not torch.equal(after['proto'], before['proto'])
        assert rel_err(after['proto'].detach().cpu(), want['proto']) <= EXACT_BAR
        same_bits(after['loc'].detach(), before['loc'].detach())
        # the graph built before the edit refuses to run backward; the one built after it runs
        with pytest.raises(RuntimeError, match='modified by an inplace operation'):
            before['proto'].sum().backward()
        after['proto'].sum().backward()
        assert w.grad is not None
    finally:
        with torch.no_grad():
            w.copy_(G['params']['proto_net.0.weight'])
        net.zero_grad()


def test_multibox_loss_on_forward_heads_output(golden):
    cfg = use_golden_cfg()
    G = golden
    net, plist, spec = G['net'], G['plist'], G['spec']
    targets = [torch.tensor([[0.10, 0.10, 0.40, 0.40, 2.0], [0.50, 0.30, 0.95, 0.80, 0.0], [0.20, 0.55, 0.45, 0.80, 4.0]]),
               torch.tensor([[0.30, 0.20, 0.80, 0.70, 1.0], [0.05, 0.60, 0.30, 0.85, 3.0]])]
    masks = []
    for t in targets:
        m = torch.zeros(t.size(0), 48, 48)
        for j, (x1, y1, x2, y2) in enumerate((t[:, :4] * 48).round().long().tolist()):
            m[j, y1:y2, x1:x2] = 1
        masks.append(m)
    net.zero_grad()
    leaves = [o.to(DEV).requires_grad_(True) for o in G['outs']]
    pred = net.forward_heads(leaves)
    for k in H.OUT_NAMES:
        pred[k].retain_grad()
    torch.manual_seed(3)
    losses = MultiBoxLoss(cfg.num_classes, 0.5, 0.4, 3)(None, pred, [t.to(DEV) for t in targets], [m.to(DEV) for m in masks], [0, 0])
    assert sorted(losses) == ['B', 'C', 'M', 'S']
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    d_preds = {k: pred[k].grad.detach().cpu() for k in H.OUT_NAMES}
    assert all(bool(d.ne(0).any()) for d in d_preds.values())
    m = H.relu_margins(G['outs'], G['params'], spec, d_preds)
    print('composition, tightest ReLU margin: %s %.3e, fp32 deviation %.3e' % H.tightest(m))
    H.assert_margins(m)
    r64, r32 = (H.run_ref(G['outs'], G['params'], spec, d_preds, dt) for dt in (torch.float64, torch.float32))
    got = {'d_' + n: p.grad.cpu() for n, p in zip(G['params'], plist)}
    got.update({'d_out%d' % i: t.grad.cpu() for i, t in enumerate(leaves)})
    compare('composition', got, {k: r64[k] for k in got}, {k: r32[k] for k in got})
    net.zero_grad()
    with pytest.raises(NotImplementedError):
        net.train()
