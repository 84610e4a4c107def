"""The train-mode FPN on the GPU (csrc/conv_train.hip: ymi_bilinear_size_bwd_nhwc_f32 and the stride of ymi_conv_wgrad_nhwc_f32;
yolact_amd/layers/train_ops.py: conv2d_down, upsample_add; Yolact.forward_fpn) against the oracle of tests/fpn_train_ref.py, which
tests/test_fpn_train_host.py pins to the reference's own FPN results.

Bar, for every output and every gradient, every element compared: rel_err(gpu, fp64 oracle) <= max(4 * rel_err(fp32 oracle, fp64
oracle), EXACT_BAR = 8e-6), the bar of tests/test_gpu_heads_train.py, printed per quantity.  Against the STORED reference results the
bar is that plus 1e-6, the distance tests/test_fpn_train_host.py allows between the fp64 oracle and the stored values.  Every case with
a ReLU first asserts on the oracle that the smallest |pre-activation| that receives gradient is at least 16 times the measured
fp32-versus-fp64 deviation of that tensor; the seeds below were chosen on the CPU so that this holds (the golden's is in its meta).  The
single-layer cases take their inputs from grids (maps in 1/256, weights in 1/2048), where the margin is the smallest non-zero
|pre-activation|.  Every case runs twice on the same inputs and must give the same bits.

WG2_WIDE holds the stride-2 weight gradients of the backbone's stage entries at their real widths, which select wgrad_k<4, 2> (nt = 4):
3x3 512 -> 512 and 1x1 1024 -> 2048 (gz = 4), and the two Cout at which the waves of a block differ: 288 (nact = 3, 2, 2, 2) and 520 (a
second z-block of 8 channels: nact = 1, 0, 0, 0).  Each also shows that it can fail: against an fp64 oracle that drops one block of 32
output channels of g the GPU result misses the bar, in dw and in db.
"""
import ctypes as C
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fpn_train_ref as R  # noqa: E402
import heads_train_ref as H  # noqa: E402
import multibox_ref as MR  # noqa: E402
import class_loss_ref as CR  # noqa: E402
import helpers  # noqa: E402
import train_helpers  # noqa: E402
from helpers import rel_err, same_bits  # noqa: E402
from train_helpers import DEV, EXACT_BAR, STORED_SLACK, down, grid_randn, guarded, twice, unguard, zero_insert_gpu  # noqa: E402
import yolact_amd  # noqa: E402
from yolact_amd import _lib as L  # noqa: E402
from yolact_amd import modules as M  # noqa: E402
from yolact_amd.layers import train_ops as TO  # noqa: E402
from yolact_amd.layers.modules import MultiBoxLoss  # noqa: E402

pytestmark = pytest.mark.gpu
SEEDS = dict(up=7, wgrad=3, conv=5, real=2, e2e=4)      # chosen on the CPU: see the module docstring
# (input size, output size): both interpolations of the golden pyramid, one pixel, x2, the identity in one axis and in both
UP_SHAPES = [((4, 3), (7, 5)), ((7, 5), (13, 10)), ((1, 1), (2, 3)), ((5, 7), (10, 14)), ((2, 9), (2, 17)), ((3, 3), (3, 3))]
# (kernel, B, H, W, Cin, Cout) at stride 2: odd extents with every window at a border and Cout < 32; even extents; 1x1; 2 * 19 * 21 =
# 798 positions: several chunks with a ragged last one
WG2_SHAPES = [(3, 2, 5, 7, 32, 12), (3, 1, 8, 6, 64, 40), (1, 2, 7, 9, 64, 32), (3, 2, 37, 41, 32, 96)]
# More than 8 column tiles of 32 output channels: wgrad_k<4, 2> (nt = 4: a wave holds the tiles wave, wave + 4, wave + 8, wave + 12 of its
# block of 512 channels), which the shapes above (nt = 1) and the FPN at 256 features (nt = 2) never launch.  All on a 5 x 4 map (odd H,
# even W; 6 or 12 positions: one ragged chunk).  Stage 3's conv2 (gz = 1, nact = 4 in every wave, gridDim.x = 9 * 16); stage 4's
# projection (gz = 4 full z-blocks: the offset ob = 512 z, gridDim.x = 32); Cout = 288 = 9 tiles (wave 0 holds 3 live tiles, waves 1 .. 3
# hold 2: nact differs per wave); Cout = 520 (gz = 2, the second z-block holds 8 channels: wave 0 has nact = 1 with 24 dead columns,
# waves 1 .. 3 return at nact == 0).  Their g has 32 NaN padding channels behind Cout.
WG2_WIDE = [(3, 2, 5, 4, 512, 512), (1, 2, 5, 4, 1024, 2048), (3, 1, 5, 4, 32, 288), (1, 2, 5, 4, 64, 520)]
WG2_SHAPES += WG2_WIDE
# conv2d_down: the first three, and mixed parity with a padded width: odd H, even W (the last odd column has a masked tap), ldg 64 with
# 24 zero channels that must contribute nothing (SEEDS['conv'] keeps the ReLU margin here too: checked on the CPU)
DOWN_SHAPES = WG2_SHAPES[:3] + [(3, 1, 5, 6, 32, 40)]
REAL_SIZES = [(5, 5), (3, 3), (2, 2)]
_MAX = {}
compare = functools.partial(train_helpers.compare, _MAX)


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    print('\ntrain-mode FPN: rel_err against the fp64 oracle (bar)')
    for case in _MAX:
        worst = max(_MAX[case].items(), key=lambda kv: kv[1][0] / kv[1][1])
        print('  %-22s largest %.2e   closest to its bar: %s %.2e (%.1e)' % (case, max(e for e, _ in _MAX[case].values()), worst[0],
                                                                          worst[1][0], worst[1][1]))


@pytest.fixture(autouse=True)
def _restore_cfg():
    yield
    yolact_amd.set_cfg('yolact_base_config')


# ---- 1. the size-form bilinear backward alone -------------------------------------------------------------------------------------------
def size_bwd_gpu(dy, Hi, Wi):
    """ymi_bilinear_size_bwd_nhwc_f32 into a NaN-filled dx with a NaN guard band behind it: every element written, the band untouched."""
    B, Ho, Wo, Cc = dy.shape
    buf = guarded(B * Hi * Wi * Cc)
    dyd = dy.to(DEV)
    L.check(L.lib().ymi_bilinear_size_bwd_nhwc_f32(dyd.data_ptr(), buf.data_ptr(), B, Hi, Wi, Cc, Ho, Wo, L.stream_ptr()), 'size bwd')
    torch.cuda.synchronize()
    return unguard(buf, (B, Hi, Wi, Cc))


@pytest.mark.parametrize('shape', UP_SHAPES, ids=lambda s: '%dx%d_to_%dx%d' % (s[0] + s[1]))
def test_bilinear_size_backward_alone(shape):
    (Hi, Wi), (Ho, Wo) = shape
    B, Cc = 2, 32
    g = torch.Generator().manual_seed(SEEDS['up'])
    dy = torch.randn(B, Ho, Wo, Cc, generator=g)
    want = {}
    for dtype in (torch.float64, torch.float32):
        leaf = torch.zeros(B, Cc, Hi, Wi, dtype=dtype, requires_grad=True)
        y = F.interpolate(leaf, size=(Ho, Wo), mode='bilinear', align_corners=False)
        (dx,) = torch.autograd.grad((y * dy.to(dtype).permute(0, 3, 1, 2)).sum(), [leaf])
        want[dtype] = dict(dx=dx.permute(0, 2, 3, 1))
    got = twice(lambda: dict(dx=size_bwd_gpu(dy, Hi, Wi)))
    compare('size_bwd_%dx%d_%dx%d' % (Hi, Wi, Ho, Wo), got, want[torch.float64], want[torch.float32])
    if (Hi, Wi) == (Ho, Wo):
        same_bits(got['dx'], dy, 'the identity')


def test_bilinear_size_backward_of_the_identity_keeps_signed_zeros():
    dy = torch.tensor([0.0, -0.0, 1.5, -2.0] * 8).repeat(1, 3, 3, 1)
    same_bits(size_bwd_gpu(dy, 3, 3), dy, 'the identity')


# ---- 2. the stride-2 weight gradient alone ------------------------------------------------------------------------------------------------
def wgrad_gpu(x, gpad, Cout, k, stride):
    """ymi_conv_wgrad_nhwc_f32 on x [B,H,W,Cin], gpad [B,Ho,Wo,ldg] -> dict(dw [Cout,Cin,k,k], db [Cout]); stride None: the field
    stays as the constructor left it (0)."""
    B, Hh, W, Cin = x.shape
    d = L.ConvWgradDesc()
    dw = torch.full((k * k * Cin, Cout), float('nan'), device=DEV)
    db = torch.full((Cout,), float('nan'), device=DEV)
    d.x, d.g, d.dw, d.db = x.data_ptr(), gpad.data_ptr(), dw.data_ptr(), db.data_ptr()
    d.B, d.H, d.W, d.Cin, d.Cout, d.ldg, d.kh, d.kw, d.pad = B, Hh, W, Cin, Cout, gpad.shape[3], k, k, k // 2
    if stride is not None:
        d.stride = stride
    assert d.stride == (stride or 0)
    nbytes = L.lib().ymi_workspace_bytes(L.WS_CONV_WGRAD, C.byref(d))
    assert nbytes > 0
    ws = torch.full((nbytes // 4,), float('nan'), device=DEV)
    d.ws, d.ws_bytes = ws.data_ptr(), nbytes
    L.check(L.lib().ymi_conv_wgrad_nhwc_f32(C.byref(d), L.stream_ptr()), 'wgrad')
    torch.cuda.synchronize()
    return dict(dw=dw.reshape(k, k, Cin, Cout).permute(3, 2, 0, 1).contiguous().cpu(), db=db.cpu())


def wgrad_case(shape, stride):
    k, B, Hh, W, Cin, Cout = shape
    Ho, Wo = (down(Hh), down(W)) if stride == 2 else (Hh, W)
    g = torch.Generator().manual_seed(SEEDS['wgrad'])
    x = torch.randn(B, Hh, W, Cin, generator=g)
    dy = torch.randn(B, Ho, Wo, Cout, generator=g)
    ldg = (Cout + 31) // 32 * 32 + (32 if shape in WG2_WIDE else 0)
    gpad = torch.full((B, Ho, Wo, ldg), float('nan'))           # the padding channels are never read
    gpad[..., :Cout] = dy
    return x, dy, gpad


@pytest.mark.parametrize('shape', WG2_SHAPES, ids=lambda s: '%dx%d_b%d_%dx%d_%dto%d' % (s[0], s[0], s[1], s[2], s[3], s[4], s[5]))
def test_stride_2_weight_gradient_alone(shape):
    k, B, Hh, W, Cin, Cout = shape
    x, dy, gpad = wgrad_case(shape, 2)
    def oracle(dy, dtype):
        w = torch.zeros(Cout, Cin, k, k, dtype=dtype, requires_grad=True)
        b = torch.zeros(Cout, dtype=dtype, requires_grad=True)
        y = F.conv2d(x.to(dtype).permute(0, 3, 1, 2), w, b, stride=2, padding=k // 2)
        assert y.shape[2:] == dy.shape[1:3]
        dw, db = torch.autograd.grad((y * dy.to(dtype).permute(0, 3, 1, 2)).sum(), [w, b])
        return dict(dw=dw, db=db)
    want = {dtype: oracle(dy, dtype) for dtype in (torch.float64, torch.float32)}
    xd, gd = x.to(DEV), gpad.to(DEV)
    assert shape not in WG2_WIDE or (gpad.shape[3] > Cout and bool(torch.isnan(gpad[..., Cout:]).all()))
    got = twice(lambda: wgrad_gpu(xd, gd, Cout, k, 2))
    name = 'wgrad_s2_%dx%d_%d_%d_%dx%d' % (k, k, Cin, Cout, Hh, W)
    compare(name, got, want[torch.float64], want[torch.float32])
    if shape in WG2_WIDE:      # the comparison can fail: an oracle that drops the last full block of 32 output channels of g is not met
        lost = dy.clone()
        lo = (Cout - 32) // 32 * 32
        lost[..., lo:lo + 32] = 0
        off = oracle(lost, torch.float64)
        for q in ('dw', 'db'):
            e, bar = rel_err(got[q], off[q]), _MAX[name][q][1]
            print('%s %s against an oracle without the channels %d .. %d of g: rel_err %.3e (bar %.3e)' % (name, q, lo, lo + 31, e, bar))
            assert e > bar


def test_stride_1_set_explicitly_gives_the_bits_of_the_field_left_zero():
    from test_gpu_heads_train import WG_SHAPES
    assert len(WG_SHAPES) == 7                            # the three real widths too: nt = 4 at stride 1, gz = 4
    for shape in WG_SHAPES:
        x, dy, gpad = wgrad_case(shape, 1)
        xd, gd = x.to(DEV), gpad.to(DEV)
        same_bits(wgrad_gpu(xd, gd, shape[5], shape[0], 1), wgrad_gpu(xd, gd, shape[5], shape[0], None))


# ---- 3. conv2d_down through autograd ----------------------------------------------------------------------------------------------------
def down_case(shape, seed):
    k, B, Hh, W, Cin, Cout = shape
    g = torch.Generator().manual_seed(seed)
    x = grid_randn(g, (B, Hh, W, Cin), 256)
    w = grid_randn(g, (Cout, Cin, k, k), 2048, std=(2.0 / (Cin * k * k)) ** 0.5, lim=0.9)
    b = grid_randn(g, (Cout,), 2048, std=0.1, lim=0.9)
    up = torch.randint(-2, 3, (B, down(Hh), down(W), Cout), generator=g).float() / 2
    return x, w, b, up


def down_oracle(x, w, b, up, k, act, dtype):
    leaves = [t.to(dtype).requires_grad_(True) for t in (x, w, b)]
    z = F.conv2d(leaves[0].permute(0, 3, 1, 2), leaves[1], leaves[2], stride=2, padding=k // 2).permute(0, 2, 3, 1)
    y = {None: z, 'relu': F.relu(z), 'tanh': torch.tanh(z)}[act]
    gr = torch.autograd.grad((y * up.to(dtype)).sum(), leaves)
    return dict(y=y.detach(), dx=gr[0], dw=gr[1], db=gr[2]), z.detach()


@pytest.mark.parametrize('act', [None, 'relu', 'tanh'], ids=['none', 'relu', 'tanh'])
@pytest.mark.parametrize('shape', DOWN_SHAPES, ids=['3x3_5x7_32to12', '3x3_8x6_64to40', '1x1_7x9_64to32', '3x3_5x6_32to40'])
def test_conv2d_down_through_autograd(shape, act):
    k = shape[0]
    x, w, b, up = down_case(shape, SEEDS['conv'])
    (o64, z64), (o32, z32) = (down_oracle(x, w, b, up, k, act, dt) for dt in (torch.float64, torch.float32))
    if act == 'relu':
        hit = (up != 0) & (z64 != 0)
        m = (z64[hit].abs().min().item(), (z32.double() - z64).abs().max().item())
        print('margin (smallest non-zero |pre-activation| with gradient, fp32 deviation):', m)
        H.assert_margins(m)

    def run():
        leaves = [t.to(DEV).requires_grad_(True) for t in (x, w, b)]
        y = TO.conv2d_down(leaves[0], leaves[1], leaves[2], act)
        gr = torch.autograd.grad((y * up.to(DEV)).sum(), leaves)
        torch.cuda.synchronize()
        return dict(y=y.detach().cpu(), dx=gr[0].cpu(), dw=gr[1].cpu(), db=gr[2].cpu())
    got = twice(run)
    compare('down_%s_%dx%d_%dx%d' % (act, k, k, shape[2], shape[3]), got, o64, o32)
    if act != 'tanh':      # exact grids (up in halves, a ReLU mask): dx has the bits of the spread-then-stride-1 route on this g
        g = up if act is None else up * (got['y'] > 0)
        same_bits(got['dx'], zero_insert_gpu(g, w, shape[2], shape[3]), 'the zero-insert route')
    if k == 1:      # the pixels no window reads: an exact +0.0
        unread = torch.ones(shape[2], shape[3], dtype=torch.bool)
        unread[::2, ::2] = False
        assert (got['dx'][:, unread].view(torch.int32) == 0).all() and bool(got['dx'][:, ~unread].ne(0).any())


def test_conv2d_down_launches_only_what_is_asked_for():
    x, w, b, up = down_case(WG2_SHAPES[0], SEEDS['conv'])
    bg = b.to(DEV).requires_grad_(True)
    y = TO.conv2d_down(x.to(DEV), w.to(DEV), bg, None)
    (db,) = torch.autograd.grad((y * up.to(DEV)).sum(), [bg])
    assert rel_err(db.cpu(), up.double().sum((0, 1, 2))) <= EXACT_BAR
    assert not TO.conv2d_down(x.to(DEV), w.to(DEV), b.to(DEV), 'relu').requires_grad
    with pytest.raises(NotImplementedError, match='5 x 5'):
        TO.conv2d_down(x.to(DEV), torch.zeros(8, 32, 5, 5, device=DEV), torch.zeros(8, device=DEV))


# ---- 4. upsample_add ----------------------------------------------------------------------------------------------------------------------
def test_upsample_add():
    g = torch.Generator().manual_seed(SEEDS['up'])
    top, lat = grid_randn(g, (2, 4, 3, 32), 256), grid_randn(g, (2, 7, 5, 32), 256)
    up = torch.randn(2, 7, 5, 32, generator=g)
    want = {}
    for dtype in (torch.float64, torch.float32):
        a, b = top.to(dtype).requires_grad_(True), lat.to(dtype).requires_grad_(True)
        y = F.interpolate(a.permute(0, 3, 1, 2), size=(7, 5), mode='bilinear', align_corners=False).permute(0, 2, 3, 1) + b
        da, db = torch.autograd.grad((y * up.to(dtype)).sum(), [a, b])
        want[dtype] = dict(y=y.detach(), d_top=da, d_lat=db)

    def run():
        a, b = top.to(DEV).requires_grad_(True), lat.to(DEV).requires_grad_(True)
        y = TO.upsample_add(a, b)
        same_bits(b.detach(), lat, 'lat after the forward')
        assert y.data_ptr() != b.data_ptr()
        da, db = torch.autograd.grad((y * up.to(DEV)).sum(), [a, b])
        torch.cuda.synchronize()
        return dict(y=y.detach().cpu(), d_top=da.cpu(), d_lat=db.cpu())
    got = twice(run)
    compare('upsample_add', got, want[torch.float64], want[torch.float32])
    same_bits(got['d_lat'], up, 'd_lat')
    with pytest.raises(NotImplementedError, match='larger'):
        TO.upsample_add(lat.to(DEV), top.to(DEV))


# ---- 5 .. 7. Yolact.forward_fpn ---------------------------------------------------------------------------------------------------------
def build_net(config, fpn_params, in_channels=None, head_params=None, golden=False):
    """A Yolact of `config` (with the golden replacements of the heads' fixture when golden) whose FPN (rebuilt for `in_channels`
    when given) holds `fpn_params` and whose head side holds `head_params`; FPN and head side on the GPU."""
    yolact_amd.set_cfg(config)
    cfg = yolact_amd.config.cfg
    if golden:
        o = H.golden_cfg_overrides()
        cfg.fpn = cfg.fpn.copy({'num_features': o.pop('num_features')})
        cfg.update(o)
    from yolact_amd.yolact import Yolact
    net = Yolact()
    if in_channels is not None:
        net.fpn = M.FPN(list(in_channels), cfg.fpn.num_features, cfg.fpn.num_downsample, cfg.fpn.pad)
    named = dict(net.named_parameters())
    with torch.no_grad():
        for n, p in list(fpn_params.items()) + list((head_params or {}).items()):
            assert named[n].shape == p.shape, n
            named[n].copy_(p)
    for m in (net.fpn, net.proto_net, net.prediction_layers, net.semantic_seg_conv):
        m.to(DEV)
    assert [n for n in named if n.startswith('fpn.')] == list(fpn_params)
    return net, [named[n] for n in fpn_params], cfg


def run_fpn(net, plist, convouts, ups):
    leaves = [c.to(DEV).requires_grad_(True) for c in convouts]
    outs = net.forward_fpn(leaves)
    assert len(outs) == len(net.selected_layers)
    for o in outs:      # a permuted view of NHWC storage: forward_heads' layout change copies nothing
        assert o.permute(0, 2, 3, 1).is_contiguous() and o.permute(0, 2, 3, 1).contiguous().data_ptr() == o.data_ptr()
    total = sum((o * u.to(DEV)).sum() for o, u in zip(outs, ups))
    gr = torch.autograd.grad(total, leaves + plist)
    torch.cuda.synchronize()
    got = {'out%d' % i: o.detach().cpu() for i, o in enumerate(outs)}
    got.update({'d_c%d' % i: t.cpu() for i, t in enumerate(gr[:len(leaves)])})
    got.update({'d_' + n: t.cpu() for n, t in zip(R.param_names(len(convouts), len(outs) - len(convouts)), gr[len(leaves):])})
    return got


def check_fpn(name, net, plist, convouts, params, ups, stored=None):
    n_down = len(net.fpn.downsample_layers)
    m = R.relu_margins(convouts, params, n_down, ups)
    print(name, 'tightest ReLU margin: %s %.3e, fp32 deviation %.3e' % R.tightest(m))
    R.assert_margins(m)
    r64, r32 = (R.run_ref(convouts, params, n_down, ups, dt) for dt in (torch.float64, torch.float32))
    keys = [k for k in r64 if not k.startswith('_')]
    got = twice(lambda: run_fpn(net, plist, convouts, ups))
    assert len(keys) == len(convouts) + n_down + len(convouts) + len(params)
    compare(name, got, {k: r64[k] for k in keys}, {k: r32[k] for k in keys})
    if stored is not None:
        assert sorted(stored) == sorted(keys)
        compare(name + '_stored', got, {k: r64[k] for k in keys}, {k: r32[k] for k in keys}, against=stored, slack=STORED_SLACK)
    return got


def test_forward_fpn_on_the_golden_case():
    meta, convouts, params, ups, want = R.load_golden()
    net, plist, _ = build_net('yolact_resnet50_config', params, in_channels=R.GOLDEN_IN, golden=True)
    assert len(plist) == 16 and len(convouts) == 3
    got = check_fpn('golden', net, plist, convouts, params, ups, stored=want)
    assert [tuple(got['out%d' % i].shape[2:]) for i in range(5)] == [(13, 10), (7, 5), (4, 3), (2, 2), (1, 1)]
    with pytest.raises(NotImplementedError):
        net.train()


@pytest.mark.parametrize('config', ['yolact_base_config', 'yolact_plus_base_config'])
def test_forward_fpn_with_256_features(config):
    in_channels = (512, 1024, 2048)
    convouts, params, ups = R.random_case(SEEDS['real'], in_channels, 256, REAL_SIZES, 1, 2)
    net, plist, cfg = build_net(config, params)
    assert cfg.fpn.num_features == 256 and [l.in_channels for l in net.fpn.lat_layers] == [2048, 1024, 512]
    got = check_fpn(config.replace('yolact_', '').replace('_config', '') + '_256', net, plist, convouts, params, ups)
    assert [tuple(got['out%d' % i].shape) for i in range(5)] == [(1, 256, s, s) for s in (5, 3, 2, 1, 1)]


def composition_oracle(convouts, fpn_params, head_params, spec, targets, masks, dtype, keep=None):
    """fpn_train_ref + heads_train_ref + multibox_ref: the loss terms, their sum's gradients in the convouts and the FPN parameters."""
    names = list(fpn_params)
    leaves = [c.detach().to(dtype).requires_grad_(True) for c in convouts]
    P = {n: fpn_params[n].detach().to(dtype).requires_grad_(True) for n in names}
    HP = {n: p.detach().to(dtype) for n, p in head_params.items()}
    with helpers.oracle_threads():
        outs = R.fpn_ref(leaves, P, 2, keep)
        pred = H.heads_ref(outs, HP, spec, keep)
        torch.manual_seed(3)
        losses, d_pred, ex = MR.multibox_ref({k: v.detach() for k, v in pred.items()}, targets, masks, [0] * len(targets), dtype)
        total = sum((pred[k] * d_pred[k]).sum() for k in MR.NAMES)
        acts = [a for _, _, a in keep] if keep is not None else []
        g = torch.autograd.grad(total, leaves + [P[n] for n in names] + acts, allow_unused=True)
    res = {k: v.view(1) for k, v in losses.items()}
    res.update({'d_c%d' % i: t for i, t in enumerate(g[:len(leaves)])})
    res.update({'d_' + n: t for n, t in zip(names, g[len(leaves):len(leaves) + len(names)])})
    return res, ex, g[len(leaves) + len(names):]


def test_multibox_loss_through_heads_and_fpn():
    """MultiBoxLoss(forward_heads(forward_fpn(convouts))) on the golden-sized config: the loss terms and the gradients in every fpn.*
    parameter and in the convouts.  The heads hold their fixture's parameters; the maps and the FPN parameters are a seeded case
    (4 of the seeds 1 .. 40 keep the 16x margin at every ReLU of the FPN AND of the heads; the first of them is used).  The boxes
    avoid the pixel borders of the 26 x 20 prototypes, where the crop of the mask loss is an fp32-versus-fp64 decision of the oracle.
    At this size no prior of P6 / P7 is matched or mined (they are larger than the image), so the downsample layers' gradients
    are exact zeros in the oracle and on the GPU; tests 5 and 6 are where those layers receive gradient."""
    convouts, fpn_params, _ = R.random_case(SEEDS['e2e'], R.GOLDEN_IN, R.GOLDEN_NF, R.GOLDEN_SIZES, R.GOLDEN_B, R.GOLDEN_DOWN)
    _, _, head_params, _, _ = H.load_golden()
    net, plist, cfg = build_net('yolact_resnet50_config', fpn_params, in_channels=R.GOLDEN_IN, head_params=head_params, golden=True)
    spec = H.spec_of(cfg)
    assert (cfg.bbox_alpha, cfg.mask_alpha, cfg.conf_alpha, cfg.semantic_segmentation_alpha, cfg.masks_to_train) == (1.5, 6.125, 1, 1, 100)
    targets = [torch.tensor([[0.11, 0.13, 0.42, 0.41, 2.0], [0.52, 0.31, 0.93, 0.79, 0.0], [0.21, 0.56, 0.44, 0.81, 4.0],
                             [0.03, 0.03, 0.97, 0.96, 1.0]]),          # (the large one is matched on P5)
               torch.tensor([[0.31, 0.22, 0.79, 0.71, 1.0], [0.06, 0.61, 0.29, 0.84, 3.0]])]
    masks = []
    for t in targets:
        m = torch.zeros(t.size(0), 48, 48)
        for j, (x1, y1, x2, y2) in enumerate((t[:, :4] * 48).round().long().tolist()):
            m[j, y1:y2, x1:x2] = 1
        masks.append(m)

    # the oracle composition, its ReLU margins (the FPN's pred layers and the heads' ReLUs) and the stability of the OHEM cut
    res = {}
    for dtype in (torch.float64, torch.float32):
        keep = []
        r, ex, ga = composition_oracle(convouts, fpn_params, head_params, spec, targets, masks, dtype, keep)
        res[dtype] = (r, ex, [(n, z.detach(), torch.zeros_like(z) if g is None else g) for (n, z, _), g in zip(keep, ga)])
    (r64, ex, k64), (r32, _, k32) = res[torch.float64], res[torch.float32]
    assert min(CR.cut_gaps(ex['key'], ex['n'])) >= 1e-3
    margins = []
    for (n, z64, g), (_, z32, _) in zip(k64, k32):
        hit = g != 0
        margins.append((n, z64[hit].abs().min().item() if hit.any() else float('inf'), (z32.double() - z64).abs().max().item()))
    print('composition, tightest ReLU margin: %s %.3e, fp32 deviation %.3e' % H.tightest(margins))
    H.assert_margins(margins)

    def run():
        net.zero_grad()
        leaves = [c.to(DEV).requires_grad_(True) for c in convouts]
        outs = net.forward_fpn(leaves)
        for o in outs:      # handed to forward_heads as they are: its NHWC tensor is forward_fpn's storage, no copy
            nhwc = o.permute(0, 2, 3, 1)
            assert nhwc.is_contiguous() and nhwc.contiguous().data_ptr() == o.data_ptr()
        pred = net.forward_heads(outs)
        torch.manual_seed(3)
        losses = MultiBoxLoss(cfg.num_classes, 0.5, 0.4, 3)(None, pred, [t.to(DEV) for t in targets], [m.to(DEV) for m in masks], [0, 0])
        assert sorted(losses) == ['B', 'C', 'M', 'S']
        sum(losses.values()).backward()
        torch.cuda.synchronize()
        got = {k: v.detach().cpu().view(1) for k, v in losses.items()}
        got.update({'d_c%d' % i: t.grad.cpu() for i, t in enumerate(leaves)})
        got.update({'d_' + n: p.grad.cpu() for n, p in zip(fpn_params, plist)})
        return got
    got = twice(run)
    assert all(bool(got['d_' + n].ne(0).any()) != ('downsample' in n) for n in fpn_params)
    assert all(bool(got['d_c%d' % i].ne(0).any()) for i in range(3))
    compare('composition', got, r64, r32)
    net.zero_grad()
    with pytest.raises(NotImplementedError):
        net.train()
