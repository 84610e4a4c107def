"""The train-mode DarkNet53 backbone on the GPU (csrc/bn_train.hip: ymi_bn_leaky_fwd_nhwc_f32, ymi_bn_leaky_bwd_nhwc_f32;
csrc/darknet_train.hip: ymi_preconv_wgrad_nhwc_f32; yolact_amd/layers/train_ops.py: batch_norm_leaky, preconv, dark_unit, dark_block;
yolact_amd/train_net.py: darknet, forward) against the oracle of tests/darknet_train_ref.py, which tests/test_darknet_train_host.py pins
to the reference's own darknetconvlayer / DarkNetBlock results.

Bars.  Every output and every gradient, every element compared: rel_err(gpu, fp64 oracle) <= max(4 * rel_err(fp32 oracle, fp64 oracle),
EXACT_BAR = 8e-6) (train_helpers.compare), printed per quantity; against the STORED reference results that plus STORED_SLACK.  On exact
grids every summation order gives the same fp32 bits, so rel_err == 0.0.  Every case runs twice on the same inputs and must give the
same bits.  Where an entry is called directly its outputs go into NaN-filled buffers with a NaN guard band behind them.

Kink condition.  Every case with an activation first asserts on the oracle that the smallest |z| that takes gradient is at least 16
times that tensor's fp32-versus-fp64 deviation.  The seeds below were chosen on the CPU (darknet_train_ref.find_bn_seed with factor 48,
find_seed with factor 32: well above what is asserted, so that another host's fp32 oracle keeps it too).  The whole-backbone case keeps
every channel on one side of 0 (darknet_train_ref.one_sided_case says why nothing else can meet the condition there).
"""
import ctypes as C
import functools
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import darknet_train_ref as R  # noqa: E402
import heads_train_ref as H  # noqa: E402
import helpers  # noqa: E402
import train_helpers  # noqa: E402
from helpers import rel_err, same_bits  # noqa: E402
from train_helpers import DEV, GUARD, STORED_SLACK, guarded, nan_padded, twice, unguard  # noqa: E402
import yolact_amd  # noqa: E402
from yolact_amd import _lib as L  # noqa: E402
from yolact_amd import modules as M  # noqa: E402
from yolact_amd import train_net as TN  # noqa: E402
from yolact_amd.layers import train_ops as TO  # noqa: E402

pytestmark = pytest.mark.gpu
# (npos, C): the smallest npos the training mode takes; three chunks with a ragged last one; many channel blocks; 95 chunks; the last
# stage's width on a 3 x 3 map (below one chunk); 512 channels on a 5 x 4 map (a full chunk and one of 8)
BN_SHAPES = [(2, 32), (70, 32), (70, 256), (3034, 64), (18, 1024), (40, 512)]
# per (npos, C, training, residual): R.find_bn_seed(npos, C, residual, (training,), last=60, factor=48) on the CPU
BN_SEEDS = {(npos, Cc, training, residual): 1 for npos, Cc in BN_SHAPES for training in (True, False) for residual in (False, True)}
BN_SEEDS.update({(70, 32, True, False): 2, (70, 32, True, True): 2, (70, 256, True, False): 2, (70, 256, True, True): 2,
                 (3034, 64, True, False): 4, (3034, 64, True, True): 4})
# (B, H, W, Cout): small odd extents; even extents, two channel groups; 3034 positions: 95 chunks with a ragged last one; one pixel
# (every tap but the centre outside); a wide strip, three channel groups
PW_SHAPES = [(2, 5, 7, 32), (1, 8, 6, 64), (2, 37, 41, 32), (1, 1, 1, 32), (1, 3, 70, 96)]
# the autograd cases: name -> (net, input shape, unit shapes); the blocks at DarkNet53's real widths run on a 2 x 5 x 4 map
UNIT_CASES = {'unit_s1': ([('unit', '', 1)], (2, 32, 9, 7), {'': (32, 64, 3)}),
              'unit_s2': ([('unit', '', 2)], (2, 32, 9, 7), {'': (32, 64, 3)}),
              'unit_1x1': ([('unit', '', 1)], (2, 64, 9, 7), {'': (64, 32, 1)}),
              'pre_unit': ([('unit', 'pre.', 1), ('unit', 'next.', 2)], (2, 3, 9, 7), {'pre.': (3, 32, 3), 'next.': (32, 64, 3)})}
BLOCK_WIDTHS = [(64, 32), (128, 64), (256, 128), (512, 256), (1024, 512)]
for _cin, _ch in BLOCK_WIDTHS:
    UNIT_CASES['block_%d_%d' % (_cin, _ch)] = ([('block', '')], (2, _cin, 5, 4), {'conv1.': (_cin, _ch, 1), 'conv2.': (_ch, _cin, 3)})
# per (case, batch statistics): R.find_seed(xshape, net, shapes, modes=(batch_stats,), last=60, factor=32, x_grad=...) on the CPU
CASE_SEEDS = {(c, bs): 1 for c in UNIT_CASES for bs in (False, True)}
CASE_SEEDS.update({('block_256_128', False): 4, ('block_512_256', False): 3, ('block_512_256', True): 4, ('block_1024_512', True): 3})
# the seam: a DarkNetBackbone of one block per stage on a [2,3,33,29] image: stages of 17 x 15, 9 x 8, 5 x 4, 3 x 2, 2 x 1
SEAM_LAYERS, SEAM_X = (1, 1, 1, 1, 1), (2, 3, 33, 29)
# per batch statistics: R.find_seed(SEAM_X, *seam_net(), (mode,), factor=32, x_grad=False, case=R.one_sided_case); one_sided_case says
# why random_case cannot serve a whole backbone (frozen: 1.5e6 times the deviation, batch statistics: 1.9e4 times)
SEAM_SEEDS = {False: 1, True: 1}
_MAX = {}
compare = functools.partial(train_helpers.compare, _MAX)
SENTINEL = -1431655766                                    # 0xAAAAAAAA: what the guard band behind a mask holds


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    print('\ntrain-mode DarkNet: rel_err against the fp64 oracle (bar)')
    for case in _MAX:
        worst = max(_MAX[case].items(), key=lambda kv: kv[1][0] / kv[1][1])
        print('  %-28s largest %.2e   closest to its bar: %s %.2e (%.1e)' % (case, max(e for e, _ in _MAX[case].values()), worst[0],
                                                                          worst[1][0], worst[1][1]))


@pytest.fixture(autouse=True)
def _restore_cfg():
    yield
    yolact_amd.set_cfg('yolact_base_config')


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def image4(x, fill=0.0):
    """[B,3,H,W] -> the NHWC image with a fourth channel of `fill`, on the GPU."""
    return F.pad(x.permute(0, 2, 3, 1), (0, 1), value=fill).contiguous().to(DEV)


# ---- 1. the leaky BatchNorm kernels alone ---------------------------------------------------------------------------------------------------
def mask_bits(mask, n):
    """The first n bits of the mask words (a CPU int32 tensor) -> bool [n]; the bits behind them are 0."""
    words = mask.numpy().view(np.uint32)
    bits = ((words[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1).reshape(-1).astype(bool)
    assert not bits[n:].any()
    return torch.from_numpy(bits[:n].copy())


def bn_leaky_gpu(case, training, bwd_training=None, sums=True, use_mask=True):
    """Both entries, called directly -> dict of CPU tensors (+ 'decisions': the mask's bits, when a mask is written).  bwd_training: the
    mode of the backward when it differs; sums False: dgamma = dbeta = NULL; use_mask False: the backward is given no mask and reads
    the decisions from y (the forward still writes one: with a residual it has to)."""
    x, gamma, beta, rmean, rvar, res, dy = case
    npos, Cc = x.shape
    lib, s = L.lib(), L.stream_ptr()
    dev = lambda t: t.to(DEV).contiguous()
    xd, gd, bd, ud = dev(x), dev(gamma), dev(beta), dev(dy)
    rm, rv = dev(rmean).clone(), dev(rvar).clone()
    rd = None if res is None else dev(res)
    y, mean, invstd = guarded(npos * Cc), guarded(Cc), guarded(Cc)
    nwords = (npos * Cc + 31) // 32
    mask = None if res is None else torch.full((nwords + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    d = L.BnDesc()
    d.x, d.res, d.gamma, d.beta = xd.data_ptr(), (None if rd is None else rd.data_ptr()), gd.data_ptr(), bd.data_ptr()
    d.running_mean, d.running_var, d.y, d.mean, d.invstd = rm.data_ptr(), rv.data_ptr(), y.data_ptr(), mean.data_ptr(), invstd.data_ptr()
    d.npos, d.C, d.training, d.relu, d.eps, d.momentum = npos, Cc, int(training), 0, R.EPS, R.MOMENTUM
    nbytes = lib.ymi_workspace_bytes(L.WS_BN, C.byref(d))
    assert nbytes > 0
    ws = torch.full((nbytes // 4,), float('nan'), device=DEV)
    d.ws, d.ws_bytes = ws.data_ptr(), nbytes
    L.check(lib.ymi_bn_leaky_fwd_nhwc_f32(C.byref(d), None if mask is None else mask.data_ptr(), s), 'bn leaky fwd')
    dx, dg, db = guarded(npos * Cc), guarded(Cc), guarded(Cc)
    d.dy, d.dx = ud.data_ptr(), dx.data_ptr()
    if sums:
        d.dgamma, d.dbeta = dg.data_ptr(), db.data_ptr()
    if bwd_training is not None:
        d.training = int(bwd_training)
    ws.fill_(float('nan'))
    L.check(lib.ymi_bn_leaky_bwd_nhwc_f32(C.byref(d), None if (mask is None or not use_mask) else mask.data_ptr(), s), 'bn leaky bwd')
    torch.cuda.synchronize()
    out = dict(y=unguard(y, (npos, Cc)), mean=unguard(mean, (Cc,)), invstd=unguard(invstd, (Cc,)), new_running_mean=rm.cpu(),
               new_running_var=rv.cpu(), dx=unguard(dx, (npos, Cc)))
    if sums:
        out.update(dgamma=unguard(dg, (Cc,)), dbeta=unguard(db, (Cc,)))
    else:
        assert torch.isnan(dg).all() and torch.isnan(db).all()
    if mask is not None:
        m = mask.cpu()
        assert bool((m[nwords:] == SENTINEL).all())                        # nothing behind the last word
        out['decisions'] = mask_bits(m[:nwords], npos * Cc).view(npos, Cc)
    return out


@pytest.mark.parametrize('training', [True, False], ids=['batch_stats', 'frozen'])
@pytest.mark.parametrize('shape', BN_SHAPES, ids=lambda s: '%dx%d' % s)
def test_leaky_batchnorm_kernels_alone(shape, training):
    npos, Cc = shape
    for residual in (False, True):
        case = R.bn_case(BN_SEEDS[(npos, Cc, training, residual)], npos, Cc, residual)
        m = R.bn_margin(case, training)
        print('margin (smallest |pre-activation| with gradient, fp32 deviation):', m)
        H.assert_margins(m)
        keep = {}
        o64 = R.bn_leaky_ref(*case, training, torch.float64, keep)
        o32 = R.bn_leaky_ref(*case, training, torch.float32)
        got = twice(lambda: bn_leaky_gpu(case, training))
        dec = got.pop('decisions', None)
        compare('leaky_%dx%d_%s%s' % (npos, Cc, 'stats' if training else 'frozen', '_res' if residual else ''), got, o64, o32)
        hit = case[6] != 0
        if residual:       # the mask holds the decision of every element; where gradient flows the margin makes it the oracle's
            assert torch.equal(dec[hit], (keep['z'] > 0)[hit])
        else:
            assert dec is None
            assert torch.equal((got['y'] > 0)[hit], (keep['z'] > 0)[hit])
        if not training:
            same_bits(got['new_running_mean'], case[3], 'frozen: nothing is updated')
            same_bits(got['new_running_var'], case[4], 'frozen: nothing is updated')
            same_bits(got['mean'], case[3])


@pytest.mark.parametrize('shape', [(70, 32), (3034, 64)], ids=lambda s: '%dx%d' % s)
def test_the_slope_decision_is_made_once(shape):
    """x within a few ulps of its channel mean: z = gamma (x - mean) invstd changes sign between neighbouring fp32 values, and any
    second computation of it that rounds differently flips decisions.  res is a tensor of zeros, so the residual path runs and y still
    shows what the forward decided.  The mask must hold exactly that, and the backward's dx must follow it in every element."""
    npos, Cc = shape
    gen = torch.Generator().manual_seed(9)
    x = 1.0 + torch.randint(-3, 4, (npos, Cc), generator=gen).float() * 2.0 ** -23
    assert bool(x.ne(1.0).any()) and float((x - 1.0).abs().max()) <= 3 * 2.0 ** -23
    gamma, beta = H.grid(0.5 + torch.rand(Cc, generator=gen), 1024), torch.zeros(Cc)
    rmean, rvar = torch.zeros(Cc), torch.ones(Cc)
    dy = torch.randint(-2, 3, (npos, Cc), generator=gen).float() / 2 + 0.25          # never 0: every element shows its slope
    case = (x, gamma, beta, rmean, rvar, torch.zeros(npos, Cc), dy)
    # forward with the batch statistics; backward with frozen = 1 and without the sums: dx = gamma invstd gh, nothing else in it
    got = twice(lambda: bn_leaky_gpu(case, True, bwd_training=False, sums=False))
    decided = got['y'] > 0
    n_pos = int(decided.sum())
    print('%d of %d elements took slope 1' % (n_pos, decided.numel()))
    assert 0 < n_pos < decided.numel()
    assert torch.equal(got['decisions'], decided)
    slope = torch.tensor(0.1, dtype=torch.float32)
    gh = torch.where(decided, dy, slope * dy)
    want = (gamma * got['invstd']) * gh
    same_bits(got['dx'], want, 'dx follows the forward\'s decision in every element')
    # without the mask the backward reads the same decisions from y
    same_bits(bn_leaky_gpu(case, True, bwd_training=False, sums=False, use_mask=False)['dx'], want, 'the decision read from y')
    # the knife edge is real: the decision recomputed from the saved fp32 mean differs somewhere or agrees everywhere, and either way
    # the kernel's own is the one dx follows; what is asserted above does not depend on it
    redo = (gamma * ((x - got['mean']) * got['invstd']) + beta) > 0
    print('a recomputation from the rounded mean would flip %d decisions' % int((redo != decided).sum()))


def column_sum(gh):
    """ymi_bn_bwd_nhwc_f32's column sum for npos <= 64 * 32: chunks of 32 positions added in ascending order from +0.0, then the chunk
    partials pairwise as the butterfly meets them; for two chunks that is p0 + p1."""
    gh = gh.numpy()
    assert gh.shape[0] <= 64
    parts = []
    for r0 in range(0, gh.shape[0], 32):
        s = np.zeros(gh.shape[1], dtype=np.float32)
        for r in range(r0, min(r0 + 32, gh.shape[0])):
            s = (s + gh[r]).astype(np.float32)
        parts.append(s)
    return torch.from_numpy(parts[0] if len(parts) == 1 else (parts[0] + parts[1]).astype(np.float32))


@pytest.mark.parametrize('residual', [False, True], ids=['from_y', 'from_mask'])
def test_a_pre_activation_of_zero_takes_the_small_slope(residual):
    """Channels 0 .. 3: gamma = beta = 0; channels 4 .. 7: beta = 0 and x = running_mean (frozen): z == 0 in every element of both,
    and gh is 0.1f * dy bit for bit, as nn.LeakyReLU's backward gives it."""
    npos, Cc = 40, 32
    x, gamma, beta, rmean, rvar, res, dy = R.bn_case(3, npos, Cc, residual)
    dy = dy + 0.25
    gamma[:4], beta[:8] = 0.0, 0.0
    x[:, 4:8] = rmean[4:8]
    case = (x, gamma, beta, rmean, rvar, res, dy)
    got = twice(lambda: bn_leaky_gpu(case, False))
    z = torch.zeros(npos, 8, requires_grad=True)
    (gh_torch,) = torch.autograd.grad((F.leaky_relu(z, 0.1) * dy[:, :8]).sum(), [z])
    gh = torch.tensor(0.1, dtype=torch.float32) * dy[:, :8]
    same_bits(gh_torch, gh, 'PyTorch: 0.1f * dy at z == 0')
    y_want = torch.zeros(npos, 8) if res is None else (torch.zeros(npos, 8) + res[:, :8])
    same_bits(got['y'][:, :8], y_want)
    if residual:
        assert not bool(got['decisions'][:, :8].any()) and bool(got['decisions'][:, 8:].any())
    same_bits(got['dx'][:, :8], (gamma[:8] * got['invstd'][:8]) * gh, 'dx = gamma invstd (0.1f dy)')
    same_bits(got['dbeta'][:8], column_sum(gh), 'dbeta = sum of 0.1f dy in the kernel\'s order')
    assert bool(got['dx'][:, 4:8].ne(0).all()) and not bool(got['dx'][:, :4].ne(0).any())


# ---- 2. the pre-convolution's weight gradient alone ---------------------------------------------------------------------------------------
def pw_gpu(x4, gpad, Cout):
    """ymi_preconv_wgrad_nhwc_f32 on x4 [B,H,W,4] and gpad [B,H,W,ldg] (device) -> dw [Cout,3,3,3] on the CPU."""
    B, Hh, W, _ = x4.shape
    assert tuple(gpad.shape[:3]) == (B, Hh, W)
    buf = guarded(27 * Cout)
    d = L.PreconvWgradDesc()
    d.x, d.g, d.dw = x4.data_ptr(), gpad.data_ptr(), buf.data_ptr()
    d.B, d.H, d.W, d.Cout, d.ldg = B, Hh, W, Cout, gpad.shape[3]
    nbytes = L.lib().ymi_workspace_bytes(L.WS_PRECONV_WGRAD, C.byref(d))
    assert nbytes > 0 and nbytes % 16 == 0
    ws = torch.full((nbytes // 4 + GUARD,), float('nan'), device=DEV)
    d.ws, d.ws_bytes = ws.data_ptr(), nbytes
    L.check(L.lib().ymi_preconv_wgrad_nhwc_f32(C.byref(d), L.stream_ptr()), 'preconv wgrad')
    torch.cuda.synchronize()
    assert torch.isnan(ws[nbytes // 4:]).all() and not torch.isnan(ws[:nbytes // 4]).any()      # the workspace: all of it, no more
    return TO._unpack_dw(unguard(buf, (27, Cout)), 3, 3)


def pw_oracle(x, g, Cout, dtype, drop=None):
    """x [B,3,H,W], g [B,H,W,Cout] -> the weight gradient of F.conv2d(x, w, None, 1, 1) under <y, g>.  drop = (ci, ky, kx): a WRONG
    oracle that loses that tap row."""
    w = torch.zeros(Cout, 3, 3, 3, dtype=dtype, requires_grad=True)
    y = F.conv2d(x.to(dtype), w, None, stride=1, padding=1)
    assert y.shape[2:] == g.shape[1:3]
    with helpers.oracle_threads():
        (dw,) = torch.autograd.grad((y * g.to(dtype).permute(0, 3, 1, 2)).sum(), [w])
    if drop is not None:
        dw = dw.clone()
        dw[:, drop[0], drop[1], drop[2]] = 0
    return dw


@pytest.mark.parametrize('shape', PW_SHAPES, ids=lambda s: 'b%d_%dx%d_to%d' % s)
def test_preconv_weight_gradient_alone(shape):
    B, Hh, W, Cout = shape
    gen = torch.Generator().manual_seed(13)
    # exact grids: x in 1/4, g in 1/8, every product a multiple of 1/32 and every sum below 2^24 of them: any order gives the same bits
    x = torch.randint(-8, 9, (B, 3, Hh, W), generator=gen).float() / 4
    g = torch.randint(-8, 9, (B, Hh, W, Cout), generator=gen).float() / 8
    want = pw_oracle(x, g, Cout, torch.float64)
    x4, gd = image4(x), g.to(DEV)
    got = twice(lambda: dict(dw=pw_gpu(x4, gd, Cout)))['dw']
    assert got.shape == want.shape and rel_err(got, want) == 0.0
    assert bool(got.ne(0).any())
    same_bits(pw_gpu(image4(x, float('nan')), gd, Cout), got, 'NaN in the padding channel of x')
    same_bits(pw_gpu(x4, nan_padded(g), Cout), got, 'ldg = Cout + 32 with NaN in the padding channels')
    g4 = torch.full((B, Hh, W, Cout + 4), float('nan'))
    g4[..., :Cout] = g
    same_bits(pw_gpu(x4, g4.to(DEV), Cout), got, 'ldg = Cout + 4')
    # random values: the order of the sums matters, the bar is compare's
    x = torch.randn(B, 3, Hh, W, generator=gen)
    g = torch.randn(B, Hh, W, Cout, generator=gen)
    x4, gd = image4(x, float('nan')), nan_padded(g)
    name = 'preconv_wgrad_random_b%d_%dx%d_to%d' % shape
    got = twice(lambda: dict(dw=pw_gpu(x4, gd, Cout)))
    compare(name, got, dict(dw=pw_oracle(x, g, Cout, torch.float64)), dict(dw=pw_oracle(x, g, Cout, torch.float32)))
    # the comparison can fail: an oracle that drops one tap row is not met (the centre tap exists at every size)
    e, bar = rel_err(got['dw'], pw_oracle(x, g, Cout, torch.float64, drop=(1, 1, 1))), _MAX[name]['dw'][1]
    print('%s against an oracle without the row (ci 1, ky 1, kx 1): rel_err %.3e (bar %.3e)' % (name, e, bar))
    assert e > bar


# ---- 3. dark_unit, dark_block and preconv through autograd --------------------------------------------------------------------------------
def make_modules(net, shapes, params):
    """One module per step on the GPU, holding `params`: a unit is the Sequential of yolact_amd.modules, a block a DarkNetBlock."""
    mods = []
    for step in net:
        if step[0] == 'unit':
            cin, cout, k = shapes[step[1]]
            m = M._dark_unit(cin, cout, k, stride=step[2], padding=k // 2)
        else:
            cin, ch, _ = shapes[step[1] + 'conv1.']
            m = M.DarkNetBlock(cin, ch)
        sd = m.state_dict()
        with torch.no_grad():
            for n in sd:
                if 'num_batches' not in n:
                    assert sd[n].shape == params[step[1] + n].shape, (step, n)
                    sd[n].copy_(params[step[1] + n])
        mods.append(m.to(DEV).eval())
    return mods


def named(net, mods, what):
    return [(step[1] + n, t) for step, m in zip(net, mods) for n, t in getattr(m, what)()]


def run_net(net, mods, params, x, ups, batch_stats, taps=None, x_grad=True):
    """The train_ops calls of every step -> the tapped outputs (NCHW), every gradient, the running statistics afterwards."""
    taps = [len(net) - 1] if taps is None else taps
    with torch.no_grad():
        for n, t in named(net, mods, 'named_buffers'):
            if 'running' in n:
                t.copy_(params[n])
    pre = x.shape[1] == 3
    leaf = image4(x) if pre else nhwc(x).to(DEV).requires_grad_(bool(x_grad))
    h, outs = leaf, []
    for i, (step, m) in enumerate(zip(net, mods)):
        if step[0] == 'block':
            h = TO.dark_block(h, m, batch_stats)
        elif pre and i == 0:
            h = TO.batch_norm_leaky(TO.preconv(h, m[0].weight), m[1], batch_stats)
        else:
            h = TO.dark_unit(h, m, batch_stats)
        outs.append(h)
    outs = [outs[t] for t in taps]
    ps = named(net, mods, 'named_parameters')
    total = sum((o * nhwc(u).to(DEV)).sum() for o, u in zip(outs, ups))
    gr = torch.autograd.grad(total, ([leaf] if (x_grad and not pre) else []) + [p for _, p in ps])
    torch.cuda.synchronize()
    got = {'y': outs[0].detach().permute(0, 3, 1, 2).cpu()} if len(outs) == 1 else \
        {'out%d' % i: o.detach().permute(0, 3, 1, 2).cpu() for i, o in enumerate(outs)}
    if x_grad and not pre:
        got['d_x'], gr = gr[0].permute(0, 3, 1, 2).cpu(), gr[1:]
    got.update({'d_' + n: t.cpu() for (n, _), t in zip(ps, gr)})
    got.update({'new_' + n: t.detach().cpu().clone() for n, t in named(net, mods, 'named_buffers') if 'running' in n})
    return got


def check_case(name, net, shapes, x, params, ups, batch_stats, taps=None, x_grad=True, stored=None):
    m = R.leaky_margins(x, params, net, ups, batch_stats, taps, x_grad)
    print(name, 'tightest margin (name, smallest, fp32 deviation):', R.tightest(m))
    R.assert_margins(m)
    r64, r32 = (R.run_ref(x, params, net, ups, batch_stats, dt, taps=taps, x_grad=x_grad) for dt in (torch.float64, torch.float32))
    keys = [k for k in r64 if not k.startswith('_')]
    mods = make_modules(net, shapes, params)
    bns = [b for m_ in mods for b in m_.modules() if isinstance(b, nn.BatchNorm2d)]
    got = twice(lambda: run_net(net, mods, params, x, ups, batch_stats, taps, x_grad))
    assert all(int(b.num_batches_tracked) == (2 if batch_stats else 0) for b in bns)
    compare(name, got, {k: r64[k] for k in keys}, {k: r32[k] for k in keys})
    if not batch_stats:
        for n in params:
            if 'running' in n:
                same_bits(got['new_' + n], params[n], n)
    if stored is not None:
        sk = sorted(k for k in stored if k in got)
        assert set(stored) - set(sk) <= {'d_x'}
        compare(name + '_stored', {k: got[k] for k in sk}, {k: r64[k] for k in sk}, {k: r32[k] for k in sk},
                against={k: stored[k] for k in sk}, slack=STORED_SLACK)
    return got, mods


@pytest.mark.parametrize('batch_stats', [False, True], ids=['frozen', 'batch_stats'])
@pytest.mark.parametrize('case', list(UNIT_CASES))
def test_units_and_blocks_through_autograd(case, batch_stats):
    net, xshape, shapes = UNIT_CASES[case]
    x_grad = xshape[1] != 3
    x, params, ups = R.random_case(CASE_SEEDS[(case, batch_stats)], xshape, net, shapes)
    got, _ = check_case('%s_%s' % (case, 'stats' if batch_stats else 'frozen'), net, shapes, x, params, ups, batch_stats, x_grad=x_grad)
    for k, v in got.items():
        assert bool(v.ne(0).any()), k
    assert ('d_x' in got) == x_grad


@pytest.mark.parametrize('mode', [('eval', False), ('train', True)], ids=['eval', 'train'])
@pytest.mark.parametrize('case', list(R.GOLDEN_CASES))
def test_the_golden_cases(case, mode):
    name, batch_stats = mode
    meta, cases = R.load_golden()
    x, params, up, want = cases[case]
    net, xshape, shapes = R.GOLDEN_CASES[case]
    got, _ = check_case('golden_%s_%s' % (case, name), net, shapes, x, params, [up], batch_stats, x_grad=case != 'pre', stored=want[name])
    assert tuple(got['y'].shape) == tuple(want[name]['y'].shape)


def test_needs_input_grad_and_the_version_check():
    net, xshape, shapes = UNIT_CASES['block_64_32']
    x, params, ups = R.random_case(CASE_SEEDS[('block_64_32', True)], xshape, net, shapes)
    mods = make_modules(net, shapes, params)
    blk = mods[0]
    full = run_net(net, mods, params, x, ups, True)
    # a subset: no gradient in x, conv1's BatchNorm frozen in its affine parameters
    for p in blk.conv1[1].parameters():
        p.requires_grad_(False)
    with torch.no_grad():
        for n, t in named(net, mods, 'named_buffers'):
            if 'running' in n:
                t.copy_(params[n])
    leaf = nhwc(x).to(DEV)
    out = TO.dark_block(leaf, blk, True)
    (out * nhwc(ups[0]).to(DEV)).sum().backward()
    torch.cuda.synchronize()
    assert blk.conv1[1].weight.grad is None and blk.conv1[1].bias.grad is None
    for n, p in blk.named_parameters():
        if p.requires_grad:
            same_bits(p.grad.cpu(), full['d_' + n], n)
    same_bits(out.detach().permute(0, 3, 1, 2).cpu(), full['y'])
    # nothing requires grad: nothing is recorded
    for p in blk.parameters():
        p.requires_grad_(False)
    out = TO.dark_block(leaf, blk, False)
    assert not out.requires_grad and out.grad_fn is None
    # only the residual path asks: its gradient is the incoming one
    bn = nn.BatchNorm2d(64).to(DEV).eval()
    for p in bn.parameters():
        p.requires_grad_(False)
    res = torch.randn(2, 5, 4, 64, device=DEV, requires_grad=True)
    dyd = torch.randn(2, 5, 4, 64, device=DEV)
    y = TO.batch_norm_leaky(torch.randn(2, 5, 4, 64, device=DEV), bn, False, residual=res)
    (g,) = torch.autograd.grad((y * dyd).sum(), [res])
    same_bits(g, dyd, 'd_res is dy')
    # a backward after an in-place edit of a parameter is refused by autograd's version check
    for p in blk.parameters():
        p.requires_grad_(True)
    for edit in (blk.conv2[1].weight, blk.conv1[0].weight):
        out = TO.dark_block(leaf, blk, False)
        with torch.no_grad():
            edit.mul_(1.0)
        with pytest.raises(RuntimeError, match='modified by an inplace operation'):
            out.sum().backward()
    w = nn.Parameter(torch.randn(32, 3, 3, 3, device=DEV))
    x4 = image4(torch.randn(2, 3, 9, 7))
    y = TO.preconv(x4, w)
    with torch.no_grad():
        w.mul_(1.0)
    with pytest.raises(RuntimeError, match='modified by an inplace operation'):
        y.sum().backward()
    frozen = nn.Parameter(w.detach().clone(), requires_grad=False)
    y = TO.preconv(x4, frozen)
    assert not y.requires_grad and y.grad_fn is None
    with pytest.raises(NotImplementedError, match='requires grad'):
        TO.preconv(x4.clone().requires_grad_(True), w)


# ---- 4. the seam: train_net.darknet --------------------------------------------------------------------------------------------------------
def seam_net():
    return R.backbone_net(SEAM_LAYERS)


def seam_model(params):
    bb = M.DarkNetBackbone(SEAM_LAYERS)
    sd = bb.state_dict()
    with torch.no_grad():
        for n in params:
            sd[n].copy_(params[n])
    return bb.to(DEV).eval()


def run_seam(bb, params, x, ups, batch_stats, forward):
    """forward(x on the GPU, batch_stats) -> the five stage outputs; -> them (NCHW), every gradient of sum_i <out i, ups[i]>, the
    running statistics afterwards."""
    with torch.no_grad():
        for n, t in bb.named_buffers():
            if 'running' in n:
                t.copy_(params[n])
    outs = forward(x.to(DEV), batch_stats)
    assert len(outs) == 5
    ps = list(bb.named_parameters())
    gr = torch.autograd.grad(sum((o * nhwc(u).to(DEV)).sum() for o, u in zip(outs, ups)), [p for _, p in ps])
    torch.cuda.synchronize()
    got = {'out%d' % i: o.detach().permute(0, 3, 1, 2).cpu() for i, o in enumerate(outs)}
    got.update({'d_' + n: t.cpu() for (n, _), t in zip(ps, gr)})
    got.update({'new_' + n: t.detach().cpu().clone() for n, t in bb.named_buffers() if 'running' in n})
    return got


def by_hand(bb):
    """train_net.darknet's composition written out: the same train_ops calls in the same order, the same alias per stage."""
    def forward(xd, batch_stats):
        h = TO.batch_norm_leaky(TO.preconv(F.pad(xd.permute(0, 2, 3, 1), (0, 1)).contiguous(), bb._preconv[0].weight), bb._preconv[1],
                                batch_stats)
        outs = []
        for layer in bb.layers:
            h = TO.dark_unit(h, layer[0], batch_stats)
            for blk in list(layer)[1:]:
                h = TO.dark_block(h, blk, batch_stats)
            outs.append(h.view_as(h))
        return outs
    return forward


def test_train_net_darknet_on_a_backbone_of_one_block_per_stage():
    """Every stage output feeds the next stage AND takes a gradient of its own.  Against the oracle with the frozen statistics."""
    net, taps, shapes = seam_net()
    x, params, ups = R.one_sided_case(SEAM_SEEDS[False], SEAM_X, net, shapes, taps)
    m = R.leaky_margins(x, params, net, ups, False, taps, False)
    print('seam tightest margin (name, smallest, fp32 deviation):', R.tightest(m))
    R.assert_margins(m)
    r64, r32 = (R.run_ref(x, params, net, ups, False, dt, taps=taps, x_grad=False) for dt in (torch.float64, torch.float32))
    keys = [k for k in r64 if not k.startswith('_')]
    bb = seam_model(params)
    holder = types.SimpleNamespace(backbone=bb)
    got = twice(lambda: run_seam(bb, params, x, ups, False, lambda xd, bs: TN.darknet(holder, xd, bs)))
    assert [tuple(got['out%d' % i].shape[1:]) for i in range(5)] == [(64, 17, 15), (128, 9, 8), (256, 5, 4), (512, 3, 2), (1024, 2, 1)]
    compare('seam_frozen', got, {k: r64[k] for k in keys}, {k: r32[k] for k in keys})
    for n in params:
        if 'running' in n:
            same_bits(got['new_' + n], params[n], n)
    same_bits(got, run_seam(bb, params, x, ups, False, by_hand(bb)), 'the train_ops calls composed by hand')
    # the gradient of an inner stage output matters: without it the first stage's weights get another gradient
    lone = R.run_ref(x, params, net, [torch.zeros_like(u) for u in ups[:-1]] + [ups[-1]], False, torch.float64, taps=taps, x_grad=False)
    assert rel_err(lone['d__preconv.0.weight'], r64['d__preconv.0.weight']) > 1e-3


def test_train_net_darknet_with_batch_statistics():
    """The same backbone with the batch statistics: the same bits twice, the bits of the calls composed by hand, finite values, every
    running statistic moved.  NOT compared with the oracle under the bar: the last stage normalises over 2 x 2 x 1 = 4 positions
    behind 15 other normalisations, and two fp32 evaluations of the ORACLE ITSELF (its convolutions on NCHW and on channels-last
    tensors, BatchNorm by F.batch_norm) differ from each other there by 1 to 3 times the bar at every seed tried, so the bar could not
    tell a right kernel from a wrong one.  Units and blocks are compared with the oracle in this mode in section 3, at every real
    width.  The figures against the oracle are printed."""
    net, taps, shapes = seam_net()
    x, params, ups = R.one_sided_case(SEAM_SEEDS[True], SEAM_X, net, shapes, taps)
    bb = seam_model(params)
    holder = types.SimpleNamespace(backbone=bb)
    got = twice(lambda: run_seam(bb, params, x, ups, True, lambda xd, bs: TN.darknet(holder, xd, bs)))
    same_bits(got, run_seam(bb, params, x, ups, True, by_hand(bb)), 'the train_ops calls composed by hand')
    assert all(int(b.num_batches_tracked) == 3 for b in bb.modules() if isinstance(b, nn.BatchNorm2d))
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()) and bool(v.ne(0).any()), k
    for n in params:
        if 'running' in n:
            assert not torch.equal(got['new_' + n], params[n]), n
    r64, r32 = (R.run_ref(x, params, net, ups, True, dt, taps=taps, x_grad=False) for dt in (torch.float64, torch.float32))
    worst = max(((rel_err(got[k], r64[k]), max(4 * rel_err(r32[k], r64[k]), train_helpers.EXACT_BAR), k) for k in got),
                key=lambda t: t[0] / t[1])
    print('seam with batch statistics, closest to the bar it is not held to: %s rel_err %.3e (bar %.3e)' % (worst[2], worst[0], worst[1]))


# ---- 5. end to end ------------------------------------------------------------------------------------------------------------------------
def test_the_darknet53_config_trains_end_to_end():
    """yolact_darknet53_config shrunk to 96 x 96 images and 32 features: train_net.forward -> MultiBoxLoss -> backward reaches every
    backbone parameter with the same bits twice; Trainer(net, forward=..) takes two steps; Yolact.forward_train keeps refusing."""
    from yolact_amd.layers.modules import MultiBoxLoss
    from yolact_amd.training import Trainer
    from yolact_amd.yolact import Yolact
    yolact_amd.set_cfg('yolact_darknet53_config')
    cfg = yolact_amd.config.cfg
    o = H.golden_cfg_overrides()
    cfg.fpn = cfg.fpn.copy({'num_features': o.pop('num_features')})
    cfg.update(o)
    cfg.update(dict(lr=1e-3, lr_warmup_until=0, lr_steps=(), freeze_bn=False))
    torch.manual_seed(5)
    net = Yolact()
    assert isinstance(net.backbone, M.DarkNetBackbone) and list(cfg.backbone.selected_layers) == [2, 3, 4]
    net.to(DEV)
    gen = torch.Generator().manual_seed(4)
    images = torch.randn(2, 3, 96, 96, generator=gen).to(DEV)
    targets = [torch.tensor([[0.11, 0.13, 0.42, 0.41, 2.0], [0.52, 0.31, 0.93, 0.79, 0.0], [0.21, 0.56, 0.44, 0.81, 4.0],
                             [0.03, 0.03, 0.97, 0.96, 1.0]]),
               torch.tensor([[0.31, 0.22, 0.79, 0.71, 1.0], [0.06, 0.61, 0.29, 0.84, 3.0]])]
    masks = []
    for t in targets:
        m = torch.zeros(t.size(0), 48, 48)
        for j, (x1, y1, x2, y2) in enumerate((t[:, :4] * 48).round().long().tolist()):
            m[j, y1:y2, x1:x2] = 1
        masks.append(m.to(DEV))
    targets = [t.to(DEV) for t in targets]
    state = {k: v.detach().clone() for k, v in net.state_dict().items()}
    crit = MultiBoxLoss(cfg.num_classes, cfg.positive_iou_threshold, cfg.negative_iou_threshold, cfg.ohem_negpos_ratio)
    backbone = [(n, p) for n, p in net.backbone.named_parameters()]
    assert len(backbone) == 3 * (1 + 5 + 2 * 23)

    def run():
        net.load_state_dict(state)
        net.zero_grad()
        cfg._tmp_img_h = cfg._tmp_img_w = None
        torch.manual_seed(3)
        losses = crit(net, TN.forward(net, images, True), targets, masks, [0, 0])
        assert (cfg._tmp_img_h, cfg._tmp_img_w) == (96, 96)
        sum(losses.values()).backward()
        torch.cuda.synchronize()
        got = {k: v.detach().cpu().view(1) for k, v in losses.items()}
        got.update({'d_' + n: p.grad.cpu() for n, p in net.named_parameters() if p.grad is not None})
        return got
    got = twice(run)
    print('losses:', {k: round(float(v), 4) for k, v in got.items() if len(k) == 1})
    assert sorted(k for k in got if len(k) == 1) == ['B', 'C', 'M', 'S'] and all(bool(torch.isfinite(v).all()) for v in got.values())
    for n, _ in backbone:
        g = got['d_backbone.' + n]
        assert bool(torch.isfinite(g).all()) and bool(g.ne(0).any()), n

    net.load_state_dict(state)
    net.zero_grad()
    tr = Trainer(net, forward=lambda x, bs: TN.forward(net, x, bs))
    assert type(tr.criterion) is MultiBoxLoss and tr.batch_stats is True
    for it in range(2):
        torch.manual_seed(100 + it)
        losses = tr.step(images, targets, masks, [0, 0])
    torch.cuda.synchronize()
    assert tr.iteration == 2 and int(tr.optimizer.skipped.item()) == 0 and all(bool(torch.isfinite(v).all()) for v in losses.values())
    last = 'layers.4.%d.conv2.0.weight' % len(net.backbone.layers[4][1:])
    for n in ('_preconv.0.weight', last):
        assert not torch.equal(dict(backbone)[n].detach(), state['backbone.' + n]), n
    # what stays refused, on the same net
    with pytest.raises(NotImplementedError, match='DarkNetBackbone'):
        net.forward_train(images)
    with pytest.raises(NotImplementedError, match='DarkNetBackbone'):
        Trainer(net).step(images, targets, masks, [0, 0])
