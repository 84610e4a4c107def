"""The first launches of every inference, through the C ABI, against tests/entry_ref.py (pinned on the CPU by
tests/test_entry_kat_host.py): the fused stem ymi_stem_pool_f32 (csrc/stem.hip) against the float64 oracle stem_fp64, and
ymi_fast_base_transform_f32 (csrc/preprocess.hip) BIT FOR BIT against its fp32 restatement.

Stem, per case: y is prefilled with NaN between NaN guards; every owned element finite, the guards intact, the error against
stem_fp64 over the WHOLE output relative to max|ref| under the bar, y_amax read as the maximum over its sub-slots equal to max(y)
exactly (and no other float of the slot written), a second launch bit-identical, y_amax = NULL the same y, and against each wrong=
oracle that changes the case (taps transposed, last stem row / column dropped, image b read as b - 1) the bar is MISSED.  Cases
(entry_ref.STEM_CASES): 1x7x7 and 3x7x7 (one tile an image, every pixel at a border); one ragged shape for every pair of remainders
(Hp % 4, Wp % 6), odd and even H, W; Bx3x200x300 with B from the device's CU count so that ntiles >= 3 CUs + 1 (blocks run three and
four tiles of the persistent loop: the prefetch, the cur = nxt hand-over, the reuse of the stem tile); a zero image between two
loud ones and an all-zero 40x40 region inside a loud image (outputs whose receptive field is zero are ReLU(bias) to the bit); a BN
bias of -1000 (the output is +0.0 everywhere: the pool's -inf padding never leaks); the 30x hot patch; the image scaled by 2^-100
and 2^100 with a zero BN bias (each result is the unscaled one times that power of two, bit for bit: the per-tile scale is an exact
power of two from the patch's own exponent).

One bar for the stem, entry_ref.STEM_BAR: <= the earlier 1e-6 and <= 4x the largest error measured on MI355X (printed at the end of
the module):

  measured max|y - ref| / max|ref|, MI355X (256 CUs: B = 5, 845 tiles at 200x300)
    1x7x7 2.58e-7   3x7x7 2.32e-7   15 ragged shapes 2.26e-7 .. 3.85e-7   5x200x300 (persistent loop) 4.46e-7
    zero image 2.73e-7   zero region 2.45e-7   negative bias 0   hot patch 1.61e-7   scale invariance 3.21e-7
    largest 4.46e-7 (4x = 1.8e-6)                                                     STEM_BAR 1e-6 (the earlier bar)
  every wrong= oracle is >= 100 x STEM_BAR away from stem_fp64 on the outputs it concerns (asserted on the host).

FastBaseTransform: modes 0 .. 3 x both output layouts on up-, down-sampling, identity, H = 1 and W = 1 sources with N = 3, and
8x16x16 -> 550x550 (9454 blocks: above the grid cap of 8192), through the C ABI and through FastBaseTransform() / to_nhwc4; every
element compared, the fourth NHWC4 channel +0.0.  Modes 0 and 2 divide: HIP's fp32 division is correctly rounded, so they are held to
equality like modes 1 and 3.

Coverage: every 'input', 'stem', ymi_bilinear_nhwc_f32, ymi_maxpool3x3s2_nhwc_f32 and ymi_bilinear_add_nhwc_f32 op of the batch-1
and batch-8 timed plans, reduced to its form (kernel, channels, explicit or derived scale, relu flag, bound slot or none), is a form
this file or tests/test_gpu_layout_kat.py runs.  Stale bounds: on the r50_dense net a quiet batch gives the same bits on a fresh
net and right after the same batch 2^10 louder, on the native executor and on the Python loop.

The whole file takes 12 s on an MI355X (38 tests): 2.2 s the persistent-loop case (its float64 oracles on the host), 1.0 s the
550x550 FastBaseTransform restatement, 1 - 1.7 s each of the four tests that build a network.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import entry_ref as R

pytestmark = pytest.mark.gpu

from yolact_amd import _lib as L  # noqa: E402

DEV = 'cuda:0'
F = np.float32
GUARD = 64                 # floats of NaN before and after y (256 bytes: y stays 16-byte aligned)
_MAX = {}                  # case -> largest error against stem_fp64
_REF = {}


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    if _MAX:
        print('\nstem KAT, max|y - stem_fp64| / max|stem_fp64| per case (bar %.1e):' % R.STEM_BAR)
        for k, e in _MAX.items():
            print('    %-28s %.2e' % (k, e))
        print('    %-28s %.2e' % ('largest', max(_MAX.values())))


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _bn_module(bn):
    gamma, beta, mean, var = bn
    m = torch.nn.BatchNorm2d(64, eps=R.BN_EPS)
    m.weight.data, m.bias.data = gamma.clone(), beta.clone()
    m.running_mean, m.running_var = mean.clone(), var.clone()
    return m.eval()


class Stem:
    """One packed stem and its launches."""

    def __init__(self, case):
        from yolact_amd.engine import Packed
        self.pk = Packed(case['w'], None, _bn_module(case['bn']), 2, 3, 4, DEV)
        self.planes, self.sc2, _ = self.pk.h2()

    def run(self, x, slot=True):
        """x [B,3,H,W] CPU -> (y [B,Hp,Wp,64] on the device, the whole guarded buffer, the slot or None)."""
        B, _, H, W = x.shape
        Hs, Ws = R.out_size(H, 7, 2, 3), R.out_size(W, 7, 2, 3)
        Hp, Wp = R.out_size(Hs, 3, 2, 1), R.out_size(Ws, 3, 2, 1)
        n = B * Hp * Wp * 64
        buf = torch.full((n + 2 * GUARD,), float('nan'), device=DEV)
        xd = x.to(DEV)
        amax = torch.zeros(L.AMAX_SLOT_FLOATS, device=DEV) if slot else None
        d = L.StemDesc()
        d.x, d.y, d.B, d.H, d.W = xd.data_ptr(), buf.data_ptr() + 4 * GUARD, B, H, W
        d.cout_pad, d.kpad = self.pk.CoutPad, self.pk.Kpad
        d.w_h2, d.scale_h2, d.bias = self.planes.data_ptr(), self.sc2.data_ptr(), self.pk.bias.data_ptr()
        d.y_amax = amax.data_ptr() if slot else None
        L.check(L.lib().ymi_stem_pool_f32(C.byref(d), L.stream_ptr()), 'stem')
        torch.cuda.synchronize()
        return buf[GUARD:GUARD + n].view(B, Hp, Wp, 64), buf, amax


def _guards_intact(buf):
    return bool(torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[-GUARD:]).all())


def _case(name):
    if name not in _REF:
        c = R.stem_case(name, cus=_cus())
        _REF[name] = (c, R.stem_fp64(c['x'], c['w'], c['bn']))
    return _REF[name]


def _err(y, ref):
    return (y.double() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-300)


@pytest.mark.parametrize('name', list(R.STEM_CASES))
def test_stem_case(name):
    c, ref = _case(name)
    x, kind = c['x'], c['kind']
    st = Stem(c)
    yd, buf, amax = st.run(x)
    y = yd.cpu()
    assert tuple(y.shape) == tuple(ref.shape)
    assert bool(torch.isfinite(y).all()), 'an owned element was not written (NaN prefill) or is not finite'
    assert _guards_intact(buf)
    # the bound: the maximum over the 16 sub-slots is max(y) (y >= 0), and only floats [64 k] of the slot were written
    sl = amax.cpu().view(16, 64)
    assert sl[:, 0].max().item() == y.max().item() and (R.bits(sl[:, 1:]) == 0).all()
    assert (sl[:, 0] >= 0).all()
    # a second launch, and one without a bound slot: the same bits
    y2, buf2, _ = st.run(x)
    assert R.same_bits(y2, y) and _guards_intact(buf2)
    y3, buf3, _ = st.run(x, slot=False)
    assert R.same_bits(y3, y) and _guards_intact(buf3)
    if kind == 'negbias':
        assert (R.bits(y) == 0).all(), 'not +0.0 everywhere'
        e = (y.double() - ref).abs().max().item()
    else:
        e = _err(y, ref)
    _MAX[name] = e
    print('%s: B %d, error %.3e of max|ref| (bar %.1e)' % (name, x.shape[0], e, R.STEM_BAR))
    assert e < R.STEM_BAR, e
    for v in R.WRONG:
        if R.wrong_applies(c, v):
            ew = _err(y, R.stem_fp64(x, c['w'], c['bn'], wrong=v))
            assert ew >= R.STEM_BAR, (v, ew)
    if kind in ('zero_image', 'zero_region'):
        bias = st.pk.bias.cpu()
        assert torch.equal(bias, R.folded_bias(c['bn']))
        m = R.zero_field(x)
        assert int(m.sum()) >= 16
        want = torch.relu(bias).view(1, 64).expand(int(m.sum()), 64).contiguous()
        assert R.same_bits(y[m].contiguous(), want), 'an output with an all-zero receptive field is not ReLU(bias)'
    if R.STEM_CASES[name][1] is None:                                 # B chosen from the device's CU count
        ntiles, cus = 169 * x.shape[0], _cus()
        assert 3 * cus + 1 <= ntiles < 4 * cus, (ntiles, cus)          # some blocks run three tiles, some four
    if kind == 'scale':
        yn = y.numpy()
        for e2 in R.SCALE_EXPONENTS:
            ys, bufs, _ = st.run(x * 2.0 ** e2)
            want = yn * F(2.0 ** e2)
            assert want.dtype == F and np.isfinite(want).all()
            assert not ((want != 0) & (np.abs(want) < F(2.0 ** -126))).any()        # (no result left the normal range)
            assert R.same_bits(ys, want), 'x * 2^%d is not y * 2^%d bit for bit' % (e2, e2)
            assert _guards_intact(bufs)


def test_stem_persistent_case_uses_the_device_cu_count():
    c, _ = _case('persistent_200x300')
    assert c['x'].shape[0] == R.persistent_B(_cus())


# ---- FastBaseTransform -------------------------------------------------------------------------------------------------------------

def _fbt_abi(img_d, N, H, W, oh, ow, mode, nhwc4):
    n = N * oh * ow * (4 if nhwc4 else 3)
    buf = torch.full((n + 2 * GUARD,), float('nan'), device=DEV)
    mean, std = (C.c_float * 3)(*R.MEANS), (C.c_float * 3)(*R.STD)
    L.check(L.lib().ymi_fast_base_transform_f32(img_d.data_ptr(), buf.data_ptr() + 4 * GUARD, N, H, W, oh, ow, mean, std, mode,
                                                1 if nhwc4 else 0, L.stream_ptr()), 'fbt')
    torch.cuda.synchronize()
    assert _guards_intact(buf)
    return buf[GUARD:GUARD + n].view((N, oh, ow, 4) if nhwc4 else (N, 3, oh, ow)).cpu().numpy()


@pytest.mark.parametrize('case', R.FBT_CASES, ids=['%dx%dx%d-%dx%d' % c for c in R.FBT_CASES])
def test_fast_base_transform_bit_for_bit(case):
    N, H, W, oh, ow = case
    img = R.fbt_input(case)
    img_d = torch.from_numpy(img).to(DEV)
    if case == R.FBT_CASES[-1]:
        assert N * oh * ow > R.FBT_GRID_CAP                       # the grid-stride path
    for mode in range(4):
        want = R.fast_base_transform(img, oh, ow, mode, False)
        got = _fbt_abi(img_d, N, H, W, oh, ow, mode, False)
        if not R.same_bits(got, want):
            ulp, cnt = R.ulp_distance(got, want)
            pytest.fail('mode %d NCHW: %d of %d elements differ, by up to %d ulp' % (mode, cnt, want.size, ulp))
        got4 = _fbt_abi(img_d, N, H, W, oh, ow, mode, True)
        want4 = R.fast_base_transform(img, oh, ow, mode, True)
        assert (R.bits(got4[..., 3]) == 0).all(), 'the fourth NHWC4 channel is not +0.0'
        if not R.same_bits(got4, want4):
            ulp, cnt = R.ulp_distance(got4, want4)
            pytest.fail('mode %d NHWC4: %d of %d elements differ, by up to %d ulp' % (mode, cnt, want4.size, ulp))


@pytest.mark.parametrize('mode', [0, 1, 2, 3])
def test_fast_base_transform_module_bit_for_bit(mode):
    """FastBaseTransform() and to_nhwc4 under each backbone transform (cfg.backbone.transform of the active config replaced for the
    call): the module's own size rule (max_size x max_size), means and standard deviations."""
    import types
    import yolact_amd
    from yolact_amd.utils.augmentations import FastBaseTransform
    yolact_amd.set_cfg('yolact_resnet50_config')
    cfg = yolact_amd.active_cfg()
    tr = ('resnet', 'vgg', 'darknet', types.SimpleNamespace(channel_order='RGB', normalize=False, subtract_means=False,
                                                            to_float=False))[mode]
    case = (3, 37, 53, cfg.max_size, cfg.max_size)
    img = R.fbt_input(case, seed=mode)
    old = cfg.backbone.transform
    cfg.backbone.transform = tr
    try:
        t = FastBaseTransform()
        got = t(torch.from_numpy(img).to(DEV)).cpu().numpy()
        got4 = t.to_nhwc4(torch.from_numpy(img).to(DEV)).cpu().numpy()
    finally:
        cfg.backbone.transform = old
    assert R.same_bits(got, R.fast_base_transform(img, cfg.max_size, cfg.max_size, mode, False))
    assert R.same_bits(got4, R.fast_base_transform(img, cfg.max_size, cfg.max_size, mode, True))


# ---- coverage of the timed plans ---------------------------------------------------------------------------------------------------

def _forms(plan):
    lib = L.lib()
    out = []
    for fn, args, name, _ in plan.ops:
        if fn == 'input':
            out.append((name, ('input', plan.in_args[3], None, None, bool(plan.h2))))
        elif fn == 'stem':
            out.append((name, ('stem', 64, None, None, bool(args.y_amax))))
        elif fn is lib.ymi_bilinear_nhwc_f32:
            explicit = args[8].value > 0 or args[9].value > 0
            assert (args[8].value > 0) == (args[9].value > 0)
            if explicit:
                assert args[8].value == 0.5 and args[9].value == 0.5, 'an explicit scale other than the 0.5 the cases run'
            out.append((name, ('bilinear', args[5], explicit, bool(args[10]), False)))
        elif fn is lib.ymi_maxpool3x3s2_nhwc_f32:
            out.append((name, ('maxpool', args[5], None, None, False)))
        elif fn is lib.ymi_bilinear_add_nhwc_f32:
            out.append((name, ('bilinear_add', args[5], None, None, args[8] is not None)))
    return out


@pytest.mark.parametrize('B', [1, 8])
def test_timed_plan_entry_and_layout_ops_are_all_covered(B):
    import yolact_amd
    from yolact_amd.utils.synth import synth_images, synth_state_dict
    yolact_amd.set_cfg('yolact_resnet50_config')
    from yolact_amd.yolact import Yolact
    net = Yolact()
    net.load_state_dict_compat(synth_state_dict([(k, tuple(v.shape)) for k, v in net.state_dict().items()], seed=0, conf_gain=0.04))
    net = net.to(DEV)
    x = synth_images(B, 550, 550, seed=1234).to(DEV)
    plan = net.plan_for(x)
    found = _forms(plan)
    covered = R.covered_forms()
    print('batch %d timed plan: %s' % (B, found))
    for name, form in found:
        assert form in covered, (name, form)
    assert any(f[0] in ('stem', 'input') for _, f in found)


# ---- stale magnitude bounds --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('native', ['1', '0'], ids=['native', 'python-loop'])
def test_quiet_batch_after_a_loud_one_gives_the_fresh_bits(native, monkeypatch):
    """engine.Plan: "magnitude bounds are re-derived by every run" (a zero_() in the Python loop, a YMI_OP_MEMSET in
    csrc/plan_exec.cpp).  A bound left over from the loud run would give the quiet one a scale 2^10 too small."""
    from gpu_utils import build_net
    from helpers import case_images, load_golden, same_bits
    monkeypatch.setenv('YOLACT_AMD_NATIVE_EXEC', native)
    meta, _ = load_golden('r50_dense')
    x = case_images(meta).to(DEV)
    keys = ('loc', 'conf_logits', 'mask', 'proto')
    net = build_net(meta)
    plan = net.plan_for(x)
    assert plan.h2, 'not an fp16x2 plan: the slots would not be in use'
    assert plan.native_exec == (native == '1')
    fresh = {k: v.clone() for k, v in net.forward_raw(x).items() if k in keys}
    loud = {k: v.clone() for k, v in net.forward_raw(x * 1024.0).items() if k in keys}
    after = {k: v.clone() for k, v in net.forward_raw(x).items() if k in keys}
    assert not torch.equal(loud['proto'], fresh['proto'])
    same_bits(after, fresh)
    # and against a net that never saw the loud batch
    same_bits({k: v for k, v in build_net(meta).forward_raw(x).items() if k in keys}, fresh)
