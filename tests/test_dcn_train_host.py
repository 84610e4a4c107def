"""The train path's deformable convolution on the CPU: the oracle of tests/dcn_train_ref.py is tied to the plain bottleneck's, two
deliberately wrong variants are shown to miss the bars tests/test_gpu_dcn_train.py applies, and what needs no GPU is checked: the
validators' messages, the refusals that stay, the ABI number, the new symbols, argument validation of the three ymi_dcn_cols_*
entries, and the construction of every case the GPU tests run (sample points off the kinks and in the fp64 points' cells, ReLU
margins of the bottleneck cases).
"""
import ctypes as C
import os
import sys

import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import backbone_train_ref as R  # noqa: E402
import dcn_train_ref as D  # noqa: E402
from helpers import rel_err  # noqa: E402
import yolact_amd  # noqa: E402
from yolact_amd import _lib as L  # noqa: E402
from yolact_amd import modules as M  # noqa: E402
from yolact_amd.layers import train_ops as TO  # noqa: E402

ENULL, EARG, ESHAPE = -3, -1, -2
HERE = os.path.dirname(os.path.abspath(__file__))
ROUND_OFF = 1e-12


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('batch_stats', [False, True], ids=['frozen', 'batch_stats'])
@pytest.mark.parametrize('variant', list(D.BLOCK_SPECS))
def test_zero_offset_mask_conv_is_the_plain_bottleneck_at_half_weight(variant, batch_stats):
    """conv_offset_mask = 0: every point is a pixel, every modulation 1/2, so conv2 is the plain 3x3 with half the weight plus the
    bias.  bottleneck_ref has no bias: with frozen statistics it is bn2's running_mean lowered by it, with batch statistics it cancels
    in the normalisation.  Output, d_x and every gradient the two have in common (conv2.weight: half the plain one's), in fp64."""
    spec, x, params, up = D.block_case(variant, batch_stats)
    stride = spec[2]
    params = dict(params)
    params['conv2.conv_offset_mask.weight'] = torch.zeros_like(params['conv2.conv_offset_mask.weight'])
    params['conv2.conv_offset_mask.bias'] = torch.zeros_like(params['conv2.conv_offset_mask.bias'])
    got = D.run_block_ref(x, params, stride, up, batch_stats, torch.float64)
    plain = {n: t for n, t in params.items() if n not in D.DCN_NAMES}
    plain['conv2.weight'] = params['conv2.weight'].double() / 2
    if not batch_stats:
        plain['bn2.running_mean'] = params['bn2.running_mean'].double() - params['conv2.bias'].double()
    want = R.run_ref(x, plain, [('', stride)], up, batch_stats, torch.float64)
    skip = {'d_conv2.weight', 'new_bn2.running_mean'}
    for k in want:
        if k.startswith('_') or k in skip:
            continue
        assert rel_err(got[k], want[k]) <= ROUND_OFF, k
    assert rel_err(2 * got['d_conv2.weight'], want['d_conv2.weight']) <= ROUND_OFF
    if batch_stats:      # the batch mean of conv2's output carries the bias
        shift = 0.1 * params['conv2.bias'].double()
        assert rel_err(got['new_bn2.running_mean'] - shift, want['new_bn2.running_mean']) <= ROUND_OFF


@pytest.mark.parametrize('wrong,misses', [('no_sigmoid_grad', ('om',)), ('swapped_offsets', ('y', 'x', 'om', 'weight'))])
def test_the_bars_reject_a_wrong_operation(wrong, misses):
    case = D.op_case(D.SMALL)
    g64, g32 = D.op_grads(case, torch.float64), D.op_grads(case, torch.float32)
    bars = D.bars(g64, g32)
    bad = D.op_grads(case, torch.float64, wrong)
    for k in g64:
        e = rel_err(bad[k], g64[k])
        print('%s %s: rel_err %.3e (bar %.3e)' % (wrong, k, e, bars[k]))
        assert (e > bars[k]) == (k in misses), (k, e, bars[k])
        assert bars[k] <= 1e-4                                  # the bar itself stays fp32-class
    if wrong == 'no_sigmoid_grad':                             # only the logit channels are wrong
        assert rel_err(bad['om'][:, :18], g64['om'][:, :18]) <= ROUND_OFF and rel_err(bad['om'][:, 18:], g64['om'][:, 18:]) > 0.1


def test_wrong_bottleneck_variants_miss_the_bar():
    spec, x, params, up = D.block_case('proj_s2', False)
    r64, r32 = (D.run_block_ref(x, params, spec[2], up, False, dt) for dt in (torch.float64, torch.float32))
    for wrong in ('no_sigmoid_grad', 'swapped_offsets'):
        bad = D.run_block_ref(x, params, spec[2], up, False, torch.float64, wrong=wrong)
        k = 'd_conv2.conv_offset_mask.bias'
        bar = max(4 * rel_err(r32[k], r64[k]), D.EXACT_BAR)
        assert rel_err(bad[k], r64[k]) > bar, (wrong, rel_err(bad[k], r64[k]), bar)


# ---- the cases of the GPU tests --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(D.OP_CASES) + ['adversarial', 'band'])
def test_sample_points_of_the_cases_are_off_the_kinks(name):
    case = {'adversarial': D.adversarial_case, 'band': D.band_case}[name]() if name not in D.OP_CASES else D.op_case(name)
    lo, hi, same = D.point_fractions(case)
    assert lo >= 1 / 16 - 1e-6 and hi <= 15 / 16 + 1e-6 and same, (lo, hi, same)
    x, om = case[0], case[1]
    assert om.shape[1] == 27 and om.dtype == torch.float32


def test_special_cases_are_what_they_say():
    from dcn_ref import sample_points
    x, om, w, b, gy, stride = D.adversarial_case()
    h, wc = sample_points(9, 9, om[:, :18], stride, 1)
    assert tuple(x.shape) == (1, 32, 9, 9) and bool(((h.floor() == 4) & (wc.floor() == 4)).all())
    x, om, w, b, gy, stride = D.outside_case()
    h, wc = sample_points(x.shape[2], x.shape[3], om[:, :18], stride, 1)
    assert bool((h <= -2).all())
    x, om, w, b, gy, stride = D.band_case()
    h, wc = sample_points(x.shape[2], x.shape[3], om[:, :18], stride, 1)
    assert bool((h.floor() >= D.BAND[0]).all()) and bool((h.floor() + 1 <= D.BAND[1]).all())
    assert not bool(D.zero_om_case()[1].ne(0).any())


@pytest.mark.parametrize('batch_stats', [False, True], ids=['frozen', 'batch_stats'])
@pytest.mark.parametrize('variant', list(D.BLOCK_SPECS))
def test_margins_of_the_bottleneck_cases(variant, batch_stats):
    spec, x, params, up = D.block_case(variant, batch_stats)
    relus, (lo, hi), same = D.block_margins(x, params, spec[2], up, batch_stats)
    print(variant, batch_stats, 'tightest ReLU margin: %s %.3e, fp32 deviation %.3e' % R.tightest(relus), 'fractions', lo, hi)
    R.assert_margins(relus)                                     # 16 times the fp32 deviation
    assert same and lo >= 1 / 8 and hi <= 7 / 8


# ---- the surface that needs no GPU -------------------------------------------------------------------------------------------------------------
def test_abi_number_and_the_new_symbols():
    lib = L.lib()
    assert lib.ymi_abi_version() == 9 and L.ABI_VERSION == 9
    header = open(os.path.join(HERE, '..', 'include', 'yolact_amd.h')).read()
    assert '#define YMI_ABI_VERSION 9' in header
    names = [n for n, _, _ in L.SYMBOLS]
    for name in ('ymi_dcn_cols_fwd_f32', 'ymi_dcn_cols_entries_f32', 'ymi_dcn_cols_bwd_f32'):
        assert name in header and name in names and hasattr(lib, name)
    assert 'ymi_dcn_cols_desc' in header and C.sizeof(L.DcnColsDesc) == 11 * 8 + 8 * 4
    for fn in ('deform_conv', 'dcn_bottleneck', 'check_dcn_bottleneck', 'check_deform', 'bottleneck', 'check_bottleneck'):
        assert callable(getattr(TO, fn))


def test_argument_validation_returns_codes_without_a_gpu():
    lib = L.lib()
    buf = (C.c_float * 64)()
    aligned = C.c_void_p((C.cast(buf, C.c_void_p).value + 15) // 16 * 16)
    off = C.c_void_p(aligned.value + 4)
    ptrs = ('x', 'om', 'col', 'dcol', 'g_om', 'gx', 'keys', 'coef', 'sorted_keys', 'order', 'seg')

    def desc(**kw):
        d = L.DcnColsDesc()
        d.B, d.H, d.W, d.Cin, d.Ho, d.Wo, d.stride = 1, 5, 7, 32, 5, 7, 1
        for k in ptrs:
            setattr(d, k, aligned)
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    fwd, ent, bwd = lib.ymi_dcn_cols_fwd_f32, lib.ymi_dcn_cols_entries_f32, lib.ymi_dcn_cols_bwd_f32
    for fn in (fwd, ent, bwd):
        assert fn(None, None) == ENULL
        for bad in (dict(B=0), dict(H=0), dict(W=-1), dict(Cin=0), dict(stride=0), dict(stride=3)):
            assert fn(C.byref(desc(**bad)), None) == EARG, bad
        for bad in (dict(Cin=48), dict(Ho=4), dict(Wo=8), dict(stride=2), dict(stride=2, Ho=3, Wo=3),
                    dict(B=1 << 10, H=1 << 9, W=1 << 9, Ho=1 << 9, Wo=1 << 9),                  # x of 2^33 elements
                    dict(B=64, H=1 << 10, W=1 << 10, Ho=1 << 10, Wo=1 << 10),                   # 36 * 2^26 entries, col of 9 * 2^31
                    dict(B=32, H=1 << 9, W=1 << 9, Ho=1 << 9, Wo=1 << 9)):                      # x of 2^28 elements, col of 9 * 2^28
            assert fn(C.byref(desc(**bad)), None) == ESHAPE, bad
    run = lambda fn, **kw: fn(C.byref(desc(**kw)), None)
    assert run(fwd, stride=2, Ho=3, Wo=4, x=None) == ENULL            # (a valid stride-2 geometry reaches the pointer checks)
    for bad in (dict(x=None), dict(om=None), dict(col=None)):
        assert run(fwd, **bad) == ENULL, bad
    assert run(fwd, x=off) == ESHAPE and run(fwd, col=off) == ESHAPE
    for bad in (dict(om=None), dict(keys=None), dict(coef=None)):
        assert run(ent, **bad) == ENULL, bad
    assert run(ent, keys=off) == ESHAPE and run(ent, coef=off) == ESHAPE
    assert run(bwd, g_om=None, gx=None) == 0                            # nothing wanted: no launch
    for bad in (dict(dcol=None), dict(gx=None, x=None), dict(gx=None, om=None), dict(g_om=None, sorted_keys=None),
                dict(g_om=None, order=None), dict(g_om=None, coef=None), dict(g_om=None, seg=None)):
        assert run(bwd, **bad) == ENULL, bad
    assert run(bwd, dcol=off) == ESHAPE and run(bwd, gx=off) == ESHAPE and run(bwd, x=off) == ESHAPE


class _OnGpu(torch.Tensor):
    """A CPU tensor that says it lives on the GPU: the refusals behind require_cuda are reached without one."""
    is_cuda = True


def _gpu(t):
    return t.as_subclass(_OnGpu)


def test_deform_conv_validators():
    w = torch.zeros(8, 32, 3, 3)
    assert TO.check_deform(w, 1) == 1 and TO.check_deform(w, (2, 2)) == 2
    for kw, what in ((dict(weight=torch.zeros(8, 32, 5, 5)), '5 x 5'), (dict(weight=torch.zeros(8, 32, 3)), 'shape'),
                     (dict(stride=3), 'stride = 3'), (dict(stride=(1, 2)), 'stride'), (dict(padding=0), 'padding = 0'),
                     (dict(dilation=2), 'dilation = 2'), (dict(deformable_groups=2), 'deformable_groups = 2'),
                     (dict(weight=torch.zeros(8, 24, 3, 3)), 'Cin = 24')):
        args = dict(weight=w, stride=1, padding=1, dilation=1, deformable_groups=1)
        args.update(kw)
        with pytest.raises(NotImplementedError, match=what):
            TO.check_deform(**args)
    # the GEMM half: a 1 x 1 convolution of 9 * 512 channels is inside what check_conv takes
    assert TO.check_conv(torch.zeros(4, 9 * 512, 1, 1), 0) == (1, 0)
    x, om = torch.zeros(1, 5, 7, 32), torch.zeros(1, 5, 7, 27)
    with pytest.raises(RuntimeError, match='GPU'):
        TO.deform_conv(x, om, w, None)
    with pytest.raises(RuntimeError, match='GPU'):
        TO.deform_conv(_gpu(x), om, _gpu(w), None)
    with pytest.raises(NotImplementedError, match='stride = 3'):
        TO.deform_conv(_gpu(x), _gpu(om), _gpu(w), None, 3)
    with pytest.raises(ValueError, match='om'):
        TO.deform_conv(_gpu(x), _gpu(torch.zeros(1, 5, 7, 18)), _gpu(w), None)
    with pytest.raises(ValueError, match='om'):
        TO.deform_conv(_gpu(x), _gpu(om), _gpu(w), None, 2)
    with pytest.raises(ValueError, match='x '):
        TO.deform_conv(_gpu(torch.zeros(1, 5, 7, 64)), _gpu(om), _gpu(w), None)
    with pytest.raises(ValueError, match='bias'):
        TO.deform_conv(_gpu(x), _gpu(om), _gpu(w), _gpu(torch.zeros(7)))
    with pytest.raises(NotImplementedError, match='column tensor'):
        TO.deform_conv(_gpu(torch.zeros(1, 1, 1, 32).expand(64, 512, 512, 32)), _gpu(torch.zeros(1, 1, 1, 27).expand(64, 512, 512, 27)),
                       _gpu(w), None)


def test_bottleneck_validators():
    dcn = M.Bottleneck(64, 32, use_dcn=True)
    TO.check_dcn_bottleneck(dcn, 'layers.1.2')
    TO.check_dcn_bottleneck(M.Bottleneck(64, 32, 2, nn.Sequential(nn.Conv2d(64, 128, 1, stride=2, bias=False), nn.BatchNorm2d(128)),
                                         use_dcn=True))
    # what stays: the plain entries refuse a DCN block, by name
    with pytest.raises(NotImplementedError, match='layers.1.2 is a DCN block'):
        TO.check_bottleneck(dcn, 'layers.1.2')
    with pytest.raises(NotImplementedError, match='DCN block'):
        TO.bottleneck(_gpu(torch.zeros(1, 4, 4, 64)), dcn)
    with pytest.raises(RuntimeError, match='GPU'):
        TO.dcn_bottleneck(torch.zeros(1, 4, 4, 64), dcn)
    with pytest.raises(NotImplementedError, match='layers.0.1 is not a DCN block'):
        TO.check_dcn_bottleneck(M.Bottleneck(64, 32), 'layers.0.1')
    with pytest.raises(NotImplementedError, match='b is a Conv2d'):
        TO.check_dcn_bottleneck(nn.Conv2d(3, 3, 1), 'b')
    odd = M.Bottleneck(64, 32, use_dcn=True)
    odd.conv1 = nn.Conv2d(64, 32, 1, bias=True)
    with pytest.raises(NotImplementedError, match=r'blk\.conv1'):
        TO.check_dcn_bottleneck(odd, 'blk')
    odd = M.Bottleneck(64, 32, use_dcn=True)
    odd.conv2.conv_offset_mask = nn.Conv2d(32, 27, 3, padding=1, bias=False)
    with pytest.raises(NotImplementedError, match=r'blk\.conv2\.conv_offset_mask'):
        TO.check_dcn_bottleneck(odd, 'blk')
    odd = M.Bottleneck(64, 32, use_dcn=True)
    odd.conv2.deformable_groups = 2
    with pytest.raises(NotImplementedError, match=r'blk\.conv2: deformable_groups = 2'):
        TO.check_dcn_bottleneck(odd, 'blk')
    odd = M.Bottleneck(64, 32, 2, use_dcn=True)
    odd.conv2.stride = (1, 1)
    with pytest.raises(NotImplementedError, match='stride'):
        TO.check_dcn_bottleneck(odd, 'blk')
    odd = M.Bottleneck(64, 24, use_dcn=True)
    with pytest.raises(NotImplementedError, match='Cin = 24'):
        TO.check_dcn_bottleneck(odd, 'blk')


def test_the_yolact_methods_keep_refusing_and_the_trainer_takes_a_forward():
    import inspect
    from yolact_amd import train_net as TN
    from yolact_amd.training import Trainer
    before = yolact_amd.config.cfg.copy()
    try:
        from yolact_amd.yolact import Yolact
        yolact_amd.set_cfg('yolact_plus_resnet50_config')
        net = Yolact()
        with pytest.raises(NotImplementedError, match=r'backbone\.layers\.1\.\d+ is a DCN block'):
            net._check_backbone()
        with pytest.raises(NotImplementedError):
            net.train()
        for si, layer in enumerate(net.backbone.layers):
            for bi, blk in enumerate(layer):
                (TO.check_dcn_bottleneck if blk.use_dcn else TO.check_bottleneck)(blk, 'backbone.layers.%d.%d' % (si, bi))
        assert sum(blk.use_dcn for layer in net.backbone.layers for blk in layer) == 13
    finally:
        yolact_amd.config.cfg.replace(before)
    sig = inspect.signature(Trainer.__init__)
    assert list(sig.parameters)[-1] == 'forward' and sig.parameters['forward'].default is None
    assert 'dcn_bottleneck' in inspect.getsource(TN.backbone) and '_tmp_img_h' in inspect.getsource(TN.forward)
