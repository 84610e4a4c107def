"""ymi_conv_wgrad_nhwc_h2 without a GPU: the entry rejects exactly what ymi_conv_wgrad_nhwc_f32 rejects, with the same codes (the
bad-descriptor lists of tests/test_heads_train_host.py and tests/test_fpn_train_host.py); the workspace query is positive and grows with
the chunk count; the mode switch of train_ops and Trainer refuses other values; and for every case of tests/test_gpu_wgrad_h2.py the
numpy restatement of the kernel's arithmetic (tests/wgrad_h2_ref.py) meets that case's bar on the CPU while the two wrong
restatements, the x_l g_h product dropped and one block of 32 channels of g dropped, miss it: the bars can be met, and they can fail.
The three cases whose answer is fixed by zeros or by the Inf (g = 0, x = 0, one +Inf) have nothing a wrong restatement could miss
and are checked for their exact answers instead.
"""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wgrad_h2_ref as R  # noqa: E402
from gpu_utils import rel_err  # noqa: E402
import yolact_amd  # noqa: E402,F401
from yolact_amd import _lib as L  # noqa: E402
from yolact_amd.layers import train_ops as TO  # noqa: E402

ENULL, EARG, ESHAPE = -3, -1, -2


def wgrad_desc(**kw):
    d = L.ConvWgradDesc()
    d.B, d.H, d.W, d.Cin, d.Cout, d.ldg, d.kh, d.kw, d.pad = 1, 2, 2, 32, 5, 32, 3, 3, 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_the_entry_is_declared_and_the_abi_number_stays():
    lib = L.lib()
    assert lib.ymi_abi_version() == 9 and L.ABI_VERSION == 9 and L.WS_CONV_WGRAD_H2 == 29 and L.WS_PRECONV_WGRAD == 28
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'yolact_amd.h')).read()
    assert '#define YMI_ABI_VERSION 9' in header and 'YMI_WS_CONV_WGRAD_H2 = 29' in header
    assert 'int ymi_conv_wgrad_nhwc_h2(const ymi_conv_wgrad_desc *d, void *stream);' in header
    bound = {name: (res, args) for name, res, args in L.SYMBOLS}
    assert bound['ymi_conv_wgrad_nhwc_h2'] == bound['ymi_conv_wgrad_nhwc_f32']
    assert hasattr(lib, 'ymi_conv_wgrad_nhwc_h2')


def test_it_rejects_what_the_fp32_entry_rejects_with_the_same_codes():
    lib = L.lib()
    buf = (C.c_float * 64)()
    ptr = C.cast(buf, C.c_void_p)
    aligned = C.c_void_p((ptr.value + 15) // 16 * 16)

    def wg(**kw):
        d = wgrad_desc(**kw)
        for k, v in dict(x=ptr, g=ptr, dw=ptr, db=ptr, ws=aligned, ws_bytes=1 << 30).items():
            if k not in kw:
                setattr(d, k, v)
        return d
    assert lib.ymi_conv_wgrad_nhwc_h2(None, None) == lib.ymi_conv_wgrad_nhwc_f32(None, None) == ENULL
    assert lib.ymi_workspace_bytes(L.WS_CONV_WGRAD_H2, None) == ENULL
    earg = (dict(B=0), dict(Cout=0), dict(kh=5, kw=5, pad=2), dict(kh=3, kw=3, pad=0), dict(kh=1, kw=1, pad=1), dict(kh=3, kw=1),
            dict(stride=3), dict(stride=-1), dict(stride=4), dict(stride=2, kh=5, kw=5, pad=2), dict(stride=2, kh=3, kw=3, pad=0),
            dict(stride=2, B=0))
    eshape = (dict(Cin=48), dict(ldg=4), dict(ws_bytes=16), dict(ws=C.c_void_p(aligned.value + 4)),
              dict(stride=2, Cin=48), dict(stride=2, ldg=4), dict(stride=2, ws_bytes=16), dict(stride=2, ws=C.c_void_p(aligned.value + 4)),
              dict(stride=2, B=1 << 12, H=1 << 10, W=1 << 10))         # x of 2^37 elements
    enull = (dict(g=None), dict(ws=None), dict(dw=None, db=None), dict(x=None),
             dict(stride=2, g=None), dict(stride=2, ws=None), dict(stride=2, dw=None, db=None), dict(stride=2, x=None))
    for bad in earg:
        assert lib.ymi_conv_wgrad_nhwc_h2(C.byref(wg(**bad)), None) == lib.ymi_conv_wgrad_nhwc_f32(C.byref(wg(**bad)), None) == EARG, bad
        assert lib.ymi_workspace_bytes(L.WS_CONV_WGRAD_H2, C.byref(wg(**bad))) == EARG, bad
    for bad in eshape:
        assert lib.ymi_conv_wgrad_nhwc_h2(C.byref(wg(**bad)), None) == lib.ymi_conv_wgrad_nhwc_f32(C.byref(wg(**bad)), None) == ESHAPE, bad
    for bad in enull:
        assert lib.ymi_conv_wgrad_nhwc_h2(C.byref(wg(**bad)), None) == lib.ymi_conv_wgrad_nhwc_f32(C.byref(wg(**bad)), None) == ENULL, bad
    # the workspace query reads the shape alone, as the fp32 entry's does
    for Cin in (16, 48, 33):
        assert lib.ymi_workspace_bytes(L.WS_CONV_WGRAD_H2, C.byref(wgrad_desc(Cin=Cin))) == ESHAPE
    assert lib.ymi_workspace_bytes(L.WS_CONV_WGRAD_H2, C.byref(wgrad_desc(Cin=0))) == EARG


def chunks_of(**kw):
    """The chunk count of a shape, from the fp32 entry's workspace: chunks * (K * Cout + Cout) floats (Cout % 4 == 0: no padding)."""
    d = wgrad_desc(**kw)
    return L.lib().ymi_workspace_bytes(L.WS_CONV_WGRAD, C.byref(d)) // (4 * (d.kh * d.kw * d.Cin * d.Cout + d.Cout))


def test_the_workspace_is_positive_and_grows_with_the_chunk_count():
    lib = L.lib()
    ws = lambda **kw: lib.ymi_workspace_bytes(L.WS_CONV_WGRAD_H2, C.byref(wgrad_desc(**kw)))
    part = lambda n: (4 * n + 15) // 16 * 16
    seen = []
    for H in (2, 8, 24, 80):                            # 1x1, 32 -> 32 on 1 x H x 4: 1, 1, 3 and 10 chunks of 32 positions
        shape = dict(B=1, H=H, W=4, Cin=32, Cout=32, ldg=32, kh=1, kw=1, pad=0)
        n = chunks_of(**shape)
        seen.append((n, ws(**shape)))
        # the fp32 entry's two parts, the two offset tables over chunks * 32 positions (+ 64 entries each), 2 * 1024 partial bounds
        assert ws(**shape) == part(n * 32 * 32) + part(n * 32) + part(n * 32 + 64) * 2 + part(2048) > 0
    assert [n for n, _ in seen] == [1, 1, 3, 10]
    assert seen[0][1] == seen[1][1] < seen[2][1] < seen[3][1]
    big = dict(B=8, H=69, W=69, Cin=256, Cout=256, ldg=256)                 # 15 chunks of 2560 positions
    assert chunks_of(**big) == 15
    assert ws(**big) == 4 * 15 * (2304 * 256 + 256) + part(9 * 15 * 2560 + 64) + part(15 * 2560 + 64) + part(2048)
    assert ws(stride=2, **big) < ws(**big)


def test_the_mode_switch_refuses_other_values():
    assert TO.get_wgrad_mode() == 'fp32'
    with TO.wgrad_mode('fp16x2'):
        assert TO.get_wgrad_mode() == 'fp16x2'
        with TO.wgrad_mode('fp32'):
            assert TO.get_wgrad_mode() == 'fp32'
        assert TO.get_wgrad_mode() == 'fp16x2'
    assert TO.get_wgrad_mode() == 'fp32'
    assert TO.set_wgrad_mode('fp16x2') == 'fp32' and TO.set_wgrad_mode('fp32') == 'fp16x2'
    for bad in ('bf16', 'fp16', None, 1):
        with pytest.raises(ValueError, match="'fp32' and 'fp16x2'"):
            TO.set_wgrad_mode(bad)
        with pytest.raises(ValueError, match="'fp32' and 'fp16x2'"):
            with TO.wgrad_mode(bad):
                pass
    assert TO.get_wgrad_mode() == 'fp32'
    with pytest.raises(RuntimeError):                    # the mode is restored when the body raises
        with TO.wgrad_mode('fp16x2'):
            raise RuntimeError('x')
    assert TO.get_wgrad_mode() == 'fp32'
    from yolact_amd.training import Trainer
    with pytest.raises(ValueError, match="'fp32' and 'fp16x2'"):
        Trainer(None, wgrad='tf32')


def test_the_scale_rule_is_ymi_h2_scale():
    for amax, want in ((1.0, 2.0 ** 13), (1.5, 2.0 ** 13), (2.0, 2.0 ** 12), (2.0 ** -60, 2.0 ** 73), (2.0 ** 50 * 1.9, 2.0 ** -37),
                       (0.0, 1.0), (float('inf'), 1.0), (float('nan'), 1.0)):
        assert R.h2_scale(amax) == want, amax
    for amax in (3.7, 2.0 ** -60 * 1.3, 2.0 ** 52):
        assert 2.0 ** 13 <= amax * R.h2_scale(amax) < 2.0 ** 14


SHAPE_CASES = [n for n, c in R.CASES.items() if c[8] == 'shape']


@pytest.mark.parametrize('name', SHAPE_CASES)
def test_the_restatement_meets_the_bar_and_the_wrong_ones_miss_it(name):
    x, g = R.inputs(name)
    k, stride = R.CASES[name][6:8]
    ref = R.references(name)
    bar = R.bar(ref['dw32'], ref['dw64'])
    right = rel_err(R.restate(x, g, k, stride), ref['dw64'])
    no_lh = rel_err(R.restate(x, g, k, stride, drop_lh=True), ref['dw64'])
    no_block = rel_err(R.restate(x, g, k, stride, drop_block=(g.shape[3] - 1) // 32 // 2), ref['dw64'])
    print('%s: bar %.3e, restatement %.3e, without lh %.3e, without a block of g %.3e' % (name, bar, right, no_lh, no_block))
    assert right <= bar < no_lh and bar < no_block
    assert ref['dw64'].shape == (k * k * x.shape[3], g.shape[3]) and bool(ref['dw64'].ne(0).all())


@pytest.mark.parametrize('name', [n for n, c in R.CASES.items() if c[8] in R.RANGE_FINITE])
def test_the_restatement_is_within_the_elementwise_bound_and_the_wrong_ones_are_not(name):
    x, g = R.inputs(name)
    k, stride = R.CASES[name][6:8]
    want = R.references(name)['dw64']
    E = R.error_bound(x, g, k, stride)
    assert bool(torch.isfinite(want).all()) and bool((E > 0).all())
    assert float(want.abs().max()) > 2.0 ** -126                              # an fp32 result that is normal
    over = lambda got: float(((got - want).abs() / E).max())
    right, no_lh, no_block = (over(R.restate(x, g, k, stride, **kw)) for kw in ({}, dict(drop_lh=True), dict(drop_block=0)))
    print('%s: largest |error| / E: restatement %.3e, without lh %.3e, without a block of g %.3e' % (name, right, no_lh, no_block))
    assert right <= 1.0 < no_lh and 1.0 < no_block


def test_the_cases_with_a_fixed_answer():
    k, stride = R.S57[6:8]
    x, g = R.inputs('range_g_zero')
    assert bool(g.eq(0).all()) and bool(R.restate(x, g, k, stride).eq(0).all()) and bool(R.references('range_g_zero')['dw64'].eq(0).all())
    x, g = R.inputs('range_x_zero')
    assert bool(x.eq(0).all()) and bool(R.restate(x, g, k, stride).eq(0).all())
    x, g = R.inputs('range_inf')
    col = R.INF_AT[3]
    assert int(torch.isinf(g).sum()) == 1 and bool(torch.isinf(g[R.INF_AT]))
    got = R.restate(x, g, k, stride)
    assert not bool(torch.isfinite(got[:, col]).any())
