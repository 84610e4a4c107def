"""train_ops.conv_mode and ymi_conv_pack_h2_f32 without a GPU: the entry is declared and the ABI number and every YMI_WS_* value stay;
every bad descriptor gets its code before any HIP call; the mode switch of train_ops and Trainer(conv=...) refuse other values and
restore the old mode; the numpy restatement of the pack (tests/conv_h2_ref.py) equals engine.split2_planes_f16 of the torch packing bit
for bit in both layouts; and for every case of tests/test_gpu_conv_h2.py the numpy restatement of the mode's arithmetic meets that
case's bar on the CPU while the two wrong restatements, the x_l w_h product dropped and one block of 32 input channels dropped, miss
it: the bars can be met, and they can fail.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_h2_ref as R  # noqa: E402
from gpu_utils import rel_err  # noqa: E402
import yolact_amd  # noqa: E402,F401
from yolact_amd import _lib as L  # noqa: E402
from yolact_amd.layers import train_ops as TO  # noqa: E402

ENULL, EARG, ESHAPE = -3, -1, -2


def test_the_entry_is_declared_and_the_abi_number_stays():
    lib = L.lib()
    assert lib.ymi_abi_version() == 9 and L.ABI_VERSION == 9
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'yolact_amd.h')).read()
    assert '#define YMI_ABI_VERSION 9' in header
    assert 'int ymi_conv_pack_h2_f32(const ymi_conv_pack_desc *d, void *stream);' in header
    bound = {name: (res, args) for name, res, args in L.SYMBOLS}
    assert bound['ymi_conv_pack_h2_f32'][0] is C.c_int and hasattr(lib, 'ymi_conv_pack_h2_f32')
    assert C.sizeof(L.ConvPackDesc) == 80                                # 6 pointers, 8 int32
    # no workspace selector has moved (the pack needs none and adds none)
    names = ('WINO_V WINO_M SPLITK MASK_IOU JPEG_COEFS JPEG_PLANES DETECT_SCORES_T DETECT_PER_PRIOR DETECT_CAND DETECT_REC AMAX_SLOT '
             'RLE_COUNTS DETECT_GREEDY JPEG_ENC JPEG_ENC_OUT MASK_LOSS MATCH BOX_LOSS CLASS_LOSS SEGM_LOSS MASKIOU_INPUT CONV_BWD '
             'MASKIOU_HEAD CONV_WGRAD BN STEM_WGRAD AUGMENT PRECONV_WGRAD CONV_WGRAD_H2').split()
    for value, name in enumerate(names, 1):
        assert getattr(L, 'WS_' + name) == value, name
        assert 'YMI_WS_%s = %d' % (name, value) in header, name
    assert 'YMI_WS_CONV_PACK' not in header and not hasattr(L, 'WS_CONV_PACK_H2')


def pack_desc(**kw):
    """A valid descriptor on host memory (never launched: each test breaks one field), mode 1 so that ld is read."""
    buf = (C.c_float * 64)()
    base = (C.cast(buf, C.c_void_p).value + 15) // 16 * 16
    d = L.ConvPackDesc()
    d._keep = buf
    d.w[0], d.w[1], d.w[2] = base + 4, base + 4, base + 4               # sources need no 16-byte alignment
    d.cout[0], d.cout[1], d.cout[2] = 5, 7, 9
    d.planes, d.winv, d.w32 = base, base + 16, base + 32
    d.n, d.Cin, d.k, d.mode, d.ld = 3, 32, 3, 1, 32
    for name, v in kw.items():
        if name in ('w', 'cout'):
            for i, e in enumerate(v):
                getattr(d, name)[i] = e
        else:
            setattr(d, name, v)
    return d, base


def test_every_bad_descriptor_gets_its_code():
    lib = L.lib()
    call = lambda **kw: lib.ymi_conv_pack_h2_f32(C.byref(pack_desc(**kw)[0]), None)
    base = pack_desc()[1]
    assert lib.ymi_conv_pack_h2_f32(None, None) == ENULL
    for bad in (dict(planes=None), dict(winv=None), dict(w=[None, base, base]), dict(w=[base, base, None]), dict(n=1, w=[None, base, base])):
        assert call(**bad) == ENULL, bad
    for bad in (dict(n=0), dict(n=4), dict(n=-1), dict(k=2), dict(k=5), dict(k=0), dict(mode=2), dict(mode=-1), dict(Cin=0), dict(Cin=-32),
                dict(cout=[5, 0, 9]), dict(cout=[-1, 7, 9]), dict(n=1, cout=[0, 7, 9])):
        assert call(**bad) == EARG, bad
    for bad in (dict(Cin=48), dict(Cin=16), dict(ld=48), dict(ld=0), dict(cout=[5, 7, 21]),                 # ld 32 < 33 channels
                dict(planes=base + 4), dict(planes=base + 8), dict(winv=base + 4), dict(w32=base + 36),
                dict(mode=0, Cin=1 << 20, cout=[64, 1, 1]),                                                   # 128 rows x 9 * 2^20
                dict(mode=1, Cin=1 << 20, ld=64)):                                                            # 2^20 rows x 576
        assert call(**bad) == ESHAPE, bad
    # what is not read is not judged: cout and w past n, ld in mode 0, a NULL w32
    assert call(n=1, cout=[5, 0, -3], w=[base, None, None], ld=32, Cin=1 << 21, mode=1) == ESHAPE           # (reaches the size check)
    assert call(mode=0, ld=-5, Cin=1 << 20, cout=[64, 1, 1]) == ESHAPE
    # the limit itself: RowsPad * Kp = 128 * 9 * Cin < 2^29 is the last thing checked, so one row less than the limit would launch;
    # only its rejection is exercised here
    assert call(mode=0, k=1, Cin=1 << 22, cout=[100, 20, 8], w32=None) == ESHAPE                            # 128 * 2^22 = 2^29


def test_the_mode_switch_refuses_other_values_and_restores():
    assert TO.CONV_MODES == ('fp32', 'fp16x2') and TO.get_conv_mode() == 'fp32'
    with TO.conv_mode('fp16x2'):
        assert TO.get_conv_mode() == 'fp16x2' and TO.get_wgrad_mode() == 'fp32'        # a switch of its own
        with TO.conv_mode('fp32'):
            assert TO.get_conv_mode() == 'fp32'
        with TO.wgrad_mode('fp16x2'):
            assert TO.get_conv_mode() == 'fp16x2'
        assert TO.get_conv_mode() == 'fp16x2'
    assert TO.get_conv_mode() == 'fp32'
    assert TO.set_conv_mode('fp16x2') == 'fp32' and TO.set_conv_mode('fp32') == 'fp16x2'
    for bad in ('bf16', 'fp16', None, 1):
        with pytest.raises(ValueError, match="'fp32' and 'fp16x2'"):
            TO.set_conv_mode(bad)
        with pytest.raises(ValueError, match="'fp32' and 'fp16x2'"):
            TO.check_conv_mode(bad)
        with pytest.raises(ValueError, match="'fp32' and 'fp16x2'"):
            with TO.conv_mode(bad):
                pass
    assert TO.get_conv_mode() == 'fp32'
    with pytest.raises(RuntimeError):                    # the mode is restored when the body raises
        with TO.conv_mode('fp16x2'):
            raise RuntimeError('x')
    assert TO.get_conv_mode() == 'fp32'
    # thread-local: another thread starts from the default
    import threading
    seen = []
    with TO.conv_mode('fp16x2'):
        t = threading.Thread(target=lambda: seen.append(TO.get_conv_mode()))
        t.start()
        t.join()
    assert seen == ['fp32']
    from yolact_amd.training import Trainer
    with pytest.raises(ValueError, match="'fp32' and 'fp16x2'"):
        Trainer(None, conv='tf32')
    with pytest.raises(ValueError, match="'fp32' and 'fp16x2'"):
        Trainer(None, conv='fp16x2', wgrad='tf32')
    import inspect
    sig = inspect.signature(Trainer.__init__)
    assert sig.parameters['conv'].default is None and list(sig.parameters)[-1] == 'forward'


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('name', list(R.PACK_CASES))
def test_the_pack_restatement_is_the_torch_packing_bit_for_bit(name, mode):
    ws, ld = R.pack_inputs(name), R.PACK_CASES[name][1]
    planes, winv = R.pack_np(ws, mode, ld)
    want_planes, want_winv = R.pack_torch(ws, mode, ld)
    assert planes.shape == want_planes.shape and planes.dtype == np.int16 and planes.shape[1] % 128 == 0
    assert np.array_equal(planes, want_planes) and np.array_equal(winv.view(np.int32), want_winv.view(np.int32))
    rows = sum(w.shape[0] for w in ws) if mode == 0 else ws[0].shape[1]
    assert not planes[:, rows:].any() and bool((winv[rows:] == 1).all())
    amax = np.abs(R.packing_np([w.numpy() for w in ws], mode, ld)).max(1)[:rows]
    assert bool(((amax == 0) | ((amax >= 2.0 ** -100) & (amax <= 2.0 ** 100))).all())    # the range of the exact oracle
    assert planes[0].any() and planes[1].any()


def test_the_pack_cases_hold_what_they_are_named_for():
    row_max = lambda name, mode: np.abs(R.packing_np([w.numpy() for w in R.pack_inputs(name)], mode, R.PACK_CASES[name][1])).max(1)
    assert row_max('zero_filter', 0)[7] == 0 and row_max('zero_channel', 1)[9] == 0
    m = row_max('mag_filters', 0)
    assert 2.0 ** -66 < m[1] < 2.0 ** -60 and 2.0 ** 44 < m[2] < 2.0 ** 50
    m = row_max('mag_channels', 1)
    assert 2.0 ** -66 < m[5] < 2.0 ** -60 and 2.0 ** 44 < m[0] < 2.0 ** 50
    assert sum(s[0] for s in R.PACK_CASES['head3'][0]) == 351 and R.PACK_CASES['head3'][1] == 352


def _forward_errors(x, w, b, act, k, stride, want):
    """rel_err of the restatement and of its two wrong variants against `want` [B,Ho,Wo,Cout] fp64."""
    out = []
    for kw in ({}, dict(drop_lh=True), dict(drop_block=(w.shape[1] // 32 - 1) // 2)):
        y = R.restate(x, w, k, k // 2, stride, **kw).double()
        if b is not None:
            y = y + b.double()
        out.append(rel_err(torch.tanh(y) if act == 'tanh' else y, want))
    return out


@pytest.mark.parametrize('name', list(R.CASES))
def test_the_restatement_meets_the_bar_and_the_wrong_ones_miss_it(name):
    op, xs, layers, stride = R.CASES[name]
    x, params, gys = R.inputs(name)
    o64, o32 = R.oracle(name, torch.float64), R.oracle(name, torch.float32)
    for i, ((w, b), (_, _, act)) in enumerate(zip(params, layers)):
        q = 'y%d' % i
        bar = R.bar(o32[q], o64[q])
        right, no_lh, no_block = _forward_errors(x, w, b, act, w.shape[2], stride, o64[q])
        print('%s %s: bar %.3e, restatement %.3e, without lh %.3e, without a block %.3e' % (name, q, bar, right, no_lh, no_block))
        assert right <= bar < no_lh and bar < no_block
    # dx of the stride-1 cases, as the forward convolution the backward launches (the pre-activation gradient: the cases without an
    # activation, whose g is gy itself)
    if stride == 1 and all(act is None for _, _, act in layers) and len(layers) == 1:
        g, wt, pad = R.dgrad_as_forward(gys[0], params[0][0], params[0][0].shape[2] // 2)
        bar = R.bar(o32['dx'], o64['dx'])
        errs = [rel_err(R.restate(g, wt, wt.shape[2], pad, 1, **kw).double(), o64['dx'])
                for kw in ({}, dict(drop_lh=True), dict(drop_block=0))]
        print('%s dx: bar %.3e, restatement %.3e, without lh %.3e, without a block %.3e' % ((name, bar) + tuple(errs)))
        assert errs[0] <= bar < errs[1] and bar < errs[2]


@pytest.mark.parametrize('kind', R.RANGE)
def test_the_restatement_is_within_the_elementwise_bound_and_the_wrong_ones_are_not(kind):
    x, w, gy = R.range_inputs(kind)
    k = w.shape[2]
    for what, (a, f, pad) in (('y', (x, w, k // 2)), ('dx', R.dgrad_as_forward(gy, w, k // 2))):
        want = R.conv64(a, f, None, pad, 1)
        E = R.error_bound(a, f, k, pad, 1)
        assert bool(torch.isfinite(want).all()) and bool((E > 0).all()) and float(want.abs().max()) > 2.0 ** -126
        over = lambda got: float(((got.double() - want).abs() / E).max())
        right, no_lh, no_block = (over(R.restate(a, f, k, pad, 1, **kw)) for kw in ({}, dict(drop_lh=True), dict(drop_block=0)))
        print('%s %s: largest |error| / E: restatement %.3e, without lh %.3e, without a block %.3e' % (kind, what, right, no_lh, no_block))
        assert right <= 1.0 < no_lh and 1.0 < no_block


def test_the_exact_answers_of_the_restatement():
    gen = torch.Generator().manual_seed(5)
    x = torch.randint(-8, 9, (2, 5, 7, 64), generator=gen).float()
    w = torch.randint(-8, 9, (40, 64, 3, 3), generator=gen).float()
    want = R.conv64(x, w, None, 1, 1)
    got = R.restate(x, w, 3, 1, 1)
    assert torch.equal(got.double(), want) and float(want.abs().max()) < 2.0 ** 24
    x, w = R.inputs('act_tanh')[0], R.inputs('act_tanh')[1][0][0]
    assert torch.equal(R.restate(x * 128, w, 3, 1, 1), R.restate(x, w, 3, 1, 1) * 128)
    assert bool(R.restate(torch.zeros_like(x), w, 3, 1, 1).view(torch.int32).eq(0).all())
    xi = x.clone()
    xi[1, 2, 3, 7] = float('inf')
    y = R.restate(xi, w, 3, 1, 1)
    reads = R.conv64((xi == float('inf')).float(), torch.ones_like(w), None, 1, 1) > 0
    assert not bool(torch.isfinite(y[reads]).any()) and int(reads.sum()) == 9 * 40
