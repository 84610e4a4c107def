"""The references of tests/entry_ref.py, pinned on the CPU before tests/test_gpu_entry_kat.py and tests/test_gpu_layout_kat.py hold
csrc/stem.hip, csrc/layout.hip and csrc/preprocess.hip to them:
  * stem_fp64 (written out tap by tap) equals torch.nn's Conv2d -> BatchNorm2d(eval) -> ReLU -> MaxPool2d in float64 to 1e-12 on
    every stem case, and each wrong= variant is at least 100 x the GPU bar away from it on the outputs it concerns;
  * every stem case meets the condition its name states, computed from the constants of csrc/stem.hip: tile counts, ragged
    remainders, all-zero patches next to loud ones, the persistent loop's trip counts, the unclamped range of ymi_h2_scale;
  * the fp32 restatements: max-pool and the layout changes equal torch exactly, the bilinear passes agree with F.interpolate to the
    distance tests/test_mask_kat_host.py allows, fast_base_transform agrees with oracle.yolact_oracle.fast_base_transform (which
    tests/test_fast_base_transform.py pins to tests/golden/fbt.npz) within that file's 1e-4 bar.
"""
import os
import re
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as TF

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'oracle'))
import entry_ref as R  # noqa: E402
import mask_ref as MR  # noqa: E402
from test_mask_kat_host import INTERP_BAR  # noqa: E402

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, 'yolact_amd', 'csrc', 'stem.hip')).read()


def _const(name):
    m = re.search(r'\b%s = (\d+)' % name, SRC)
    assert m, name
    return int(m.group(1))


PH, PW = _const('PH'), _const('PW')
IH, IW = 2 * (2 * PH + 1) + 5, 2 * (2 * PW + 1) + 5
_REF = {}


def _ref(name):
    if name not in _REF:
        c = R.stem_case(name)
        _REF[name] = (c, R.stem_fp64(c['x'], c['w'], c['bn']))
    return _REF[name]


def _geometry(H, W):
    Hs, Ws = R.out_size(H, 7, 2, 3), R.out_size(W, 7, 2, 3)
    Hp, Wp = R.out_size(Hs, 3, 2, 1), R.out_size(Ws, 3, 2, 1)
    return Hs, Ws, Hp, Wp, -(-Hp // PH), -(-Wp // PW)


def _patch_maxima(x):
    """max |x| of every tile's IH x IW patch (zero outside the image) -> [B, tiles_y, tiles_x]."""
    B, _, H, W = x.shape
    *_, ty, tx = _geometry(H, W)
    a = x.abs().amax(1)
    out = torch.zeros(B, ty, tx)
    for i in range(ty):
        for j in range(tx):
            r0, c0 = 4 * i * PH - 5, 4 * j * PW - 5
            p = a[:, max(r0, 0):max(min(r0 + IH, H), 0), max(c0, 0):max(min(c0 + IW, W), 0)]
            out[:, i, j] = p.reshape(B, -1).amax(1) if p.numel() else 0
    return out


@pytest.mark.parametrize('name', list(R.STEM_CASES))
def test_stem_oracle_equals_torch_nn_in_float64(name):
    c, ref = _ref(name)
    gamma, beta, mean, var = c['bn']
    conv = nn.Conv2d(3, 64, 7, 2, 3, bias=False).double()
    bn = nn.BatchNorm2d(64, eps=R.BN_EPS).double().eval()
    with torch.no_grad():
        conv.weight.copy_(c['w'].double())
        bn.weight.copy_(gamma.double()); bn.bias.copy_(beta.double())
        bn.running_mean.copy_(mean.double()); bn.running_var.copy_(var.double())
        want = nn.MaxPool2d(3, 2, 1)(torch.relu(bn(conv(c['x'].double())))).permute(0, 2, 3, 1)
    assert ref.shape == want.shape and ref.dtype == torch.float64
    d = (ref - want).abs().max().item() / max(want.abs().max().item(), 1e-300)
    assert d <= 1e-12, d


@pytest.mark.parametrize('name', list(R.STEM_CASES))
def test_wrong_oracles_are_far_from_the_oracle(name):
    c, ref = _ref(name)
    den = ref.abs().max().item()
    for v in R.WRONG:
        if not R.wrong_applies(c, v):
            assert torch.equal(R.stem_fp64(c['x'], c['w'], c['bn'], wrong=v), ref)       # the variant changes nothing here
            continue
        bad = R.stem_fp64(c['x'], c['w'], c['bn'], wrong=v)
        m = R.wrong_region(ref, v)
        d = (bad - ref)[m].abs().max().item() / den
        print('%s %s: %.2e of max|ref| on the outputs it concerns' % (name, v, d))
        assert d >= 100 * R.STEM_BAR, (name, v, d)
        if v != 'taps_transposed':
            assert torch.equal(bad[~m], ref[~m])         # and only there


def test_stem_cases_meet_what_their_names_state():
    seen = set()
    for name, (kind, B, H, W) in R.STEM_CASES.items():
        Hs, Ws, Hp, Wp, ty, tx = _geometry(H, W)
        if name.startswith('ragged'):
            assert H < 100 and W < 100 and Hp % PH and Wp % PW
            seen.add((Hp % PH, Wp % PW, H % 2, W % 2))
    assert {s[:2] for s in seen} == {(a, b) for a in range(1, PH) for b in range(1, PW)}
    assert {s[2] for s in seen} == {0, 1} and {s[3] for s in seen} == {0, 1}
    assert _geometry(7, 7)[2:] == (2, 2, 1, 1)                         # one tile, every pixel at a border
    # persistent loop: 169 tiles an image; some blocks run three tiles and some four
    assert _geometry(200, 300)[4:] == (13, 13)
    for cus in (R.CUS_DEFAULT, 304, 228):
        nt = 169 * R.persistent_B(cus)
        assert 3 * cus + 1 <= nt < 4 * cus and nt % cus != 0
    x = R.stem_case('persistent_200x300')['x']
    assert all(not torch.equal(x[a], x[b]) for a in range(x.shape[0]) for b in range(a))


def test_zero_cases_have_all_zero_patches_next_to_loud_ones():
    c = R.stem_case('zero_image_between_loud')
    pm = _patch_maxima(c['x'])
    assert (pm[1] == 0).all() and (pm[0] > 100).all() and (pm[2] > 100).all()
    c = R.stem_case('zero_region_in_loud')
    pm = _patch_maxima(c['x'])[0]
    zero = pm == 0
    assert zero[1, 1] and zero[2, 1] and int(zero.sum()) == 2, zero   # tiles (1, 1) and (2, 1): rows 11 .. 49, columns 19 .. 49
    assert (pm[~zero] > 100).all()                                   # its neighbours are loud
    # the pooled pixels whose receptive field is all zero (zero_field) exist and are exactly ReLU(bias) in the oracle
    m = R.zero_field(c['x'])
    assert int(m.sum()) >= 16
    ref = _ref('zero_region_in_loud')[1]
    want = torch.relu(R.folded_bias(c['bn']).double())
    assert (ref[m] - want).abs().max().item() < 1e-6


def test_negative_bias_case_is_zero_everywhere():
    c, ref = _ref('negative_bias')
    assert (ref == 0).all()
    # and by a wide margin: the largest pre-activation value stays below -900
    gamma, beta, mean, var = c['bn']
    t = TF.conv2d(c['x'].double(), c['w'].double(), None, 2, 3) * (gamma.double() / torch.sqrt(var.double() + R.BN_EPS)).view(1, -1, 1, 1)
    assert t.abs().max().item() < 100 and R.folded_bias(c['bn']).max().item() == -1000.0


def test_scale_invariance_case_stays_inside_the_unclamped_scale_range():
    """ymi_h2_scale clamps its exponent outside [2^-112, 2^127): there the scale no longer follows the patch.  Every patch maximum
    of the case, scaled by 2^-100 and by 2^100, stays inside; the folded bias is exactly 0."""
    c = R.stem_case('scale_invariance')
    assert (R.folded_bias(c['bn']) == 0).all()
    pm = _patch_maxima(c['x']).double()
    assert (pm > 0).all()
    for e in R.SCALE_EXPONENTS:
        s = pm * 2.0 ** e
        assert (s >= 2.0 ** -112).all() and (s < 2.0 ** 127).all(), e
        xs = c['x'] * 2.0 ** e
        assert torch.equal(xs.double(), c['x'].double() * 2.0 ** e)            # the scaling itself is exact in fp32


# ---- restatements --------------------------------------------------------------------------------------------------------------

def test_up_coord_with_the_derived_scale_is_mask_refs():
    for n_out, n_in in ((26, 13), (30, 13), (8, 21), (5, 1), (550, 16), (7, 7)):
        a, b = R.up_coord_scale(n_out, n_in, F(n_in) / F(n_out)), MR.up_coord(n_out, n_in)
        assert all(np.array_equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize('case', R.MAXPOOL_CASES)
def test_maxpool_restatement_equals_torch(case):
    B, H, W, Cc, kind = case
    if H > 100:
        H = W = 57
    x = R.layer_input(kind, (B, H, W, Cc), seed=H * 31 + W)
    want = TF.max_pool2d(torch.from_numpy(x).permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    assert R.same_bits(R.maxpool3x3s2(x), want)


def test_layout_and_global_max_restatements_equal_torch():
    for B, Cc, H, W in R.NHWC4_CASES[:4]:
        x = R.layer_input('randn', (B, Cc, H, W), seed=Cc)
        y = R.nchw_to_nhwc4(x)
        assert R.same_bits(y[..., :Cc], torch.from_numpy(x).permute(0, 2, 3, 1)) and (R.bits(y[..., Cc:]) == 0).all()
    for B, Cc, H, W in R.NCHW_CASES:
        x = R.layer_input('randn', (B, H, W, Cc), seed=Cc + H)
        assert R.same_bits(R.nhwc_to_nchw(x), torch.from_numpy(x).permute(0, 3, 1, 2))
    for B, HW, Cc, kind in R.GLOBAL_CASES:
        x = R.layer_input(kind, (B, HW, Cc), seed=HW + Cc)
        assert R.same_bits(R.global_max(x), torch.from_numpy(x).amax(1))


def test_amax_restatement():
    x = np.array([1.0, -3.5, np.nan, 2.0], F)
    assert R.amax(x) == F(3.5) and R.amax(np.full(4, -0.0, F)) == 0 and R.bits(np.array([R.amax(np.full(4, -0.0, F))], F))[0] == 0
    assert R.amax(np.full(4, np.nan, F)) == 0 and R.amax(np.array([1, np.inf, -2, 0], F)) == np.inf
    d = np.array([0, 1e-45, -3e-45, 0], F)
    assert R.amax(d) == F(3e-45) and R.amax(d) > 0


@pytest.mark.parametrize('case', R.BILINEAR_CASES)
def test_bilinear_restatement_agrees_with_interpolate(case):
    B, Hi, Wi, Cc, Ho, Wo, scale, relu = case
    x = R.bilinear_input(case)
    got = R.bilinear_nhwc(x, Ho, Wo, scale, scale, relu)
    t = torch.from_numpy(x).permute(0, 3, 1, 2)
    if scale is not None:
        assert (Ho, Wo) == (2 * Hi, 2 * Wi)
        want = TF.interpolate(t, scale_factor=2, mode='bilinear', align_corners=False)
    else:
        want = TF.interpolate(t, (Ho, Wo), mode='bilinear', align_corners=False)
    if relu:
        want = torch.relu(want)
    d = (torch.from_numpy(got).permute(0, 3, 1, 2) - want).abs().max().item()
    assert got.shape == (B, Ho, Wo, Cc) and d < INTERP_BAR, d
    if relu:
        assert (got >= 0).all()
    if (Ho, Wo) == (Hi, Wi):
        assert R.same_bits(got, np.where(x < 0, F(0), x) if relu else x)      # identity: weights 0, exact


@pytest.mark.parametrize('case', R.ADD_CASES)
def test_bilinear_add_restatement_agrees_with_interpolate(case):
    B, Hi, Wi, Cc, Ho, Wo = case
    x = R.layer_input('randn', (B, Hi, Wi, Cc), seed=1)
    y = R.layer_input('randn', (B, Ho, Wo, Cc), seed=2)
    want = torch.from_numpy(y) + TF.interpolate(torch.from_numpy(x).permute(0, 3, 1, 2), (Ho, Wo), mode='bilinear',
                                                align_corners=False).permute(0, 2, 3, 1)
    assert (torch.from_numpy(R.bilinear_add(x, y)) - want).abs().max().item() < INTERP_BAR


@pytest.mark.parametrize('case', R.FBT_CASES[:5])
def test_fbt_restatement_agrees_with_the_oracle(case):
    from oracle import yolact_oracle as O
    N, H, W, oh, ow = case
    img = R.fbt_input(case)
    for mode, tr in enumerate(('resnet', 'vgg', 'darknet', 'none')):
        cfg = types.SimpleNamespace(max_size=oh, preserve_aspect_ratio=False, backbone=types.SimpleNamespace(transform=tr))
        want = O.fast_base_transform(torch.from_numpy(img), cfg)               # (square target: the oracle's size rule)
        got = R.fast_base_transform(img, oh, oh, mode, False)
        assert got.shape == tuple(want.shape)
        d = np.abs(got - want.numpy()).max()
        assert d <= 1e-4 * max(1.0, want.abs().max().item()), (mode, d)
        n4 = R.fast_base_transform(img, oh, oh, mode, True)
        assert R.same_bits(np.ascontiguousarray(n4[..., :3].transpose(0, 3, 1, 2)), got) and (R.bits(n4[..., 3]) == 0).all()


def test_fbt_restatement_on_the_golden_cases():
    """The cases of tests/test_fast_base_transform.py, whose oracle output is pinned to tests/golden/fbt.npz there."""
    from oracle import yolact_oracle as O
    from yolact_amd.config import CONFIGS
    from test_fast_base_transform import CASES, GOLD, synth_frame
    z = np.load(GOLD)
    for name, config, n, h, w, seed in CASES:
        cfg = CONFIGS[config].copy()
        img = synth_frame(n, h, w, seed)
        want = O.fast_base_transform(img, cfg)
        tr = cfg.backbone.transform
        mode = {'resnet': 0, 'vgg': 1, 'darknet': 2}[tr] if isinstance(tr, str) else (0 if tr.normalize else 1 if tr.subtract_means else 2)
        got = R.fast_base_transform(img.numpy(), cfg.max_size, cfg.max_size, mode, False)
        tol = 1e-4 * max(1.0, want.abs().max().item())
        assert np.abs(got - want.numpy()).max() <= tol, name
        assert got.shape == tuple(z[name + '_shape'])                    # and against the recorded reference values themselves
        assert np.abs(got.reshape(-1)[z[name + '_idx']] - z[name + '_val']).max() <= tol, name
