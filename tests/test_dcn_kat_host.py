"""Known-answer tests for the DCNv2 forward, on the CPU.

tests/dcn_ref.py::dcn_ref (F.grid_sample in fp64, torch only) is pinned to closed-form answers (shifted_conv_ref: per-tap
integer shifts of the input and their dyadic bilinear combinations), and then the CPU oracle the GPU tests used to rely on alone
(oracle/yolact_oracle.py::dcn_v2_forward) is pinned to dcn_ref.  The known answers use a different (dh_k, dw_k) on every tap
with dh_k != dw_k, non-square maps, stride 1 and 2, and sample points exactly on the image edges; the last test shows that they
reject the errors an implementation and its own restatement could share (dh / dw swapped, offset sign, tap order, the bilinear
corners at the edges, the -1 < h < H gate).
"""
import pytest
import torch

from dcn_ref import (const_offmask, dcn_ref, edge_offsets, edge_taps, fp32_point_offsets, fractional_taps, integer_taps, out_hw,
                     shifted_conv_ref)

MASKS = (0.25, 1.0, 0.5, 0.0, 1.0, 0.75, 0.5, 1.0, 0.25)       # per-tap modulation (0 on tap 3: that tap contributes nothing)


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _kats():
    """(name, x, offset, mask, weight, bias, stride, expected) with closed-form expected values (fp64)."""
    out = []
    for stride in (1, 2):
        B, C, H, W, Co = 2, 5, 7, 11, 4
        g = _g(10 + stride)
        x = torch.randn(B, C, H, W, generator=g)
        w = torch.randn(Co, C, 3, 3, generator=g)
        b = torch.randn(Co, generator=g)
        Ho, Wo = out_hw(H, W, stride, 1)
        cases = [('integer', integer_taps(H, W)), ('fractional', fractional_taps())]
        cases += [('edge_lo%d' % q, edge_taps(H, W, stride, 1, True, q)) for q in range(4)]
        cases += [('edge_hi%d' % q, edge_taps(H, W, stride, 1, False, q)) for q in range(4)]
        for name, taps in cases:
            off, m = const_offmask(B, Ho, Wo, taps, MASKS)
            out.append(('%s/s%d' % (name, stride), x, off, m, w, b, stride, shifted_conv_ref(x, taps, w, b, stride, 1, MASKS)))
    return out


KATS = _kats()


def _err(a, b):
    return (a - b).abs().max().item() / b.abs().max().item()


@pytest.mark.parametrize('i', range(len(KATS)), ids=[k[0] for k in KATS])
def test_dcn_ref_equals_closed_form(i):
    name, x, off, m, w, b, stride, want = KATS[i]
    assert _err(dcn_ref(x, off, m, w, b, stride, 1), want) < 1e-12


def test_closed_form_builder_is_a_convolution_at_zero_offset():
    """shifted_conv_ref itself: zero offsets, unit masks == F.conv2d (fp64), stride 1 and 2."""
    g = _g(3)
    x, w, b = torch.randn(2, 5, 7, 11, generator=g), torch.randn(4, 5, 3, 3, generator=g), torch.randn(4, generator=g)
    for stride in (1, 2):
        want = torch.nn.functional.conv2d(x.double(), w.double(), b.double(), stride, 1)
        assert _err(shifted_conv_ref(x, [(0, 0)] * 9, w, b, stride, 1), want) < 1e-13


def _random_case(seed, B, C, H, W, Co, stride, spread):
    g = _g(seed)
    x, w, b = torch.randn(B, C, H, W, generator=g), torch.randn(Co, C, 3, 3, generator=g), torch.randn(Co, generator=g)
    Ho, Wo = out_hw(H, W, stride, 1)
    sgn = torch.where(torch.rand(B, 18, Ho, Wo, generator=g) < 0.5, -1.0, 1.0)
    off = sgn * (2 + 2 * torch.rand(B, 18, Ho, Wo, generator=g)) if spread is None else edge_offsets(B, H, W, stride, 1, g, spread)
    return x, off, torch.rand(B, 9, Ho, Wo, generator=g), w, b


@pytest.mark.parametrize('stride', [1, 2])
def test_oracle_equals_dcn_ref(stride):
    """oracle.yolact_oracle.dcn_v2_forward (its own restatement of the original kernel) == dcn_ref, fp64: on every known answer,
    on random offsets of 2 to 4 px, on per-pixel exact edge placements with batch 3, and on offsets of +-1000 and +-(H+W).
    The oracle forms sample points in fp64, dcn_ref in fp32 as the kernels do, so the oracle gets the offsets that give it the
    same points (fp32_point_offsets; an identity on every known answer, whose points are exact in fp32)."""
    from oracle.yolact_oracle import dcn_v2_forward
    H, W = 7, 11

    def orc(x, off, m, w, b, s):
        return dcn_v2_forward(x.double(), fp32_point_offsets(off, H, W, s, 1), m.double(), w.double(), b.double(), s, 1, 1)

    for name, x, off, m, w, b, s, want in KATS:
        if s == stride:
            assert torch.equal(fp32_point_offsets(off, H, W, s, 1), off.double())
            assert _err(orc(x, off, m, w, b, s), want) < 1e-12, name
    for seed, spread in ((1, None), (2, 1.5), (3, 3.0)):
        x, off, m, w, b = _random_case(seed * 10 + stride, 3, 5, H, W, 4, stride, spread)
        if seed == 3:
            off[0, :, 1, 1], off[1, ::2, 2, 2], off[2, 1::2, 0, 1] = 1000.3, -1000.7, float(H + W)
        assert _err(orc(x, off, m, w, b, stride), dcn_ref(x, off, m, w, b, stride, 1)) < 1e-12


def _taps_transposed(t, per):
    """Channels of tap k (groups of `per`) moved to tap (k % 3)*3 + k // 3."""
    B, _, Ho, Wo = t.shape
    perm = [(k % 3) * 3 + k // 3 for k in range(9)]
    return t.view(B, 9, per, Ho, Wo)[:, perm].reshape(B, 9 * per, Ho, Wo)


def _dh_dw_swapped(off):
    B, _, Ho, Wo = off.shape
    return off.view(B, 9, 2, Ho, Wo).flip(2).reshape(B, 18, Ho, Wo)


WRONG = {
    'dh / dw swapped': lambda x, o, m, w, b, s: dcn_ref(x, _dh_dw_swapped(o), m, w, b, s, 1),
    'offset sign flipped': lambda x, o, m, w, b, s: dcn_ref(x, -o, m, w, b, s, 1),
    'taps transposed (k = j*3 + i)': lambda x, o, m, w, b, s: dcn_ref(x, _taps_transposed(o, 2), _taps_transposed(m, 1), w, b, s, 1),
    "padding_mode='border'": lambda x, o, m, w, b, s: dcn_ref(x, o, m, w, b, s, 1, padding_mode='border'),
    'gate tightened to h, w >= 0': lambda x, o, m, w, b, s: dcn_ref(x, o, m, w, b, s, 1, gate_min=0.0),
    'align_corners=True': lambda x, o, m, w, b, s: dcn_ref(x, o, m, w, b, s, 1, align_corners=True),
}


@pytest.mark.parametrize('variant', sorted(WRONG))
def test_known_answers_reject_wrong_variant(variant):
    """The tests can fail: each deliberately wrong variant of dcn_ref is rejected by at least one known answer (and the known
    answers that reject it are reported)."""
    f = WRONG[variant]
    caught = [name for name, x, off, m, w, b, s, want in KATS if _err(f(x, off, m, w, b, s), want) > 1e-6]
    print('%s: rejected by %d of %d known answers (%s)' % (variant, len(caught), len(KATS), ', '.join(caught)))
    assert caught
