"""The restatements of tests/mask_ref.py, pinned on the CPU before tests/test_gpu_mask_kat.py holds csrc/mask.hip to them bit for bit:
  * the upsample restatement (both lerp orders, which are the same bits) is F.interpolate(bilinear, align_corners=False) to the
    project's 1e-5 absolute (tests/test_gpu_path.py), fp32 and fp64, up- and down-sampling, 1-pixel sources, 138 -> 550;
  * the crop window and boxes_to_pixels restatements equal oracle.yolact_oracle.crop / postprocess exactly on hand-made boxes;
  * the bit packing restatement on a hand-checked case;
  * ymi_mask_upsample_kernel (the launcher's own choice, exported) names the kernel of every shipped launch: 138x138 -> 550x550
    with 100 masks per image is the band kernel at batch 1, rows16 at batch 2, rows32 at batch 4 and 8.
"""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_ref as MR  # noqa: E402

F = np.float32
INTERP_BAR = 1e-5            # absolute, masks in [0, 1]: the bar tests/test_gpu_path.py holds the soft masks to

# (ph, pw, h, w): up, down, mixed, 1-pixel sources and targets, the shipped 138 -> 550
SIZES = [(13, 11, 37, 67), (9, 12, 70, 65), (100, 90, 30, 64), (51, 20, 17, 221), (1, 1, 5, 7), (1, 9, 4, 3), (7, 1, 3, 20),
         (5, 7, 1, 1), (5, 7, 3, 2049), (138, 138, 97, 131), (138, 138, 550, 550)]


def coord_bound(ph, pw):
    """How far fp32 source coordinates can move a value of a {0,1} map from its fp64 value.  src = fl(fl(scale * (dst + 0.5)) - 0.5)
    with scale = fl(n_in / n_out): the scale's rounding, the product's and the difference's are each <= 2^-24 * n_in (src < n_in), so
    a coordinate is off by <= 3 * 2^-24 * n_in; a lerp weight moves a value by at most that times the difference of the two
    neighbours (1 on a {0,1} map), on both axes; plus the four value roundings of the lerps.  138 x 138: 4.96e-5, above the 1e-5
    the project holds smooth masks to, and true of every fp32 evaluation, torch's own included."""
    return 3 * 2.0 ** -24 * (ph + pw) + 4 * 2.0 ** -24


@pytest.mark.parametrize('ph,pw,h,w', SIZES)
def test_both_lerp_orders_are_the_same_bits_and_equal_torch_bilinear(ph, pw, h, w):
    """Bars: uniform and ulp inputs INTERP_BAR against F.interpolate in fp32 and in fp64.  The {0,1} maps, whose neighbours differ by 1,
    show the rounding of the fp32 coordinates undamped: coord_bound against fp64, twice that against torch's fp32 (two fp32
    evaluations).  Measured, 138x138 -> 550x550: uniform 7.0e-6 (fp32) / 9.1e-6 (fp64), {0,1} 9.1e-6 / 1.21e-5, ulp 6.0e-8 / 6.0e-8;
    138x138 -> 97x131: uniform 1.8e-6 / 9.3e-6, {0,1} 2.2e-6 / 1.36e-5."""
    N = 3
    for kind in MR.UP_INPUTS:
        lo = MR.up_input(kind, N, ph, pw, seed=ph * 1000 + w)
        a, b = MR.upsample_lerp2(lo, h, w), MR.upsample_rows(lo, h, w)
        assert a.shape == (N, h, w) and a.tobytes() == b.tobytes()
        t = torch.from_numpy(lo)[None]
        d32 = np.abs(a - torch.nn.functional.interpolate(t, (h, w), mode='bilinear', align_corners=False)[0].numpy()).max()
        d64 = np.abs(a.astype(np.float64)
                     - torch.nn.functional.interpolate(t.double(), (h, w), mode='bilinear', align_corners=False)[0].numpy()).max()
        bar64 = coord_bound(ph, pw) if kind == 'edges' else INTERP_BAR
        bar32 = 2 * coord_bound(ph, pw) if kind == 'edges' else INTERP_BAR
        print('%dx%d -> %dx%d %-7s: restatement vs F.interpolate fp32 %.2e (bar %.2e), fp64 %.2e (bar %.2e)'
              % (ph, pw, h, w, kind, d32, bar32, d64, bar64))
        assert d32 < bar32 and d64 < bar64


def test_restatement_makes_torch_decisions_on_uniform_inputs():
    """> 0.5 on the restatement and on F.interpolate may differ only where the value is within the bar of 0.5 (7.8 M pixels)."""
    lo = MR.up_input('uniform', 26, 138, 138, seed=5)
    a = MR.upsample_rows(lo, 550, 550)
    ref = torch.nn.functional.interpolate(torch.from_numpy(lo)[None], (550, 550), mode='bilinear', align_corners=False)[0].numpy()
    bad = (a > F(0.5)) != (ref > F(0.5))
    print('decisions that differ: %d of %d' % (bad.sum(), bad.size))
    assert bad.sum() == 0 or np.abs(a[bad] - F(0.5)).max() < INTERP_BAR


def _wrong_upsample(lo, h, w, variant):
    """The restatement with one deliberate change."""
    _, ph, pw = lo.shape
    if variant == 'scale as h / ph, then a division':
        def coord(n_out, n_in):
            inv = F(n_out) / F(n_in)
            src = (np.arange(n_out, dtype=np.int32).astype(F) + F(0.5)) / inv - F(0.5)
            src = np.where(src < 0, F(0), src)
            i0 = np.minimum(src.astype(np.int32), n_in - 1)
            return i0, i0 + (i0 < n_in - 1), src - i0.astype(F)
    elif variant == 'coordinates in fp64, rounded once':
        def coord(n_out, n_in):
            src = np.maximum(n_in / n_out * (np.arange(n_out) + 0.5) - 0.5, 0)
            i0 = np.minimum(src.astype(np.int32), n_in - 1)
            return i0, i0 + (i0 < n_in - 1), (src - i0).astype(F)
    else:
        coord = MR.up_coord
    y0, y1, ly = coord(h, ph)
    x0, x1, lx = coord(w, pw)
    ly, lx = ly[None, :, None], lx[None, None, :]
    v00, v01, v10, v11 = lo[:, y0][:, :, x0], lo[:, y0][:, :, x1], lo[:, y1][:, :, x0], lo[:, y1][:, :, x1]
    if variant == 'lerp as a + l * (b - a)':
        top, bot = v00 + lx * (v01 - v00), v10 + lx * (v11 - v10)
        return top + ly * (bot - top)
    if variant == 'vertical lerp first':
        left, right = (F(1) - ly) * v00 + ly * v10, (F(1) - ly) * v01 + ly * v11
        return (F(1) - lx) * left + lx * right
    if variant == 'products contracted into fused multiply-adds':
        fma = lambda a, b, c: (a.astype(np.float64) * b + c).astype(F)          # exact product (48 bits), one rounding (to 1 double ulp)
        top, bot = fma(lx + 0 * v01, v01, (F(1) - lx) * v00), fma(lx + 0 * v11, v11, (F(1) - lx) * v10)
        return fma(ly + 0 * bot, bot, (F(1) - ly) * top)
    return (F(1) - ly) * ((F(1) - lx) * v00 + lx * v01) + ly * ((F(1) - lx) * v10 + lx * v11)


@pytest.mark.parametrize('variant', ['scale as h / ph, then a division', 'coordinates in fp64, rounded once', 'lerp as a + l * (b - a)',
                                     'vertical lerp first', 'products contracted into fused multiply-adds'])
def test_bit_comparison_rejects_near_misses(variant):
    """The GPU tests can fail: on the first two shapes of their table the soft bits of the uniform input tell the restatement from
    an upsample that is the same function to rounding (another scale, another association, contraction), and a change to the
    lerps also flips 0.5 decisions of the input one ulp from the threshold (whose neighbours are too close for a moved
    coordinate to show)."""
    for ph, pw, h, w in SIZES[:2]:
        for kind in MR.UP_INPUTS:
            lo = MR.up_input(kind, 8, ph, pw, seed=3)
            want, wrong = MR.upsample_lerp2(lo, h, w), _wrong_upsample(lo, h, w, variant)
            assert np.abs(want - wrong).max() < INTERP_BAR                       # a tolerance would let it through
            n_soft, n_hard = (want != wrong).sum(), ((want > F(0.5)) != (wrong > F(0.5))).sum()
            print('%s, %dx%d -> %dx%d %s: %d soft values differ, %d decisions' % (variant, ph, pw, h, w, kind, n_soft, n_hard))
            if kind == 'uniform':
                assert n_soft > 0
            if 'lerp' in variant or 'fused' in variant:
                assert n_soft > 0 and (n_hard > 0 or kind != 'ulp')
    assert np.array_equal(_wrong_upsample(lo, h, w, None), want)               # the scaffold itself is the restatement


def test_up_coord_by_hand():
    """138 -> 550 and 3 -> 2 against values worked out by hand in exact arithmetic (where fp32 is exact)."""
    i0, i1, l1 = MR.up_coord(2, 3)                 # scale 1.5: src = 0.25, 1.75
    assert i0.tolist() == [0, 1] and i1.tolist() == [1, 2] and l1.tolist() == [0.25, 0.75]
    i0, i1, l1 = MR.up_coord(8, 2)                 # scale 0.25: src = max(-0.375, 0), ..., 1.375 -> clamped to the last pixel
    assert i0.tolist() == [0, 0, 0, 0, 0, 0, 1, 1] and i1.tolist() == [1, 1, 1, 1, 1, 1, 1, 1]
    assert l1.tolist() == [0.0, 0.0, 0.125, 0.375, 0.625, 0.875, 0.125, 0.375]
    i0, i1, l1 = MR.up_coord(5, 1)
    assert i0.tolist() == [0] * 5 and i1.tolist() == [0] * 5


def test_pack_bits_by_hand():
    hard = np.zeros((2, 70), bool)
    hard[0, [0, 3, 63, 64, 69]] = True
    hard[1, :] = True
    got = MR.pack_bits(hard)
    assert got.dtype == np.uint64 and got.shape == (2, 2)
    assert got[0].tolist() == [(1 << 0) | (1 << 3) | (1 << 63), (1 << 0) | (1 << 5)]
    assert got[1].tolist() == [(1 << 64) - 1, (1 << 6) - 1]                       # tail bits zero


@pytest.mark.parametrize('ph,pw', [(5, 7), (12, 11), (138, 138), (9, 15), (30, 64)])
def test_crop_window_equals_the_oracle(ph, pw):
    from oracle import yolact_oracle as O
    box = np.concatenate([MR.hand_boxes(pw, ph), MR.boxes_for(40, pw, ph, seed=ph)])
    want = O.crop(torch.ones(ph, pw, box.shape[0]), torch.from_numpy(box)).permute(2, 0, 1).numpy() != 0
    got = MR.crop_window(box, ph, pw)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert MR.crop_window(box, ph, pw, crop=False).all()
    # the hand-made set does what it is there for: empty windows, full windows, and windows that differ from the unreversed box's
    area = got[:len(MR.hand_boxes(pw, ph))].reshape(len(MR.hand_boxes(pw, ph)), -1).sum(1)
    assert area.min() == 0 and area.max() == ph * pw and np.array_equal(got[0], got[1])


@pytest.mark.parametrize('w,h', [(550, 550), (320, 240), (7, 5), (64, 33), (1, 1)])
def test_boxes_to_pixels_equals_the_oracle(w, h):
    """oracle postprocess() with the mask branch off returns exactly the boxes it returns with it on (sanitize, stack, .long())."""
    from oracle import yolact_oracle as O
    box = np.concatenate([MR.hand_boxes(w, h), MR.boxes_for(65, w, h, seed=w)])
    n = box.shape[0]
    det = {'class': torch.zeros(n, dtype=torch.int64), 'box': torch.from_numpy(box), 'score': torch.ones(n),
           'mask': torch.zeros(n, 32), 'proto': None}
    _, _, want, _ = O.postprocess(det, w, h, types.SimpleNamespace(eval_mask_branch=False))
    got = MR.boxes_to_pixels(box, w, h)
    assert want.dtype == torch.int64 and got.dtype == np.int64 and np.array_equal(got, want.numpy())
    assert got[:, 0].min() >= 0 and got[:, 1].min() >= 0 and got[:, 2].max() <= w and got[:, 3].max() <= h     # each clamped on ONE side


def test_logit_statements_agree():
    g = torch.Generator().manual_seed(1)
    proto, coef = torch.randn(9, 15, 32, generator=g), torch.randn(33, 32, generator=g)
    a, b = MR.masks_lo_torch(proto, coef, torch.float64), MR.masks_lo_torch(proto, coef, torch.float32)
    assert a.shape == (33, 9, 15) and (a - b.double()).abs().max().item() < 1e-6
    assert (torch.sigmoid(MR.logits64(proto, coef)) - a).abs().max().item() < 1e-15
    assert abs(a[5, 2, 3].item() - 1 / (1 + np.exp(-float(proto[2, 3].double() @ coef[5].double())))) < 1e-15


# ---- the exported kernel choice ----------------------------------------------------------------------------------------------------

def test_query_is_exported_and_bound_at_abi_9():
    from yolact_amd import _lib as L
    lib = L.lib()
    assert lib.ymi_abi_version() == 9 and L.ABI_VERSION == 9
    assert any(name == 'ymi_mask_upsample_kernel' for name, _, _ in L.SYMBOLS)
    assert (L.UP_FLAT, L.UP_BAND, L.UP_ROWS16, L.UP_ROWS32) == (1, 2, 3, 4)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'yolact_amd.h')).read()
    assert 'enum { YMI_UP_FLAT = 1, YMI_UP_BAND = 2, YMI_UP_ROWS16 = 3, YMI_UP_ROWS32 = 4 };' in hdr


def test_shipped_launches_run_the_kernels_the_plan_names():
    from yolact_amd import _lib as L
    q = L.lib().ymi_mask_upsample_kernel
    want = {1: L.UP_BAND, 2: L.UP_ROWS16, 4: L.UP_ROWS32, 8: L.UP_ROWS32}
    for B, k in want.items():
        for has_count in (0, 1):
            got = q(100 * B, 138, 138, 550, 550, 1 << 20, has_count)
            print('138x138 -> 550x550, batch %d (count %d): %s' % (B, has_count, L.UP_NAMES.get(got, got)))
            assert got == k


def test_query_conditions_and_rejections():
    """Either side of every condition of the launcher, and the codes the calls return instead of launching."""
    from yolact_amd import _lib as L
    q = L.lib().ymi_mask_upsample_kernel
    A = 1 << 20
    assert q(2560, 9, 12, 33, 64, A, 0) == L.UP_ROWS32 and q(2559, 9, 12, 33, 64, A, 0) == L.UP_ROWS16      # 2 * 2560 = 5120
    assert q(2048, 51, 20, 17, 220, A, 0) == L.UP_ROWS16 and q(2047, 51, 20, 17, 220, A, 0) == L.UP_BAND    # 2 * 2048 = 4096
    assert q(2048, 51, 20, 17, 221, A, 0) == L.UP_BAND                                                      # 49 164 B of LDS > 48 KB
    assert q(1400, 9, 12, 37, 64, A, 0) == L.UP_ROWS16 and q(1400, 9, 12, 37, 63, A, 0) == L.UP_BAND        # w >= 64
    assert q(1400, 13, 11, 37, 67, A + 16, 0) == L.UP_ROWS16 and q(1400, 13, 11, 37, 67, A + 4, 0) == L.UP_FLAT   # 16-byte alignment
    assert q(2, 5, 7, 3, 2047, A, 0) == L.UP_BAND and q(2, 5, 7, 3, 2048, A, 0) == L.UP_FLAT                # a band of 8 rows in 64 KB
    assert q(65535, 5, 7, 3, 64, A, 0) == L.UP_ROWS32 and q(65536, 5, 7, 3, 64, A, 0) == L.UP_FLAT          # grid.y
    assert q(2, 5, 7, 3, 2048, A, 1) == -2 and q(2, 5, 7, 3, 64, A + 4, 1) == -2                            # a count needs band / rows
    assert q(65536, 5, 7, 3, 64, A, 1) == -1
    for bad in ((0, 5, 7, 3, 64), (1, 0, 7, 3, 64), (1, 5, -1, 3, 64), (1, 5, 7, 0, 64), (1, 5, 7, 3, 0)):
        assert q(*bad, A, 0) == -1
    assert q(1, 5, 7, 3, 64, 0, 0) == -3


def test_calls_reject_bad_arguments_without_a_gpu():
    """Validation returns before any launch (pointers nothing may touch)."""
    import ctypes as C
    from yolact_amd import _lib as L
    lib, P, thr = L.lib(), 16, C.c_float(0.5)
    assert lib.ymi_lincomb_crop_f32(P, P, P, P, 5, 7, 32, 1025, 1, None) == -1
    assert lib.ymi_lincomb_crop_f32(P, P, P, P, 5, 7, 32, 0, 1, None) == -1
    assert lib.ymi_lincomb_crop_f32(P, P, P, P, 5, 7, 16, 4, 1, None) == -2
    assert lib.ymi_lincomb_crop_batch_f32(P, P, P, P, P, 3, 1025, 5, 7, 32, 1, None) == -1
    assert lib.ymi_lincomb_crop_batch_f32(P, P, P, P, P, 3, 40, 5, 7, 16, 1, None) == -2
    for k in range(4):
        a = [P] * 4
        a[k] = None
        assert lib.ymi_lincomb_crop_f32(*a, 5, 7, 32, 4, 1, None) == -3
        b = a[:3] + [P] + a[3:]                                                   # count may be null, the other four may not
        assert lib.ymi_lincomb_crop_batch_f32(*b, 3, 40, 5, 7, 32, 1, None) == -3
    assert lib.ymi_mask_upsample_batch_f32(P, P, P, 3, 21846, 5, 7, 3, 64, thr, None) == -1       # B * cap = 65538
    assert lib.ymi_mask_upsample_batch_f32(P, P, P, 3, 8, 5, 7, 3, 2048, thr, None) == -2         # a count and the flat kernel
    assert lib.ymi_mask_upsample_batch_f32(None, P, P, 3, 8, 5, 7, 3, 64, thr, None) == -3
    assert lib.ymi_mask_upsample_f32(P, None, 3, 5, 7, 3, 64, thr, None) == -3
    assert lib.ymi_mask_upsample_f32(P, P, 0, 5, 7, 3, 64, thr, None) == -1
    assert lib.ymi_boxes_to_pixels(None, P, 1, 7, 5, None) == -3 and lib.ymi_boxes_to_pixels(P, P, 0, 7, 5, None) == -1
