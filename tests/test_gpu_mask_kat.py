"""Known-answer tests of the mask assembly behind postprocess() / postprocess_batch(): csrc/mask.hip and mask_upsample_bits_k of
csrc/metrics.hip, at every launch the benchmarked path ships and at the sizes where each kernel takes another path.

Upsample: csrc/upsample_math.h is plain fp32 without contraction, so the numpy fp32 restatement of tests/mask_ref.py (pinned to
F.interpolate and to the oracle on the CPU by tests/test_mask_kat_host.py) gives the answer BIT FOR BIT: soft outputs are compared
as bits, hard outputs exactly, nothing is left out, for all four kernels (flat, band, rows16, rows32).  Which kernel ran is
asserted through ymi_mask_upsample_kernel, the launcher's own choice.  Outputs start 4 floats into a NaN-filled buffer (16-byte
but not 128-byte aligned: the rows kernel's 64-float segments then start off the cache lines) and the floats before and after
must stay NaN.

lincomb_crop_k: outside the crop window exact +0.0 bits and the window exactly the restatement's; inside
rel_err(gpu, fp64) <= max(4 * rel_err(fp32 on the CPU, fp64), EXACT_BAR = 8e-6), the project's bar (tests/test_gpu_mask_loss.py).
Measured on the MI355X: 1.1e-7 to 9.9e-7 against a bar of 8e-6 (test_lincomb_crop's docstring has the table).
"""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_ref as MR  # noqa: E402
from yolact_amd import _lib as L  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EXACT_BAR = 8e-6
F = np.float32
NAN = float('nan')

# (name, ph, pw, h, w, nmask, kernel): the smallest shapes that meet each condition of the launcher (csrc/mask.hip choose_upsample)
UP_CASES = [
    ('rows16 odd sizes, last band 5 rows', 13, 11, 37, 67, 1400, 'rows16'),
    ('rows32, last band 6 rows, segments straddle rows', 9, 12, 70, 65, 1710, 'rows32'),
    ('rows32 at the 5120 threshold, w == 64, one-row last band', 9, 12, 33, 64, 2560, 'rows32'),
    ('rows16 downsampling, ns near ns_max', 100, 90, 30, 64, 2100, 'rows16'),
    ('rows16 under the 48 KB of LDS, 4096 bands', 51, 20, 17, 220, 2048, 'rows16'),
    ('band: rows over the 48 KB of LDS', 51, 20, 17, 221, 2048, 'band'),
    ('band: rows refused, w < 64', 9, 12, 37, 63, 1400, 'band'),
    ('band 97x131', 138, 138, 97, 131, 7, 'band'),
    ('band 33x1', 138, 138, 33, 1, 7, 'band'),
    ('band 5x1023', 138, 138, 5, 1023, 7, 'band'),
    ('band, largest LDS (65 520 B)', 5, 7, 3, 2047, 2, 'band'),
    ('flat by width', 5, 7, 3, 2048, 2, 'flat'),
    ('flat by width, total % 4 != 0', 5, 7, 3, 2049, 1, 'flat'),
]
KERNELS = {'flat': L.UP_FLAT, 'band': L.UP_BAND, 'rows16': L.UP_ROWS16, 'rows32': L.UP_ROWS32}

_REF = {}


def case_input(ci, kind):
    _, ph, pw, _, _, nmask, _ = UP_CASES[ci]
    return MR.up_input(kind, nmask, ph, pw, seed=100 * ci + MR.UP_INPUTS.index(kind))


def case_ref(ci, kind):
    """(lo, soft restatement) of a case; kept for the two cases the variants test runs again, computed once."""
    if (ci, kind) in _REF:
        return _REF[ci, kind]
    _, _, _, h, w, _, _ = UP_CASES[ci]
    lo = case_input(ci, kind)
    r = (lo, MR.upsample_rows(lo, h, w))
    if ci < 2:
        _REF[ci, kind] = r
    return r


def guarded(total, dtype=torch.float32, fill=NAN, tail=60):
    """-> (buffer, view of `total` elements starting 4 elements in).  float32: 16-byte but not 128-byte aligned."""
    buf = torch.full((4 + total + tail,), fill, dtype=dtype, device=DEV)
    out = buf[4:4 + total]
    if dtype == torch.float32:
        assert out.data_ptr() % 128 == 16
    return buf, out


def guards_intact(buf, total, fill=NAN):
    g = torch.cat([buf[:4], buf[4 + total:]])
    return bool(torch.isnan(g).all()) if buf.dtype.is_floating_point else bool((g == fill).all())


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32))


def run_upsample(lo, nmask, ph, pw, h, w, thresh, count=None, cap=None):
    """ymi_mask_upsample_f32 (count None) / ymi_mask_upsample_batch_f32 into a guarded buffer -> (numpy [nmask,h,w], kernel id)."""
    total = nmask * h * w
    buf, out = guarded(total)
    k = L.lib().ymi_mask_upsample_kernel(nmask, ph, pw, h, w, out.data_ptr(), 0 if count is None else 1)
    if count is None:
        L.check(L.lib().ymi_mask_upsample_f32(lo.data_ptr(), out.data_ptr(), nmask, ph, pw, h, w, C.c_float(thresh), L.stream_ptr()),
                'ymi_mask_upsample_f32')
    else:
        L.check(L.lib().ymi_mask_upsample_batch_f32(lo.data_ptr(), count.data_ptr(), out.data_ptr(), nmask // cap, cap, ph, pw, h, w,
                                                    C.c_float(thresh), L.stream_ptr()), 'ymi_mask_upsample_batch_f32')
    torch.cuda.synchronize()
    assert guards_intact(buf, total), 'wrote outside the output'
    return out.view(nmask, h, w).cpu().numpy(), k


# ---- upsample --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('ci', range(len(UP_CASES)), ids=['%dx%d-%dx%d-n%d-%s' % c[1:] for c in UP_CASES])
def test_upsample_is_the_restatement_bit_for_bit(ci):
    name, ph, pw, h, w, nmask, kernel = UP_CASES[ci]
    for kind in MR.UP_INPUTS:
        lo_np, want = case_ref(ci, kind)
        lo = torch.from_numpy(lo_np).to(DEV)
        for thresh in (-1.0, 0.5) + ((0.0,) if ci in (0, 1, 7) else ()):
            got, k = run_upsample(lo, nmask, ph, pw, h, w, thresh)
            if kind == MR.UP_INPUTS[0] and thresh < 0:
                print('%s: %dx%d -> %dx%d, %d masks: %s' % (name, ph, pw, h, w, nmask, L.UP_NAMES.get(k, k)))
            assert k == KERNELS[kernel], (name, L.UP_NAMES.get(k, k))
            ref = MR.binarise(want, thresh)
            if not bits_equal(got, ref):
                bad = np.argwhere(got.view(np.int32) != ref.view(np.int32))
                raise AssertionError('%s, %s, thresh %g: %d of %d values differ, first at (n, y, x) = %s: got %r, want %r'
                                     % (name, kind, thresh, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])],
                                        ref[tuple(bad[0])]))
        if kind == 'ulp':
            assert 0.02 < MR.binarise(want, 0.5).mean() < 0.98          # the threshold does decide on this input


def test_upsample_count_form_skips_rows_past_count():
    """B = 3, cap 456 (rows16 with a count), count = [cap, 0, 5]: rows < count exact.  The rows of masks_lo past count hold NaN (they
    must never be read); their outputs are unspecified and nothing is asserted about them.  Then the two rejections of the
    batch call: a count with a width only the flat kernel takes, and B * cap > 65535."""
    B, cap, ph, pw, h, w = 3, 456, 13, 11, 37, 67
    counts = [cap, 0, 5]
    lo_np = MR.up_input('uniform', B * cap, ph, pw, seed=77).reshape(B, cap, ph, pw)
    for b, c in enumerate(counts):
        lo_np[b, c:] = np.nan
    want = MR.upsample_rows(lo_np.reshape(B * cap, ph, pw), h, w).reshape(B, cap, h, w)
    lo = torch.from_numpy(lo_np).to(DEV)
    count = torch.tensor(counts, dtype=torch.int32, device=DEV)
    for thresh in (-1.0, 0.5):
        got, k = run_upsample(lo, B * cap, ph, pw, h, w, thresh, count=count, cap=cap)
        print('count form %dx%d -> %dx%d, B %d cap %d: %s' % (ph, pw, h, w, B, cap, L.UP_NAMES.get(k, k)))
        assert k == L.UP_ROWS16
        got = got.reshape(B, cap, h, w)
        for b, c in enumerate(counts):
            assert bits_equal(got[b, :c], MR.binarise(want[b, :c], thresh)), (b, thresh)
    buf, out = guarded(16)
    thr, s = C.c_float(0.5), L.stream_ptr()
    assert L.lib().ymi_mask_upsample_batch_f32(lo.data_ptr(), count.data_ptr(), out.data_ptr(), 3, 2, ph, pw, 3, 2048, thr, s) == -2
    assert L.lib().ymi_mask_upsample_batch_f32(lo.data_ptr(), count.data_ptr(), out.data_ptr(), 3, 21846, ph, pw, 3, 64, thr, s) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())


def test_upsample_shipped_batch8_launch():
    """138x138 -> 550x550, B = 8, cap 100, no count: rows32 with nontemporal stores, the launch that writes 968 MB per step.
    lo[n] = lo[n % 6]: every mask must equal the mask of its source bit for bit ON THE DEVICE (the segment offset `lead` differs
    per n), and out[:6] is the restatement."""
    nmask, ph, pw, h, w = 800, 138, 138, 550, 550
    six = np.concatenate([MR.up_input(kind, 2, ph, pw, seed=40 + i) for i, kind in enumerate(MR.UP_INPUTS)])
    want = MR.upsample_rows(six, h, w)
    lo = torch.from_numpy(six).to(DEV)[torch.arange(nmask, device=DEV) % 6].contiguous()
    total = nmask * h * w
    buf, out = guarded(total)
    q = L.lib().ymi_mask_upsample_kernel
    assert q(nmask, ph, pw, h, w, out.data_ptr(), 0) == L.UP_ROWS32 == q(nmask, ph, pw, h, w, out.data_ptr(), 1)
    print('138x138 -> 550x550, 800 masks: rows32')
    for thresh in (-1.0, 0.5):
        buf.fill_(NAN)
        L.check(L.lib().ymi_mask_upsample_batch_f32(lo.data_ptr(), None, out.data_ptr(), 8, 100, ph, pw, h, w, C.c_float(thresh),
                                                    L.stream_ptr()), 'ymi_mask_upsample_batch_f32')
        torch.cuda.synchronize()
        assert guards_intact(buf, total)
        o = out.view(nmask, h * w).view(torch.int32)
        for r in range(6):
            assert bool((o[r::6] == o[r]).all()), (thresh, r)
        assert bits_equal(out.view(nmask, h, w)[:6].cpu().numpy(), MR.binarise(want, thresh)), thresh


# Measured on the MI355X: the two shapes x three inputs x (soft, hard) with the .npy writes take 0.5 s in-process (CHILD_WORK_S); a
# child adds the interpreter, the torch import and the HIP start-up: 2.4 - 2.5 s from start to exit (CHILD_TOTAL_S), the same for
# all three settings.  The limit is 24x that: room for a cold import on a busy machine, still short of a hang's cost.
CHILD_WORK_S, CHILD_TOTAL_S, CHILD_TIMEOUT_S = 0.5, 2.5, 60
VARIANTS = [({'YOLACT_AMD_UPSAMPLE': 'rows'}, ('rows16', 'rows32')), ({'YOLACT_AMD_UPSAMPLE': 'band'}, ('band', 'band')),
            ({'YOLACT_AMD_UPSAMPLE_FLAT': '1'}, ('flat', 'flat'))]


def test_env_variants_write_the_same_bits(tmp_path):
    """YOLACT_AMD_UPSAMPLE=rows (plain stores), =band and YOLACT_AMD_UPSAMPLE_FLAT=1 are read once per process: one fresh child
    per setting, one after another, each under its own time limit; a child that does not exit 0 fails the test at once."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'mask_kat_child.py')
    base = {k: v for k, v in os.environ.items() if k not in ('YOLACT_AMD_UPSAMPLE', 'YOLACT_AMD_UPSAMPLE_FLAT')}
    for env, kernels in VARIANTS:
        out = tmp_path / '_'.join('%s=%s' % kv for kv in env.items())
        out.mkdir()
        t0 = time.time()
        r = subprocess.run([sys.executable, child, str(out)], env=dict(base, **env), timeout=CHILD_TIMEOUT_S, capture_output=True,
                           text=True)
        if r.returncode != 0:
            pytest.fail('child %s exited %d:\n%s' % (env, r.returncode, r.stderr[-2000:]))
        meta = json.load(open(out / 'meta.json'))
        print('%s: child %.1f s (work %.1f s, in-process total %.1f s), kernels %s'
              % (env, time.time() - t0, meta['seconds_work'], meta['seconds_total'], kernels))
        for ci in (0, 1):
            for kind in MR.UP_INPUTS:
                assert meta['%d_%s' % (ci, kind)] == KERNELS[kernels[ci]], (env, ci, meta)
                _, want = case_ref(ci, kind)
                assert bits_equal(np.load(out / ('soft_%d_%s.npy' % (ci, kind))), want), (env, ci, kind)
                hard = np.load(out / ('hard_%d_%s.npy' % (ci, kind)))
                assert hard.dtype == np.uint8 and np.array_equal(hard, (want > F(0.5)).astype(np.uint8)), (env, ci, kind)
        for f in out.iterdir():
            f.unlink()


def test_upsample_bits_are_the_packed_restatement():
    """13x11 -> 37x67, N = 3: h * w = 2479 is no multiple of 64; the words, tail bits included, over a buffer of all-ones."""
    N, ph, pw, h, w = 3, 13, 11, 37, 67
    W64 = (h * w + 63) // 64
    for i, kind in enumerate(MR.UP_INPUTS):
        lo_np = MR.up_input(kind, N, ph, pw, seed=60 + i)
        for thresh in (0.5, 0.0):
            want = MR.pack_bits((MR.upsample_lerp2(lo_np, h, w) > F(thresh)).reshape(N, -1))
            buf, bits = guarded(N * W64, torch.int64, -1, tail=8)
            lo = torch.from_numpy(lo_np).to(DEV)
            L.check(L.lib().ymi_mask_upsample_bits(lo.data_ptr(), N, ph, pw, h, w, C.c_float(thresh), bits.data_ptr(), L.stream_ptr()),
                    'ymi_mask_upsample_bits')
            torch.cuda.synchronize()
            assert guards_intact(buf, N * W64, -1)
            got = bits.view(N, W64).cpu().numpy().view(np.uint64)
            assert np.array_equal(got, want), (kind, thresh)
            assert int(got[0, -1]) >> (h * w - 64 * (W64 - 1)) == 0


# ---- lincomb + crop --------------------------------------------------------------------------------------------------------------

def rel_err(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300))


def lincomb_inputs(ph, pw, N, seed, logit_max=None):
    g = torch.Generator().manual_seed(seed)
    proto = torch.randn(ph, pw, 32, generator=g)
    coef = torch.randn(N, 32, generator=g) * 0.5
    if logit_max is not None:
        coef = (coef * (logit_max / MR.logits64(proto, coef).abs().max().item())).float()
    return proto, coef, MR.boxes_for(N, pw, ph, seed)


def check_lincomb(got, proto, coef, box, crop, label, logit_max=None):
    """got [N,ph,pw] numpy fp32 against the window (exact) and the logits (the project's bar) -> (err, bar)."""
    N, ph, pw = got.shape
    win = MR.crop_window(box, ph, pw, crop)
    assert np.array_equal(got.view(np.int32)[~win], np.zeros((~win).sum(), np.int32)), '%s: not +0.0 outside the window' % label
    assert np.isfinite(got).all() and got.min() >= 0 and got.max() <= 1
    s64 = MR.masks_lo_torch(proto, coef, torch.float64).numpy()
    assert (got[win & (s64 > 1e-30)] > 0).all(), '%s: zero inside the window' % label          # with the line above: the window, exactly
    r64 = s64 * win
    r32 = MR.masks_lo_torch(proto, coef, torch.float32).numpy().astype(np.float64) * win
    err, bar = rel_err(got.astype(np.float64), r64), max(4 * rel_err(r32, r64), EXACT_BAR)
    print('%s: rel_err gpu %.2e, fp32 on the CPU %.2e, bar %.2e' % (label, err, rel_err(r32, r64), bar))
    if logit_max is not None:
        z = MR.logits64(proto, coef).numpy()
        assert np.abs(z).max() >= 0.999 * logit_max
        assert (got[win & (z > 50)] == 1).all() and (got[win & (z < -50)] < 1e-20).all(), '%s: not saturated' % label
    assert err <= bar, (label, err, bar)
    return err, bar


LINCOMB_CASES = [(5, 7, 1, None), (12, 11, 32, None), (138, 138, 33, None), (9, 15, 1024, None), (12, 11, 32, 120.0)]


@pytest.mark.parametrize('ph,pw,N,logit_max', LINCOMB_CASES)
def test_lincomb_crop(ph, pw, N, logit_max):
    """Measured on the MI355X, rel_err(gpu, fp64) with crop 1 / crop 0 (fp32 on the CPU in brackets); the bar is EXACT_BAR = 8e-6
    in every case, 4x the CPU's fp32 error being smaller:
        5x7     N 1      1.10e-7 / 1.10e-7   (2.10e-7 / 2.10e-7)
        12x11   N 32     1.52e-7 / 2.42e-7   (1.94e-7 / 2.42e-7)
        138x138 N 33     3.14e-7 / 3.85e-7   (3.30e-7 / 3.36e-7)
        9x15    N 1024   3.27e-7 / 3.27e-7   (3.22e-7 / 3.22e-7)
        12x11   N 32, logits to +-120   7.18e-7 / 9.90e-7   (8.57e-7 / 1.06e-6)"""
    proto, coef, box = lincomb_inputs(ph, pw, N, seed=ph * 100 + N, logit_max=logit_max)
    pd, cd, bd = proto.to(DEV).contiguous(), coef.to(DEV).contiguous(), torch.from_numpy(box).to(DEV)
    for crop in (1, 0):
        buf, out = guarded(N * ph * pw)
        L.check(L.lib().ymi_lincomb_crop_f32(pd.data_ptr(), cd.data_ptr(), bd.data_ptr(), out.data_ptr(), ph, pw, 32, N, crop,
                                             L.stream_ptr()), 'ymi_lincomb_crop_f32')
        torch.cuda.synchronize()
        assert guards_intact(buf, N * ph * pw)
        check_lincomb(out.view(N, ph, pw).cpu().numpy(), proto, coef, box, crop,
                      'lincomb %dx%d N %d crop %d%s' % (ph, pw, N, crop, ' logits to +-%g' % logit_max if logit_max else ''), logit_max)


@pytest.mark.parametrize('counts', [[40, 0, 7], [55, 3, 0], None])
def test_lincomb_crop_batch_leaves_rows_past_count_untouched(counts):
    """B = 3, cap 40.  count[b] > cap clamps to cap; rows >= count keep the bits they had (NaN here): postprocess_bits_batch
    zero-fills masks_lo and relies on exactly this for its all-zero bit rows.  The coefficient and box rows past count hold NaN."""
    B, cap, ph, pw = 3, 40, 12, 11
    live = [cap] * B if counts is None else [min(c, cap) for c in counts]
    ins = [lincomb_inputs(ph, pw, cap, seed=900 + b) for b in range(B)]
    proto = torch.stack([i[0] for i in ins])
    coef = torch.stack([i[1] for i in ins])
    box = torch.stack([torch.from_numpy(i[2]) for i in ins])
    for b, c in enumerate(live):
        coef[b, c:], box[b, c:] = NAN, NAN
    pd, cd, bd = proto.to(DEV).contiguous(), coef.to(DEV).contiguous(), box.to(DEV).contiguous()
    count = None if counts is None else torch.tensor(counts, dtype=torch.int32, device=DEV)
    for crop in (1, 0):
        buf, out = guarded(B * cap * ph * pw)
        L.check(L.lib().ymi_lincomb_crop_batch_f32(pd.data_ptr(), cd.data_ptr(), bd.data_ptr(), count.data_ptr() if count is not None else None,
                                                   out.data_ptr(), B, cap, ph, pw, 32, crop, L.stream_ptr()), 'ymi_lincomb_crop_batch_f32')
        torch.cuda.synchronize()
        assert guards_intact(buf, B * cap * ph * pw)
        got = out.view(B, cap, ph, pw).cpu().numpy()
        nan_bits = torch.full((1,), NAN).numpy().view(np.int32)[0]
        for b, c in enumerate(live):
            assert (got[b, c:].view(np.int32) == nan_bits).all(), 'image %d: rows past count %d were written' % (b, c)
            if c:
                check_lincomb(got[b, :c], ins[b][0], ins[b][1][:c], ins[b][2][:c], crop, 'batch %s image %d crop %d' % (counts, b, crop))


def test_lincomb_crop_rejections():
    P = torch.zeros(64, device=DEV).data_ptr()
    lib, s = L.lib(), L.stream_ptr()
    assert lib.ymi_lincomb_crop_f32(P, P, P, P, 5, 7, 32, 1025, 1, s) == -1
    assert lib.ymi_lincomb_crop_batch_f32(P, P, P, None, P, 3, 1025, 5, 7, 32, 1, s) == -1
    assert lib.ymi_lincomb_crop_f32(P, P, P, P, 5, 7, 16, 4, 1, s) == -2 and lib.ymi_lincomb_crop_batch_f32(P, P, P, None, P, 3, 40, 5, 7, 16, 1, s) == -2
    for k in range(4):
        a = [P] * 4
        a[k] = None
        assert lib.ymi_lincomb_crop_f32(*a, 5, 7, 32, 4, 1, s) == -3
        assert lib.ymi_lincomb_crop_batch_f32(*(a[:3] + [None] + a[3:]), 3, 40, 5, 7, 32, 1, s) == -3


# ---- the two stages chained ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('h,w', [(97, 131), (550, 550)])
def test_chain_upsample_of_the_gpus_own_masks_lo_is_exact(h, w):
    """postprocess end to end without an undecidable threshold: the GPU's own masks_lo (138x138, N = 33, cropped) goes to the GPU
    upsample, and the restatement applied to the SAME masks_lo must give the same bits, soft and binarised at 0.5."""
    ph, pw, N = 138, 138, 33
    proto, coef, box = lincomb_inputs(ph, pw, N, seed=ph * 100 + N)
    pd, cd, bd = proto.to(DEV).contiguous(), coef.to(DEV).contiguous(), torch.from_numpy(box).to(DEV)
    lo = torch.full((N, ph, pw), NAN, device=DEV)
    L.check(L.lib().ymi_lincomb_crop_f32(pd.data_ptr(), cd.data_ptr(), bd.data_ptr(), lo.data_ptr(), ph, pw, 32, N, 1, L.stream_ptr()),
            'ymi_lincomb_crop_f32')
    want = MR.upsample_rows(lo.cpu().numpy(), h, w)
    for thresh in (-1.0, 0.5):
        got, k = run_upsample(lo, N, ph, pw, h, w, thresh)
        assert k == L.UP_BAND
        assert bits_equal(got, MR.binarise(want, thresh)), thresh
    assert 0.01 < (want > F(0.5)).mean() < 0.99


# ---- boxes_to_pixels -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('N', [1, 65])
def test_boxes_to_pixels_is_the_restatement(N):
    """N = 65 takes two blocks.  w != h."""
    for w, h in ((320, 240), (7, 5)):
        box = MR.boxes_for(N, w, h, seed=N) if N > 1 else MR.hand_boxes(w, h)[1:2]
        buf, out = guarded(N * 4, torch.int64, -7, tail=8)
        bd = torch.from_numpy(box).to(DEV)
        L.check(L.lib().ymi_boxes_to_pixels(bd.data_ptr(), out.data_ptr(), N, w, h, L.stream_ptr()), 'ymi_boxes_to_pixels')
        torch.cuda.synchronize()
        assert guards_intact(buf, N * 4, -7)
        assert np.array_equal(out.view(N, 4).cpu().numpy(), MR.boxes_to_pixels(box, w, h)), (N, w, h)
