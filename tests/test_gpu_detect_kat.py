"""Known-answer tests of Detect's Fast NMS kernels (csrc/detect.hip) on every dispatch branch and decision edge.

ymi_detect_f32 is driven through L.DetectDesc directly, workspaces sized by ymi_workspace_bytes; every output and workspace
buffer starts 4 elements into a sentinel-filled allocation, and the elements before and after must keep the sentinel.  After
each launch what EVERY kernel hands on is compared with tests/detect_ref.py (pinned to the oracle by test_detect_kat_host.py),
as bits or exact integers:
    K1  keep, num_keep, maxsc, argmax, scores_t          K2  cand_score, cand_prior, all top_k slots
    K3  out_count, then [:count] of box, score, class, coef, prior          the record: out_rec equals the separate outputs
Every case is launched twice and the two results must be bit-equal.

Floats enter in two places only.  Random-box cases: the device's expf may differ from the host's by an ulp or two, so the case's
smallest deciding IoU margin is re-asserted (>= 16 x detect_ref.iou_bound) before anything is compared, no decision is left
out, and boxes are held to |gpu - float64 decode| < 1e-6 (exact cases: bits).  Fused softmax: |gpu - float64 softmax| < 1e-6.
Which instantiation a case reaches is arithmetic on the host: the table in test_detect_kat_host.py.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detect_ref as R  # noqa: E402
from yolact_amd import _lib as L  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F = np.float32
NAN = float('nan')
ISENT = -7
EARG, ESHAPE, ENULL = -1, -2, -3
BOX_BAR = 1e-6
_REF = {}


def ref_of(cid):
    if cid not in _REF:
        case = R.build_case(cid)
        _REF[cid] = (case, R.detect(case, margins=(case['group'] in R.RANDOM_GROUPS)))
    return _REF[cid]


def guarded(total, dtype=torch.float32, tail=12):
    """-> (buffer, view of `total` elements starting 4 elements in), sentinel-filled: NaN (floats) or -7."""
    fill = NAN if dtype == torch.float32 else ISENT
    buf = torch.full((4 + total + tail,), fill, dtype=dtype, device=DEV)
    return buf, buf[4:4 + total]


def untouched(t):
    return bool(torch.isnan(t).all()) if t.dtype.is_floating_point else bool((t == ISENT).all())


def same_bits(a, b):
    """float32 arrays bit for bit; two NaNs are equal whatever their sign and payload."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and bool(((a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))).all())


BUFFERS = (('scores_t', torch.float32), ('keep', torch.int32), ('num_keep', torch.int32), ('maxsc', torch.float32),
           ('argmax', torch.int32), ('cand_score', torch.float32), ('cand_prior', torch.int32), ('out_count', torch.int32),
           ('out_box', torch.float32), ('out_score', torch.float32), ('out_class', torch.int64), ('out_coef', torch.float32),
           ('out_prior', torch.int32), ('out_rec', torch.float32))
INPUTS = ('conf', 'loc', 'coef', 'priors')


def launch(case, mutate=None, want_rc=0):
    """One ymi_detect_f32 call of a case -> dict of numpy arrays (want_rc == 0), or asserts the error code and that no buffer was
    written.  `mutate(d)` edits the descriptor before the call."""
    B, P, Cc, D, top_k, max_det = (case[k] for k in ('B', 'P', 'C', 'D', 'top_k', 'max_det'))
    cap = top_k if case['cross_class'] else max_det
    d = L.DetectDesc()
    d.B, d.P, d.C, d.D = B, P, Cc, D
    d.conf_ld = case['ld'] if case['ld'] != Cc or case.get('pass_ld') else 0
    d.conf_is_logits = int(case['is_logits'])
    d.top_k, d.max_det = top_k, max_det
    d.conf_thresh, d.nms_thresh = case['conf_thresh'], case['nms_thresh']
    d.cross_class = int(case['cross_class'])
    wb = lambda what: int(L.lib().ymi_workspace_bytes(what, C.byref(d)))
    n_st, n_pp, n_cand, n_rec = (wb(w) // 4 for w in (L.WS_DETECT_SCORES_T, L.WS_DETECT_PER_PRIOR, L.WS_DETECT_CAND, L.WS_DETECT_REC))
    assert (n_st, n_pp, n_cand, n_rec) == (B * (Cc - 1) * P, B * P, B * (Cc - 1) * top_k, B * (1 + cap * (6 + D)))
    sizes = dict(scores_t=n_st, keep=n_pp, num_keep=B, maxsc=n_pp, argmax=n_pp, cand_score=n_cand, cand_prior=n_cand, out_count=B,
                 out_box=B * cap * 4, out_score=B * cap, out_class=B * cap, out_coef=B * cap * D, out_prior=B * cap, out_rec=n_rec)
    ins = {k: torch.from_numpy(case[k]).to(DEV).contiguous() for k in INPUTS}
    for k in INPUTS:
        setattr(d, k, ins[k].data_ptr())
    bufs = {}
    for name, dt in BUFFERS:
        bufs[name] = guarded(sizes[name], dt)
        assert bufs[name][1].data_ptr() % 16 == 0
        setattr(d, name, bufs[name][1].data_ptr())
    if mutate is not None:
        mutate(d)
    rc = L.lib().ymi_detect_f32(C.byref(d), L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == want_rc, (case['name'], rc, want_rc)
    for name, (buf, view) in bufs.items():
        n = view.numel()
        assert untouched(buf[:4]) and untouched(buf[4 + n:]), '%s: wrote outside %s' % (case['name'], name)
        if want_rc != 0:
            assert untouched(buf), '%s: %s was written although the call returned %d' % (case['name'], name, rc)
    if want_rc != 0:
        return None
    nclass = 1 if case['cross_class'] else Cc - 1
    g = {k: v[1].cpu().numpy() for k, v in bufs.items()}
    used = B * nclass * top_k
    for k in ('cand_score', 'cand_prior'):             # cross-class uses the first B * top_k slots of a buffer sized for C - 1 classes
        assert untouched(bufs[k][1][used:]), '%s: %s past [B,nclass,top_k] was written' % (case['name'], k)
    return dict(keep=g['keep'].reshape(B, P), num_keep=g['num_keep'], maxsc=g['maxsc'].reshape(B, P), argmax=g['argmax'].reshape(B, P),
                scores_t=g['scores_t'].reshape(B, Cc - 1, P), cand_score=g['cand_score'][:used].reshape(B, nclass, top_k),
                cand_prior=g['cand_prior'][:used].reshape(B, nclass, top_k), count=g['out_count'], box=g['out_box'].reshape(B, cap, 4),
                score=g['out_score'].reshape(B, cap), cls=g['out_class'].reshape(B, cap), coef=g['out_coef'].reshape(B, cap, D),
                prior=g['out_prior'].reshape(B, cap), rec=g['out_rec'].reshape(B, 1 + cap * (6 + D)))


def launch_twice(case):
    a, b = launch(case), launch(case)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), '%s: %s differs between two launches' % (case['name'], k)
    return a


def check_k1(case, got, ref):
    k = ref['k1']
    for name in ('keep', 'num_keep', 'argmax'):
        assert np.array_equal(got[name], k[name]), '%s: K1 %s' % (case['name'], name)
    assert same_bits(got['maxsc'], k['maxsc']), '%s: K1 maxsc' % case['name']
    assert same_bits(got['scores_t'], k['scores_t']), '%s: K1 scores_t (sign bit = not kept)' % case['name']


def check_k2(case, got, ref):
    bad = np.argwhere(got['cand_prior'] != ref['k2']['cand_prior'])
    assert len(bad) == 0, '%s: K2 cand_prior differs in %d slots, first (image, class, rank) = %s: got %d, want %d (selected: %d)' % (
        case['name'], len(bad), tuple(bad[0]), got['cand_prior'][tuple(bad[0])], ref['k2']['cand_prior'][tuple(bad[0])],
        ref['k2']['rank_prior'][tuple(bad[0])])
    assert same_bits(got['cand_score'], ref['k2']['cand_score']), '%s: K2 cand_score' % case['name']


def check_k3(case, got, ref, exact_boxes):
    k, D = ref['k3'], case['D']
    assert np.array_equal(got['count'], k['count']), '%s: K3 count %s, want %s' % (case['name'], got['count'], k['count'])
    for b in range(case['B']):
        n = int(k['count'][b])
        assert np.array_equal(got['prior'][b, :n], k['prior'][b, :n]), '%s: K3 prior, image %d' % (case['name'], b)
        assert got['cls'].dtype == np.int64 and np.array_equal(got['cls'][b, :n], k['cls'][b, :n]), '%s: K3 class, image %d' % (case['name'], b)
        assert same_bits(got['score'][b, :n], k['score'][b, :n]) and same_bits(got['coef'][b, :n], k['coef'][b, :n]), (case['name'], b)
        if exact_boxes:
            assert same_bits(got['box'][b, :n], k['box'][b, :n]), '%s: K3 box bits, image %d' % (case['name'], b)
        elif n:
            pri = k['prior'][b, :n]
            err = np.abs(got['box'][b, :n].astype(np.float64) - R.decode64(case['loc'][b, pri], case['priors'][pri])).max()
            assert err < BOX_BAR, '%s: box error %g, image %d' % (case['name'], err, b)
        # the packed record: count | cap x (box 4, score, class, coef D), equal to the separate outputs
        assert got['rec'][b, 0] == F(n)
        r = got['rec'][b, 1:].reshape(-1, 6 + D)[:n]
        assert same_bits(r[:, :4], got['box'][b, :n]) and same_bits(r[:, 4], got['score'][b, :n]), (case['name'], b)
        assert same_bits(r[:, 5], got['cls'][b, :n].astype(F)) and same_bits(r[:, 6:], got['coef'][b, :n]), (case['name'], b)


def run_case(cid):
    case, ref = ref_of(cid)
    exact = case['group'] not in R.RANDOM_GROUPS
    if not exact:                                      # no decision may hang on the device's expf
        margin, bar = R.margin_ok(case, ref)
        assert margin >= bar and ref['k1']['min_conf_margin'] > 1e-4, (cid, margin, bar)
    got = launch_twice(case)
    check_k1(case, got, ref)
    if case['group'] == 7:                             # K1 edges: compared on K1's five outputs
        return case, ref, got
    check_k2(case, got, ref)
    check_k3(case, got, ref, exact)
    return case, ref, got


# ---- 1-6: K2 / K3 dispatch, selection sizes, the IoU triangle, the threshold, degenerate boxes -------------------------------------

@pytest.mark.parametrize('cid', R.case_ids(1))
def test_k2_dispatch_and_ties_on_the_cut(cid):
    """P around 24 * 1024 and 64 * 1024, B = 2 (image 1's rows are unaligned when P % 4 != 0), per-class and cross-class: EPT 24 / 64
    with 16-byte and scalar loads, keys in memory; 3 x as many exact ties on the cut as slots, the lowest indices win."""
    run_case(cid)


@pytest.mark.parametrize('cid', R.case_ids(2))
def test_k3_dispatch_and_ties_over_classes(cid):
    """final_topk_k<64> with 16-byte (20 480 candidates) and scalar loads (16 575), <16> with scalar loads and an unaligned second
    image (765) and at the boundary (16 384); max_det 256 / 100 / 1 / 100, the cut inside a tie that spans the classes."""
    run_case(cid)


@pytest.mark.parametrize('cid', R.case_ids(3))
def test_selection_sizes(cid):
    """top_k in {1, 2, 3, 9, 255, 256}, image b with K in {1, top_k - 1, top_k, top_k + 1}, P = 1024."""
    run_case(cid)


@pytest.mark.parametrize('cid', R.case_ids(4))
def test_iou_triangle_row_by_row(cid):
    """Two priors carry one box: class c puts them at ranks (i, j) and exactly column j must go, for every pair of k <= 17 and for
    the longest column, the first row, the diagonal and random pairs of k = 255 / 256 (odd k: the middle column stands alone)."""
    case, ref, got = run_case(cid)
    for b in range(case['B']):
        for c, (i, j) in enumerate(case['pairs'][b]):
            cp = got['cand_prior'][b, c]
            assert cp[j] == -1 and cp[i] == 0 and (np.delete(cp, j) >= 0).all(), (cid, b, c, i, j)


@pytest.mark.parametrize('ab', R.RCP_DIFFERS + R.RCP_AGREES, ids=lambda ab: '%d_%d' % ab)
def test_iou_on_the_threshold(ab):
    """IoU = fl(a / b) exactly; nms_thresh one ulp below, on, one ulp above: suppressed, kept, kept.  For the first 14 pairs the
    float32 a * (1 / b) rounds differently from a / b: a kernel that trusted the reciprocal everywhere fails here."""
    for tag, gone in zip('m0p', (True, False, False)):
        case, ref, got = run_case('iou-%d-%d-%s' % (ab + (tag,)))
        assert (got['cand_prior'][0, 0, 1] == -1) == gone and (got['cand_prior'][0, 1, 1] == -1) == gone, (ab, tag)


@pytest.mark.parametrize('cid', R.case_ids(6))
def test_degenerate_boxes_and_threshold_edges(cid):
    """0 / 0 (NaN: suppressed), zero area against an ordinary box (0: kept), infinite width as a row and as a column (x2 = NaN),
    nms_thresh = 0 (only zero overlap survives), nms_thresh = -0.5 (count 0, every candidate -1), IoU 0.5 at 0.5 and 1 at 1.0 (kept)."""
    case, ref, got = run_case(cid)
    assert got['cand_prior'][0, 0].tolist() == case['want0']


# ---- 7: K1 edges -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('C_ld', R.K1_SHAPES, ids=lambda s: 'C%d_ld%d' % s)
def test_k1_scores_input(C_ld):
    """Post-softmax input, P in {1, 63, 64, 65, 700}: a maximum equal to conf_thresh is not kept, next(conf_thresh) is; foreground
    maxima tied 1 to 4 classes apart go to the first; an image with K = 0 between two with K > 0; padded rows (ld > C), even C,
    C at the LDS limit."""
    for P in R.K1_PS:
        run_case('k1-%d-%d-%d-scores' % (C_ld + (P,)))


@pytest.mark.parametrize('C_ld', R.K1_SHAPES, ids=lambda s: 'C%d_ld%d' % s)
def test_k1_logits_input(C_ld):
    """Fused softmax: |gpu - float64 softmax| < 1e-6 on every score; keep, num_keep and argmax exact (the host test asserts that
    every row's float64 margin to conf_thresh and every kept row's margin to the runner-up exceed the bar); the sign bit of
    scores_t is set exactly where keep == 0, also on scores that are exactly 0.0.
    Largest |gpu - float64 softmax| seen on the MI355X, over the five P of each shape, against the bar of 1e-6:
        C 2: 8.78e-8    C 3: 1.32e-7    C 4: 1.29e-7    C 81 (ld 81, 82, 84): 4.17e-7    C 234 (ld 234, 236): 6.51e-7"""
    worst = 0.0
    for P in R.K1_PS:
        case, ref = ref_of('k1-%d-%d-%d-logits' % (C_ld + (P,)))
        got = launch_twice(case)
        k = ref['k1']
        keep_sure, arg_sure = R.k1_sure(k, case['conf_thresh'])
        assert keep_sure.all()
        s64 = k['scores64'][:, :, 1:].transpose(0, 2, 1)
        err = float(np.abs(np.abs(got['scores_t']).astype(np.float64) - s64).max())
        worst = max(worst, err, float(np.abs(got['maxsc'].astype(np.float64) - s64.max(1)).max()))
        assert np.array_equal(got['keep'], k['keep']) and np.array_equal(got['num_keep'], k['num_keep']), case['name']
        assert np.array_equal(got['argmax'][arg_sure], k['argmax'][arg_sure]), case['name']
        assert np.array_equal(np.signbit(got['scores_t']), np.broadcast_to(k['keep'][:, None, :] == 0, got['scores_t'].shape)), case['name']
        assert np.array_equal(got['maxsc'], np.abs(got['scores_t']).max(1)), case['name']
    print('C %d ld %d: largest |gpu - float64 softmax| = %.3g (bar %g)' % (C_ld + (worst, R.SCORE_BAR)))
    assert worst < R.SCORE_BAR


def test_k1_rejects_c_over_the_lds_limit():
    case, _ = ref_of('k1-234-234-1-scores')
    launch(case, lambda d: (setattr(d, 'C', 235), setattr(d, 'conf_ld', 0)), ESHAPE)


# ---- 8: argument rejection ---------------------------------------------------------------------------------------------------------

def test_argument_rejection_launches_nothing():
    case, _ = ref_of('deg-1')
    for field, value in (('top_k', 0), ('top_k', 257), ('max_det', 0), ('max_det', 257), ('C', 1), ('conf_ld', 2), ('conf_ld', 1),
                         ('B', 65536), ('B', 0), ('P', 0), ('D', 0)):
        launch(case, lambda d: setattr(d, field, value), EARG)
    for name in INPUTS + tuple(n for n, _ in BUFFERS if n != 'out_rec'):
        launch(case, lambda d: setattr(d, name, None), ENULL)
    assert L.lib().ymi_detect_f32(None, L.stream_ptr()) == ENULL
    launch(case, lambda d: setattr(d, 'out_rec', None))          # the record is optional


# ---- 9: one batch, mixed -----------------------------------------------------------------------------------------------------------

def test_mixed_batch_equals_single_images():
    """B = 8, P = 24 577: K = 0, 1, 150, 200 (= top_k), 700 with 600 tied on the cut, 24 577 (all kept), 201, 0.  Bit-equal to the
    eight single-image launches and to the reference."""
    case, ref, got = run_case('mixed')
    for b in range(case['B']):
        one = launch(R.slice_image(case, b))
        n = int(got['count'][b])
        assert one['count'][0] == n == ref['k3']['count'][b]
        for k in ('keep', 'num_keep', 'maxsc', 'argmax', 'scores_t', 'cand_score', 'cand_prior'):
            assert one[k][0].tobytes() == got[k][b].tobytes(), (b, k)
        for k in ('box', 'score', 'cls', 'coef', 'prior'):
            assert one[k][0, :n].tobytes() == got[k][b, :n].tobytes(), (b, k)
        assert one['rec'][0, :1 + n * (6 + case['D'])].tobytes() == got['rec'][b, :1 + n * (6 + case['D'])].tobytes(), b


# ---- 10: through Detect ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('mode', ['pc', 'cc'])
def test_through_detect_at_top_k_256(mode):
    """Detect(81, 0, 256, 0.05, 0.5) with max_num_detections = 256: the wrapper's workspace sizing at a top_k it has never been given."""
    import yolact_amd
    from yolact_amd.config import active_cfg
    from yolact_amd.layers.detection import Detect
    case, ref = ref_of('wrap-' + mode)
    margin, bar = R.margin_ok(case, ref)
    assert margin >= bar
    yolact_amd.set_cfg('yolact_resnet50_config')
    cfg = active_cfg()
    old = cfg.max_num_detections
    cfg.max_num_detections = 256
    try:
        det = Detect(81, 0, 256, 0.05, 0.5)
        det.use_fast_nms, det.use_cross_class_nms = True, mode == 'cc'
        preds = {'loc': torch.from_numpy(case['loc']).to(DEV), 'conf': torch.from_numpy(case['conf']).to(DEV),
                 'mask': torch.from_numpy(case['coef']).to(DEV), 'priors': torch.from_numpy(case['priors']).to(DEV)}
        out = det(preds, None)
        assert int(ref['k3']['count'].max()) == 256
        for b in range(case['B']):
            n = int(ref['k3']['count'][b])
            got = out[b]['detection']
            assert np.array_equal(det.last_prior_idx[b].cpu().numpy(), ref['k3']['prior'][b, :n])
            assert np.array_equal(got['class'].cpu().numpy(), ref['k3']['cls'][b, :n])
            assert same_bits(got['score'].cpu().numpy(), ref['k3']['score'][b, :n])
            assert same_bits(got['mask'].cpu().numpy(), ref['k3']['coef'][b, :n])
        bad = Detect(81, 0, 257, 0.05, 0.5)
        bad.use_fast_nms = True
        with pytest.raises(RuntimeError):
            bad(preds, None)
    finally:
        cfg.max_num_detections = old
