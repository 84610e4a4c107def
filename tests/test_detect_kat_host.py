"""CPU side of the Detect known-answer tests: tests/detect_ref.py is pinned to the oracle, and every case that
tests/test_gpu_detect_kat.py launches on the MI355X is built here and checked for what that file relies on.

Agreement with the oracle: prior, class and score exactly, boxes by bits.  exp is the one library function inside decode, and
torch's float32 exp differs from the correctly rounded one in about 1% of arguments (measured: 21 932 of 2 000 000), so for this
comparison, and only here, the reference is handed torch's exp; everything else in it is numpy.

Dispatch arithmetic of ymi_detect_f32 (csrc/detect.hip), asserted by test_dispatch_table_covers_every_reachable_instantiation:
    K2 class_topk_nms_k<EPT, 1024, SIGNED>: EPT = 24 for P <= 24 * 1024, 64 for P <= 64 * 1024, else 0 (keys in memory);
       SIGNED = per-class mode; 16-byte loads when P % 4 == 0 and the row pointers are 16-byte aligned (for image b > 0 and
       class c > 0 the rows start at multiples of P elements: aligned exactly when P % 4 == 0), else scalar loads.
    K3 final_topk_k<EPT>: n = nclass * top_k; EPT = 16 for n <= 16 * 1024, 64 for n <= 64 * 1024, else 0; 16-byte loads when
       n % 4 == 0.
    final_topk_k<0> CANNOT be reached through ymi_detect_f32: the LDS check 64 * C * 4 <= 60 000 gives C <= 234 and top_k <= 256,
    so n <= 233 * 256 = 59 648 < 65 536.  The kernel is left as it is; no case can run it.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detect_ref as R  # noqa: E402
from helpers import oracle_run  # noqa: E402
from oracle import yolact_oracle as O  # noqa: E402

F = np.float32
_REF = {}


def torch_exp(x):
    return torch.exp(torch.from_numpy(np.ascontiguousarray(x))).numpy()


def ref_of(cid):
    """(case, reference) of a registered case, computed once."""
    if cid not in _REF:
        case = R.build_case(cid)
        _REF[cid] = (case, R.detect(case))
    return _REF[cid]


def same_bits(a, b):
    """Bit equality of float32 arrays; two NaNs are equal whatever their sign and payload (IEEE 754 does not fix them)."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and bool(((a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))).all())


def assert_is_oracle(case, ref, what):
    """The reference's K3 output of every image against oracle.detect_image."""
    for b in range(case['B']):
        o = O.detect_image(torch.from_numpy(case['conf'][b, :, :case['C']].copy()), torch.from_numpy(case['loc'][b]),
                           torch.from_numpy(case['coef'][b]), torch.from_numpy(case['priors']), case['conf_thresh'],
                           case['nms_thresh'], case['top_k'], case['max_det'], case['cross_class'])
        n = int(ref['k3']['count'][b])
        if o is None or len(o['prior']) == 0:
            assert n == 0, (what, b, n)
            continue
        assert n == len(o['prior']), (what, b, n, len(o['prior']))
        assert np.array_equal(ref['k3']['prior'][b, :n], o['prior'].numpy()), (what, b, 'prior')
        assert np.array_equal(ref['k3']['cls'][b, :n], o['class'].numpy()), (what, b, 'class')
        assert same_bits(ref['k3']['score'][b, :n], o['score'].numpy()), (what, b, 'score')
        assert same_bits(ref['k3']['box'][b, :n], o['box'].numpy()), (what, b, 'box')
        assert same_bits(ref['k3']['coef'][b, :n], o['mask'].numpy()), (what, b, 'coef')


# ---- agreement with the oracle -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['r50_dense', 'r50_sparse', 'r50_empty', 'im700', 'plus_r50', 'r50_cc', 'r50_few'])
def test_reference_is_the_oracle_on_the_detect_goldens(name):
    meta, arrays, cfg, sd, raw, dets = oracle_run(name)
    case = R.make_case(name, 'golden', raw['conf'].numpy(), raw['loc'].numpy(), raw['priors'].numpy(), coef=raw['mask'].numpy(),
                       top_k=cfg.nms_top_k, max_det=cfg.max_num_detections, conf_thresh=cfg.nms_conf_thresh,
                       nms_thresh=cfg.nms_thresh, cross_class=bool(meta.get('cross_class', False)))
    ref = R.detect(case, exp32=torch_exp, margins=False)
    assert_is_oracle(case, ref, name)
    for b, d in enumerate(dets):                       # and the detections helpers.oracle_run itself made
        assert int(ref['k3']['count'][b]) == (0 if d is None else len(d['prior']))


def random_case(i):
    """Seeded, with non-default top_k, max_det and thresholds; odd i: cross-class.  Boxes large enough for the NMS to act."""
    rs = np.random.RandomState(500 + i)
    B, P, C = 2, int(rs.randint(50, 400)), int(rs.randint(2, 12))
    conf = rs.rand(B, P, C).astype(F)
    conf[:, ::3, 1:] = conf[:, ::3, 1:2]              # ties across classes and priors
    conf[:, 1::7] = conf[:, :1]
    pri = np.empty((P, 4), F)
    pri[:, :2] = rs.rand(P, 2)
    pri[:, 2:] = 0.1 + 0.5 * rs.rand(P, 2)
    loc = (rs.randn(B, P, 4) * 0.5).astype(F)
    return R.make_case('random %d' % i, 'random', conf, loc, pri, coef=rs.randn(B, P, 5).astype(F),
                       top_k=int(rs.choice([1, 2, 3, 7, 50, 255, 256])), max_det=int(rs.choice([1, 3, 20, 256])),
                       conf_thresh=float(rs.choice([0.0, 0.05, 0.3, 0.7])), nms_thresh=float(rs.choice([0.0, 0.1, 0.3, 0.5, 0.7, 1.0])),
                       cross_class=bool(i & 1))


def test_reference_is_the_oracle_on_random_cases():
    acted = 0
    for i in range(24):
        case = random_case(i)
        ref = R.detect(case, exp32=torch_exp, margins=False)
        assert_is_oracle(case, ref, case['name'])
        acted += int(((ref['k2']['rank_prior'] >= 0) & (ref['k2']['cand_prior'] < 0)).any())
    assert acted >= 12                                # the NMS suppressed something in at least half of them


# ---- conditions the GPU tests rely on ----------------------------------------------------------------------------------------------

NONFINITE = ('deg-2', 'deg-3')                        # the infinite-width cases: float64 does not overflow where float32 does


@pytest.mark.parametrize('group', [4, 5, 6])
def test_exact_cases_are_exact(group):
    """loc = 0 and priors on a 2^-k grid: the float32 and the float64 decode and IoU agree bit for bit after rounding, so the
    device has no rounding of its own to add (expf(0) = 1).  The two infinite-width cases are pinned to the oracle instead."""
    for cid in R.case_ids(group):
        case, ref = ref_of(cid)
        assert not case['loc'][np.isfinite(case['loc']) & (case['loc'] != 1000)].any()
        if cid not in NONFINITE:
            assert ref['k2']['exact'], cid


def test_degenerate_cases_are_the_oracle_and_the_hand_answers():
    for cid in R.case_ids(6):
        case, ref = ref_of(cid)
        assert_is_oracle(case, ref, case['name'])
        assert ref['k2']['cand_prior'][0, 0].tolist() == case['want0'], (case['name'], ref['k2']['cand_prior'][0, 0])
    case, ref = ref_of('deg-2')
    assert np.isnan(R.decode32(case['loc'][0], case['priors'])[0, 2]) and np.isinf(R.decode32(case['loc'][0], case['priors'])[0, 0])
    case, ref = ref_of('deg-5')
    assert ref['k3']['count'].tolist() == [0] and (ref['k2']['cand_prior'] == -1).all() and (ref['k2']['cand_score'] == -1).all()


@pytest.mark.parametrize('group', R.RANDOM_GROUPS)
def test_random_cases_clear_their_margin(group):
    """The device's expf may differ from the host's by an ulp or two; a deciding IoU near nms_thresh could then flip with no bug.
    Bound on the IoU change, from a 2-ulp error in w and h:
      w is off by 2^-22 w; x1 = cx - w / 2 and x2 = w + x1 then by 1.5 * 2^-22 w plus their own roundings (2^-24 |x| each): every
      coordinate moves by at most e = 2^-21 M, M = the largest |coordinate| of the case (sides are smaller than that).
      An area w h changes by dA <= 2 e (w + h) + 4 e^2, so dA / A <= 4 e / m + 4 e^2 / m^2 with m = the case's SMALLEST box side; the
      intersection is a box no larger than either, so dI <= dA_i.  IoU = I / U, U = A_i + A_j - I >= max(A_i, A_j), I <= U:
      d(IoU) <= (dI + dU) / U <= (2 dI + dA_i + dA_j) / U <= 3 dA_i / A_i + dA_j / A_j <= 16 (e / m) (1 + e / m).
      The float32 evaluation of the IoU itself (8 roundings) adds less than 2^-20.
    R.iou_bound is that sum; the smallest deciding margin |IoU64 - nms_thresh| over ALL pairs i < j of every (image, class) top-k,
    float64 from the reference alone, must be at least 16 x it (the seed margin of backbone_train_ref.find_seed)."""
    for cid in R.case_ids(group):
        case, ref = ref_of(cid)
        margin, bar = R.margin_ok(case, ref)
        print('%s: smallest side %.4g, largest coordinate %.3g, margin %.4g, 16 x bound %.4g; conf margin %.3g'
              % (cid, ref['k2']['min_side'], ref['k2']['max_coord'], margin, bar, ref['k1']['min_conf_margin']))
        assert margin >= bar, (cid, margin, bar)
        assert ref['k1']['min_conf_margin'] > 1e-4      # post-softmax input: K1 compares the given floats, nothing to round


def test_k2_tie_cases_have_more_equals_than_slots():
    for cid in R.case_ids(1):
        case, ref = ref_of(cid)
        P, top_k = case['P'], case['top_k']
        for b in range(case['B']):
            keep = ref['k1']['keep'][b] != 0
            assert keep.sum() > top_k
            for c in range(ref['k2']['rank_prior'].shape[1]):
                sc = ref['k1']['maxsc'][b] if case['cross_class'] else case['conf'][b, :, 1 + c]
                n_gt, eq = int((keep & (sc > R.TIE)).sum()), keep & (sc == R.TIE)
                assert 4 <= n_gt < top_k and eq.sum() >= 3 * (top_k - n_gt), (cid, b, c, n_gt, eq.sum())
                assert eq[R.k2_tie_indices(P)].all()
                sel = ref['k2']['rank_prior'][b, c]
                tied_sel = np.sort(sel[n_gt:])
                assert np.array_equal(tied_sel, np.nonzero(eq)[0][:top_k - n_gt])       # the lowest indices, 0, 3 and 4 among them
                assert {0, 3, 4, 4095, 4096} <= set(sel.tolist()) and P - 1 not in sel and P - 2 not in sel
    case, ref = ref_of('mixed')
    b = case['Ks'].index(700)
    eq = case['conf'][b, :, 1] == R.TIE
    assert eq.sum() == 600 and (case['conf'][b, :, 1] > R.TIE).sum() == 100


def test_k3_tie_cases_cut_inside_a_tie_over_several_classes():
    for cid in R.case_ids(2):
        case, ref = ref_of(cid)
        for b in range(case['B']):
            n = int(ref['k3']['count'][b])
            survivors = int((ref['k2']['cand_prior'][b] >= 0).sum())
            assert n == case['max_det'] < survivors
            last = ref['k3']['score'][b, n - 1]
            tied_all = int(((ref['k2']['cand_score'][b] == last) & (ref['k2']['cand_prior'][b] >= 0)).sum())
            tied_taken = ref['k3']['score'][b, :n] == last
            assert tied_all > tied_taken.sum()                              # the cut falls inside the tie
            assert len(np.unique(ref['k2']['cand_score'][b][ref['k2']['cand_prior'][b] >= 0])) > 2
            ncls_all = int(((ref['k2']['cand_score'][b] == last) & (ref['k2']['cand_prior'][b] >= 0)).any(1).sum())
            assert ncls_all >= 3, (cid, ncls_all)                           # the tie spans several classes ...
            if case['max_det'] > 1:
                assert len(np.unique(ref['k3']['cls'][b, :n][tied_taken])) >= 2   # ... and so do the tied detections taken


def test_selection_cases_have_the_listed_K():
    for cid in R.case_ids(3):
        case, ref = ref_of(cid)
        k = case['top_k']
        assert ref['k1']['num_keep'].tolist() == sorted({x for x in (1, k - 1, k, k + 1) if x > 0}) == case['Ks']
    case, ref = ref_of('mixed')
    assert ref['k1']['num_keep'].tolist() == case['Ks'] == [0, 1, 150, 200, 700, 24577, 201, 0]


def test_triangle_cases_suppress_exactly_column_j():
    seen = {}
    for cid in R.case_ids(4):
        case, ref = ref_of(cid)
        k = case['top_k']
        pairs = set()
        for b in range(case['B']):
            for c, (i, j) in enumerate(case['pairs'][b]):
                pairs.add((i, j))
                rp, cp = ref['k2']['rank_prior'][b, c], ref['k2']['cand_prior'][b, c]
                assert rp[i] == 0 and rp[j] == 1
                want = rp.copy()
                want[j] = -1
                assert np.array_equal(cp, want), (cid, b, c, i, j)
        seen[k] = pairs
        if k <= 17:
            assert len(pairs) == k * (k - 1) // 2
        else:
            assert {(i, k - 1) for i in range(k - 1)} | {(0, j) for j in range(1, k)} | {(j - 1, j) for j in range(1, k)} <= pairs
            assert len(pairs) == 8 * 233 and case['C'] == 234
    assert sorted(seen) == [2, 3, 4, 9, 17, 255, 256]


def test_on_threshold_cases_sit_on_the_threshold():
    assert len(R.RCP_DIFFERS) >= 12
    for a, b in R.RCP_DIFFERS + R.RCP_AGREES:
        q = F(a) / F(b)
        assert (F(a) * (F(1) / F(b)) != q) == ((a, b) in R.RCP_DIFFERS)
        for w, tag in zip((-1, 0, 1), 'm0p'):
            case, ref = ref_of('iou-%d-%d-%s' % (a, b, tag))
            bx = R.decode32(case['loc'][0], case['priors'])
            iou = R.iou_matrix(bx)[0, 1]
            assert iou == q and R.iou_matrix(R.decode64(case['loc'][0], case['priors']))[0, 1] == a / b      # exact a / b, rounded once
            th = F(case['nms_thresh'])
            assert th == [R.prv(q), q, R.nxt(q)][w + 1]
            for c in (0, 1):                              # class 0: box 1 is the column; class 1: box 0 is
                cp = ref['k2']['cand_prior'][0, c]
                col = 1 - c
                assert (cp[1] == -1) == (w < 0) and cp[0] == c and cp[1] in (-1, col), (a, b, w, cp)
                assert cp[2] >= 0 and cp[3] >= 0


def test_k1_cases_hold_what_they_claim():
    for cid in R.case_ids(7):
        case, ref = ref_of(cid)
        k = ref['k1']
        assert k['num_keep'][1] == 0 and (case['P'] == 1 or (k['num_keep'][0] > 0 and k['num_keep'][2] > 0)), cid
        if case['ld'] > case['C']:
            assert (case['conf'][:, :, case['C']:] > case['conf'][:, :, :case['C']].max()).all()       # the padding would win
        if case['is_logits']:
            keep_sure, arg_sure = R.k1_sure(k, case['conf_thresh'])
            assert keep_sure.all(), cid                   # keep and num_keep are decided on every row
            assert arg_sure[k['keep'] != 0].all(), cid    # and argmax on every kept row
            if case['P'] >= 63:
                kept = k['keep'] != 0
                st = np.abs(k['scores_t']).transpose(0, 2, 1)            # [B,P,C-1]
                assert (st[kept] == 0).any() or case['C'] == 2            # +-80 rows: exactly 0.0 ...
                assert not np.signbit(k['scores_t'].transpose(0, 2, 1)[kept]).any()     # ... and still a candidate of a kept prior
                assert ((st[kept] > 0) & (st[kept] < 1e-20)).any() or case['C'] == 2    # 60 above the rest: ~8.8e-27, not 0
        else:
            th = F(case['conf_thresh'])
            on, nx = k['maxsc'] == th, k['maxsc'] == R.nxt(th)
            assert on.any() and not k['keep'][on].any()
            if case['P'] >= 63:
                assert nx.any() and k['keep'][nx].all()
                if case['C'] >= 81:
                    fg = case['conf'][:, :, 1:case['C']]
                    tied = (fg == k['maxsc'][:, :, None])
                    d = {int(np.diff(np.nonzero(r)[0])[0]) for r in tied.reshape(-1, fg.shape[2]) if r.sum() == 2}
                    assert {1, 2, 3, 4} <= d, (cid, d)


# ---- teeth -------------------------------------------------------------------------------------------------------------------------

def differs(cid, variant, keys=('cand_prior',), stage='k2'):
    case, ref = ref_of(cid)
    other = R.detect(case, variant=variant, margins=False)
    return any(not np.array_equal(ref[stage][k], other[stage][k]) for k in keys)


def test_teeth_ties_to_the_highest_index():
    for cid in R.case_ids(1) + ['mixed']:
        assert differs(cid, 'ties_high'), cid                                        # K2's cut
    for cid in R.case_ids(2) + ['tri-17', 'tri-256']:
        assert differs(cid, 'ties_high', ('prior', 'cls'), 'k3'), cid                # K3's cut


def test_teeth_strict_comparison_and_reciprocal_quotient():
    for a, b in R.RCP_DIFFERS + R.RCP_AGREES:
        assert differs('iou-%d-%d-0' % (a, b), 'lt'), (a, b)                         # IoU == thresh: `<` suppresses
        hit = [differs('iou-%d-%d-%s' % (a, b, t), 'rcp') for t in 'm0p']
        assert any(hit) == ((a, b) in R.RCP_DIFFERS), (a, b, hit)
    for cid in ('deg-4', 'deg-6', 'deg-7'):
        assert differs(cid, 'lt'), cid


def test_teeth_conf_thresh_and_nan():
    for cid in R.case_ids(7):
        if cid.endswith('scores'):
            assert differs(cid, 'conf_ge', ('keep', 'num_keep', 'scores_t'), 'k1'), cid
    for cid in ('deg-0', 'deg-2', 'deg-3'):
        assert differs(cid, 'nan_zero'), cid


# ---- dispatch arithmetic -----------------------------------------------------------------------------------------------------------

# case id -> the instantiations and load forms it reaches: ('K2', EPT, SIGNED, loads), ('K3', EPT, loads)
DISPATCH = {
    'k2-24574-pc': {('K2', 24, True, 'scalar'), ('K3', 16, 'vec')}, 'k2-24574-cc': {('K2', 24, False, 'scalar'), ('K3', 16, 'vec')},
    'k2-24576-pc': {('K2', 24, True, 'vec'), ('K3', 16, 'vec')}, 'k2-24576-cc': {('K2', 24, False, 'vec'), ('K3', 16, 'vec')},
    'k2-24577-pc': {('K2', 64, True, 'scalar'), ('K3', 16, 'vec')}, 'k2-24577-cc': {('K2', 64, False, 'scalar'), ('K3', 16, 'vec')},
    'k2-65536-pc': {('K2', 64, True, 'vec'), ('K3', 16, 'vec')}, 'k2-65536-cc': {('K2', 64, False, 'vec'), ('K3', 16, 'vec')},
    'k2-65537-pc': {('K2', 0, True, 'memory'), ('K3', 16, 'vec')}, 'k2-65537-cc': {('K2', 0, False, 'memory'), ('K3', 16, 'vec')},
    'k2-65539-pc': {('K2', 0, True, 'memory'), ('K3', 16, 'vec')}, 'k2-65539-cc': {('K2', 0, False, 'memory'), ('K3', 16, 'vec')},
    'k3-81-256-256-1': {('K2', 24, True, 'vec'), ('K3', 64, 'vec')},        # 20 480 candidates
    'k3-66-255-100-1': {('K2', 24, True, 'vec'), ('K3', 64, 'scalar')},     # 16 575
    'k3-4-255-1-2': {('K2', 24, True, 'vec'), ('K3', 16, 'scalar')},        # 765; image 1 starts 765 elements in
    'k3-65-256-100-1': {('K2', 24, True, 'vec'), ('K3', 16, 'vec')},        # 16 384: the boundary
    'mixed': {('K2', 64, True, 'scalar'), ('K3', 16, 'vec')},
    'sel-255-cc': {('K2', 24, False, 'vec'), ('K3', 16, 'scalar')},         # cross-class: n = top_k = 255
}


def test_dispatch_table_covers_every_reachable_instantiation():
    reached = set()
    for cid, want in DISPATCH.items():
        case, _ = ref_of(cid)
        assert R.branches(case) == want, (cid, R.branches(case))
        reached |= want
    assert reached == R.REACHABLE and len(R.REACHABLE) == 14
    # the rule itself at its edges, and the one instantiation nothing reaches
    assert R.k2_branch(24 * 1024, False)[1] == 24 and R.k2_branch(24 * 1024 + 1, False)[1] == 64
    assert R.k2_branch(64 * 1024, False)[1] == 64 and R.k2_branch(64 * 1024 + 1, False)[1] == 0
    assert R.k3_branch(65, 256, False)[1] == 16 and R.k3_branch(66, 255, False)[1] == 64
    assert (R.C_MAX - 1) * R.SORT_N == 59648 <= 64 * R.NT and 64 * R.C_MAX * 4 <= 60000 < 64 * (R.C_MAX + 1) * 4
    assert R.k3_branch(R.C_MAX, R.SORT_N, False)[1] == 64
