"""MultiBoxLoss target assignment and the box loss, on the CPU: tests/match_ref.py is pinned to what the reference's own
MultiBoxLoss.forward computed (tests/golden/match.npz, written by tools/make_golden_match.py), shown to tell wrong variants apart,
and the C ABI / Python surface of ymi_match_f32 is checked as far as that goes without a GPU.

Golden bars: conf_t, idx_t and gt_box_t exact; loc_t, 'B' and d B / d loc_data relative error <= 1e-6 (both sides are fp32 on the
CPU; what differs is the summation order of 'B' and 0.1 w against w / 10 style rewrites of encode, a few ulp).
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_ref as R  # noqa: E402
import yolact_amd.layers.match as M  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
META, CASES = R.load_golden()
NAMES = [c['name'] for c in META['cases']]
GOLDEN_BAR = 1e-6


def test_golden_holds_the_cases_the_kernel_can_get_wrong():
    assert NAMES == ['plain3', 'shared_best', 'degenerate', 'crowds', 'many_gt']
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'match.npz')) < 256 * 1024
    by = {c['name']: c for c in META['cases']}
    assert by['crowds']['num_crowds'] == [1, 0, 2]
    assert by['many_gt']['n'][0] - 1 > 64 and all(c['P'] % 256 for c in META['cases'])
    t = CASES['shared_best']
    ov = R.iou(t['targets'][0][:, :4], R.point_form(t['priors']))
    assert ov[0].argmax() == ov[1].argmax() == 100                     # two GTs, one best prior
    t = CASES['crowds']
    c = t['conf_t'][0]
    assert c[114] == 12 and (c == -1).sum() > 100                       # the positive inside the crowd stays; its background turns neutral


@pytest.mark.parametrize('name', NAMES)
def test_ref_equals_the_reference(name):
    t = CASES[name]
    out = R.match_batch_ref(t['priors'], t['targets'], t['num_crowds'])
    for k in ('conf_t', 'idx_t', 'gt_box_t'):
        assert torch.equal(out[k], t[k]), k
    loss, d_loc = R.box_loss_ref(t['loc_data'], out['loc_t'], out['pos'], META['bbox_alpha'])
    errs = (R.rel_err(out['loc_t'], t['loc_t']), R.rel_err(loss.view(1), t['B']), R.rel_err(d_loc, t['d_loc']))
    print('%s: loc_t %.3e B %.3e d_loc %.3e' % ((name,) + errs))
    assert max(errs) <= GOLDEN_BAR, errs
    assert torch.equal(d_loc[~out['pos']], torch.zeros_like(d_loc[~out['pos']]))


@pytest.mark.parametrize('name', NAMES)
def test_plain_torch_encode_equals_the_reference(name):
    from yolact_amd.layers.box_utils import encode
    t = CASES[name]
    for b in range(len(t['targets'])):
        assert R.rel_err(encode(t['gt_box_t'][b], t['priors']), t['loc_t'][b]) <= GOLDEN_BAR


@pytest.mark.parametrize('case,variant', [('degenerate', dict(tie='highest')), ('plain3', dict(pos_first=False)),
                                          ('crowds', dict(crowd_over='crowd')), ('degenerate', dict(forced=False)),
                                          ('shared_best', dict(forced=False))],
                         ids=lambda v: v if isinstance(v, str) else '-'.join('%s=%s' % kv for kv in v.items()))
def test_golden_rejects_wrong_variants(case, variant):
    t = CASES[case]
    out = R.match_batch_ref(t['priors'], t['targets'], t['num_crowds'], **variant)
    assert not (torch.equal(out['conf_t'], t['conf_t']) and torch.equal(out['idx_t'], t['idx_t']))


def threshold_case():
    """Prior 0 is the unit square; the GT (0, 0, w, 1) overlaps it by exactly w for w = float32(0.4) and its two neighbours.
    Prior 1 = (0, 0, 0.5, 1) overlaps the GT more and takes the forced match, so prior 0 is judged by the thresholds alone."""
    priors = torch.tensor([[0.5, 0.5, 1.0, 1.0], [0.25, 0.5, 0.5, 1.0]])
    x = np.float32(0.4)
    ws = [np.nextafter(x, np.float32(0)), x, np.nextafter(x, np.float32(1))]
    targets = [torch.tensor([[0.0, 0.0, float(w), 1.0, 4.0]]) for w in ws]
    return priors, targets, ws


def test_thresholds_compare_in_fp32():
    priors, targets, ws = threshold_case()
    ov = torch.stack([R.iou(t[:, :4], R.point_form(priors))[0, 0] for t in targets])
    assert ov.dtype == torch.float32 and [float(v) for v in ov] == [float(w) for w in ws]
    # torch compares an fp32 tensor with a Python float in fp32: float32(0.4) is not below 0.4, its lower neighbour is
    assert (ov < 0.4).tolist() == [True, False, False]
    assert (ov < torch.tensor(0.4, dtype=torch.float32)).tolist() == [True, False, False]
    assert [bool(np.float32(v) < np.float32(0.4)) for v in ov.numpy()] == [True, False, False]
    out = R.match_batch_ref(priors, targets, [0, 0, 0])
    assert out['conf_t'][:, 0].tolist() == [0, -1, -1] and out['conf_t'][:, 1].tolist() == [5, 5, 5]
    # the crowd rule is a strict > against float32(0.7)
    r = torch.tensor([np.nextafter(np.float32(0.7), np.float32(0)), np.float32(0.7), np.nextafter(np.float32(0.7), np.float32(1))])
    assert (r > 0.7).tolist() == [False, False, True]


# ---- the C ABI and the Python surface, without a GPU -----------------------------------------------------------------------

def test_entries_are_exported_and_bound_at_abi_9():
    from yolact_amd import _lib as L
    lib = L.lib()
    assert lib.ymi_abi_version() == 9 and L.ABI_VERSION == 9
    assert {'ymi_match_f32', 'ymi_box_loss_f32'} <= {name for name, _, _ in L.SYMBOLS}
    assert lib.ymi_match_f32.argtypes[0] == ctypes.POINTER(L.MatchDesc)
    assert L.WS_MATCH == 17


def test_descriptor_matches_c_compiler(tmp_path):
    from yolact_amd import _lib as L
    fields = [f for f, _ in L.MatchDesc._fields_]
    src = tmp_path / 'sz.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu %%d"%s);'
                   % (os.path.join(ROOT, 'include', 'yolact_amd.h'), ',sizeof(ymi_match_desc),(int)YMI_WS_MATCH')
                   + ''.join('printf(" %%zu",offsetof(ymi_match_desc,%s));' % f for f in fields) + 'return 0;}')
    exe = tmp_path / 'sz'
    subprocess.run(['gcc', str(src), '-o', str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    D = L.MatchDesc
    assert got == [ctypes.sizeof(D), 17] + [getattr(D, f).offset for f in fields]
    assert ctypes.sizeof(D) == 18 * 8 + 8 * 4


POINTERS = ('priors', 'truth', 'label', 'gt_off', 'crowd', 'crowd_off', 'loc_data', 'loc_t', 'gt_box_t', 'conf_t', 'idx_t', 'pos',
            'num_pos', 'd_loc', 'loss', 'ws')
REQUIRED = ('priors', 'truth', 'label', 'gt_off', 'gt_off_host', 'loc_t', 'gt_box_t', 'conf_t', 'idx_t', 'pos', 'num_pos', 'ws')


def _desc(gt_vals=(0, 2, 5), crowd_vals=(0, 1, 1), **over):
    """Every device pointer set to an address nothing may touch: a launch would fault, a validation error returns."""
    from yolact_amd import _lib as L
    d = L.MatchDesc()
    for f in POINTERS:
        setattr(d, f, 16)
    keep = [(ctypes.c_int32 * len(gt_vals))(*gt_vals), (ctypes.c_int32 * len(crowd_vals))(*crowd_vals)]
    d.gt_off_host = ctypes.cast(keep[0], ctypes.c_void_p)
    d.crowd_off_host = ctypes.cast(keep[1], ctypes.c_void_p)
    d.B, d.P, d.G, d.Gc = 2, 300, 5, 1
    d.pos_thresh, d.neg_thresh, d.crowd_thresh, d.bbox_alpha = 0.5, 0.4, 0.7, 1.5
    for k, v in over.items():
        setattr(d, k, v)
    return d, keep


BAD = [({f: None}, -3) for f in REQUIRED] + [
    ({'crowd': None}, -3), ({'crowd_off': None}, -3), ({'crowd_off_host': None}, -3),
    ({'P': 0}, -1), ({'P': -5}, -1), ({'B': 0}, -1), ({'G': 0}, -1), ({'Gc': -1}, -1),
    ({'gt_off': (0, 0, 5)}, -1),                        # an image without a GT
    ({'gt_off': (0, 5, 5)}, -1),
    ({'gt_off': (0, 3, 5), 'P': 2}, -1),                # more GTs than priors
    ({'gt_off': (0, 6, 5)}, -1),                        # decreasing
    ({'gt_off': (1, 2, 5)}, -1), ({'gt_off': (0, 2, 4)}, -1),
    ({'crowd_off': (0, 2, 1)}, -1), ({'crowd_off': (0, 0, 0)}, -1),
    ({'loc_data': None}, -1),                           # d_loc and loss without loc_data
    ({'loc_data': None, 'loss': None}, -1), ({'loc_data': None, 'd_loc': None}, -1),
    ({'priors': 20}, -2), ({'ws': 24}, -2), ({'d_loc': 8}, -2),
]


@pytest.mark.parametrize('over,code', BAD, ids=lambda v: '-'.join('%s=%s' % kv for kv in v.items()) if isinstance(v, dict) else str(v))
def test_rejects_bad_descriptors_without_a_gpu(over, code):
    from yolact_amd import _lib as L
    offs = {k.replace('off', 'vals'): v for k, v in over.items() if isinstance(v, tuple)}     # tuples: the HOST offsets' values
    rest = {k: v for k, v in over.items() if not isinstance(v, tuple)}
    d, keep = _desc(**offs, **rest)
    assert L.lib().ymi_match_f32(ctypes.byref(d), None) == code
    assert L.lib().ymi_match_f32(None, None) == -3


def test_box_loss_entry_rejects_bad_arguments_without_a_gpu():
    from yolact_amd import _lib as L
    f = L.lib().ymi_box_loss_f32
    assert f(None, 16, 16, 2, 300, 1.5, 16, 16, 16, None) == -3 and f(16, 16, 16, 2, 300, 1.5, None, 16, 16, None) == -3
    assert f(16, 16, 16, 0, 300, 1.5, 16, 16, 16, None) == -1 and f(16, 16, 16, 2, 0, 1.5, 16, 16, 16, None) == -1
    assert f(16, 20, 16, 2, 300, 1.5, 16, 16, 16, None) == -2


def test_workspace_sizes():
    from yolact_amd import _lib as L
    def ws(what=None, **o):
        d, keep = _desc(**o)
        return L.lib().ymi_workspace_bytes(L.WS_MATCH if what is None else what, ctypes.byref(d))
    T = (19248 + 255) // 256
    assert ws(B=8, P=19248, G=96) >= 4 * (2 * T * 96 + 4 * 8 * 19248 + 2 * 96 + 2 * 8 * T)
    assert ws(B=8, P=19248, G=96) % 16 == 0 and ws(B=8, P=19248, G=200) > ws(B=8, P=19248, G=96)
    assert ws(P=0) == -1 and ws(B=0) == -1 and ws(G=0) == -1
    assert ws(L.WS_BOX_LOSS, B=8, P=19248) >= 2 * 4 * 8 * T and ws(L.WS_BOX_LOSS, P=0) == -1
    assert L.lib().ymi_workspace_bytes(L.WS_MATCH, None) == -3


@pytest.mark.parametrize('field,value', [('use_prediction_matching', True), ('use_change_matching', True),
                                         ('use_yolo_regressors', True), ('train_boxes', False)])
def test_every_unsupported_switch_names_its_field(monkeypatch, field, value):
    import yolact_amd
    cfg = yolact_amd.CONFIGS['yolact_base_config'].copy({field: value})
    with pytest.raises(NotImplementedError, match=field):
        M.check_switches(cfg)
    monkeypatch.setattr(M, 'active_cfg', lambda: cfg)
    t = CASES['plain3']
    with pytest.raises(NotImplementedError, match=field):
        M.match_targets(t['priors'], t['targets'], t['num_crowds'])
    with pytest.raises(NotImplementedError, match=field):
        M.box_loss(t['loc_data'], t['loc_t'], t['conf_t'] > 0)


def test_every_shipped_config_carries_the_reference_values():
    """data/config.py:443,553,600,620,698-701."""
    import yolact_amd
    for name, cfg in yolact_amd.CONFIGS.items():
        M.check_switches(cfg)
        assert (cfg.positive_iou_threshold, cfg.negative_iou_threshold, cfg.crowd_iou_threshold, cfg.bbox_alpha) == (0.5, 0.4, 0.7, 1.5), name
        assert cfg.train_boxes is True and cfg.use_prediction_matching is False and cfg.use_change_matching is False, name


def test_cpu_tensors_raise(monkeypatch):
    import yolact_amd
    from yolact_amd.layers import box_utils as BU
    cfg = yolact_amd.CONFIGS['yolact_base_config'].copy()
    monkeypatch.setattr(M, 'active_cfg', lambda: cfg)
    t = CASES['plain3']
    with pytest.raises(RuntimeError):
        M.match_targets(t['priors'], t['targets'], t['num_crowds'])
    with pytest.raises(RuntimeError):
        M.box_loss(t['loc_data'].clone().requires_grad_(True), t['loc_t'], t['conf_t'] > 0)
    tg = t['targets'][0]
    P = t['priors'].size(0)
    with pytest.raises(RuntimeError):
        BU.match(0.5, 0.4, tg[:, :4], t['priors'], tg[:, 4].long(), None, torch.zeros(1, P, 4), torch.zeros(1, P).long(),
                 torch.zeros(1, P).long(), 0, t['loc_data'][0])
    assert issubclass(M.LC.LossFunction, torch.autograd.Function)


def test_shim_re_exports_encode_and_match():
    src = open(os.path.join(ROOT, 'shim', 'layers', 'box_utils.py')).read()
    assert ' encode,' in src and ' match,' in src
