"""The OHEM class loss 'C' on the CPU: tests/class_loss_ref.py is pinned to what the reference's own ohem_conf_loss computed
(tests/golden/multibox.npz, written by tools/make_golden_multibox.py), shown to tell wrong variants apart, and the C ABI / Python
surface of ymi_class_loss_f32 is checked as far as that goes without a GPU.

Golden bars: neg and n exact; 'C' and d C / d conf relative error <= 1e-6 (both sides are fp32 on the CPU).
"""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import class_loss_ref as R  # noqa: E402
import yolact_amd.layers.class_loss as CL  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
META, G = R.load_golden()
GOLDEN_BAR = 1e-6
CASES = ['ohemA', 'ohemB']


def case(name):
    return G[name + '_conf'].float(), G[name + '_conf_t'].long()


def test_golden_holds_the_cases_the_kernel_can_get_wrong():
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'multibox.npz')) < 256 * 1024
    P = META['P']
    ct = G['ohemA_conf_t']
    assert (ct[0] < 0).sum() == 12 and (ct[0] > 0).sum() == 9            # neutrals
    assert (ct[1] > 0).sum() == 0 and G['ohemA_n'].tolist() == [27, 0]  # an image without positives
    assert not G['ohemA_neg'][1].any() and not G['ohemA_d_conf'][1].any()
    assert G['ohemB_n'].tolist() == [P - 1] and 3 * int((G['ohemB_conf_t'] > 0).sum()) > P - 1      # clamped
    for name in CASES + ['fwd']:
        assert G[name + '_conf'].float().abs().max() <= 8.25
    for name in CASES:                                                  # the cut of every image is open on the oracle's keys
        conf, ct = case(name)
        r = R.ohem_ref(conf.double(), ct, META['negpos_ratio'])
        assert min(R.cut_gaps(r['key'], r['n'])) >= META['gap']


@pytest.mark.parametrize('name', CASES)
def test_ref_equals_the_reference(name):
    conf, ct = case(name)
    r = R.ohem_ref(conf, ct, META['negpos_ratio'], META['conf_alpha'])
    assert torch.equal(r['neg'], G[name + '_neg'].bool()) and torch.equal(r['n'].int(), G[name + '_n'])
    errs = (R.rel_err(r['loss'].view(1), G[name + '_C']), R.rel_err(r['d_conf'], G[name + '_d_conf']))
    print('%s: C %.3e d_conf %.3e' % ((name,) + errs))
    assert max(errs) <= GOLDEN_BAR, errs
    off = ~(r['neg'] | (ct > 0))
    assert not G[name + '_d_conf'][off].any() and not r['d_conf'][off].any()


@pytest.mark.parametrize('name,variant', [('ohemB', dict(ratio_after_clamp=True)), ('ohemA', dict(mine_neutrals=True)),
                                          ('ohemA', dict(zero_pos=False)), ('ohemA', dict(key='max_softmax'))],
                         ids=lambda v: v if isinstance(v, str) else '-'.join('%s=%s' % kv for kv in v.items()))
def test_golden_rejects_wrong_variants(name, variant):
    conf, ct = case(name)
    r = R.ohem_ref(conf, ct, META['negpos_ratio'], META['conf_alpha'], **variant)
    assert not (torch.equal(r['neg'], G[name + '_neg'].bool()) and torch.equal(r['n'].int(), G[name + '_n']))


def test_ties_go_to_the_lowest_prior_and_the_key_is_finite_far_below_the_batch_maximum():
    g = torch.Generator().manual_seed(3)
    conf = torch.randn(1, 40, 5, generator=g)
    conf[0, 10:30] = conf[0, 10]                                        # 20 equal keys
    ct = torch.zeros(1, 40, dtype=torch.long)
    ct[0, :3] = 1
    conf[0, 10:30, 0] -= 4                                              # the tie group outranks every other negative
    r = R.ohem_ref(conf.double(), ct, 3)
    assert r['neg'][0].nonzero().view(-1).tolist() == list(range(10, 19))
    conf[0, 39] -= 200                                                  # the reference's global maximum would give log 0 here
    assert torch.isfinite(R.ohem_ref(conf, ct, 3)['key']).all()


# ---- the C ABI and the Python surface, without a GPU -----------------------------------------------------------------------

def test_entries_are_exported_and_bound_at_abi_9():
    from yolact_amd import _lib as L
    lib = L.lib()
    assert lib.ymi_abi_version() == 9 and L.ABI_VERSION == 9
    assert 'ymi_class_loss_f32' in {name for name, _, _ in L.SYMBOLS}
    assert lib.ymi_class_loss_f32.argtypes[0] == ctypes.POINTER(L.ClassLossDesc)
    assert L.WS_CLASS_LOSS == 19


def test_descriptor_matches_c_compiler(tmp_path):
    from yolact_amd import _lib as L
    fields = [f for f, _ in L.ClassLossDesc._fields_]
    src = tmp_path / 'sz.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu %%d"%s);'
                   % (os.path.join(ROOT, 'include', 'yolact_amd.h'), ',sizeof(ymi_class_loss_desc),(int)YMI_WS_CLASS_LOSS')
                   + ''.join('printf(" %%zu",offsetof(ymi_class_loss_desc,%s));' % f for f in fields) + 'return 0;}')
    exe = tmp_path / 'sz'
    subprocess.run(['gcc', str(src), '-o', str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    D = L.ClassLossDesc
    assert got == [ctypes.sizeof(D), 19] + [getattr(D, f).offset for f in fields]
    assert ctypes.sizeof(D) == 7 * 8 + 6 * 4


POINTERS = ('conf', 'conf_t', 'loss', 'neg', 'num_neg', 'd_conf', 'ws')
REQUIRED = ('conf', 'conf_t', 'loss', 'neg', 'num_neg', 'ws')


def _desc(**over):
    """Every device pointer set to an address nothing may touch: a launch would fault, a validation error returns."""
    from yolact_amd import _lib as L
    d = L.ClassLossDesc()
    for f in POINTERS:
        setattr(d, f, 16)
    d.B, d.P, d.C, d.negpos_ratio, d.conf_alpha = 2, 300, 81, 3, 1.0
    for k, v in over.items():
        setattr(d, k, v)
    return d


BAD = [({f: None}, -3) for f in REQUIRED] + [
    ({'B': 0}, -1), ({'B': 65536}, -1), ({'P': 1}, -1), ({'P': -4}, -1), ({'C': 1}, -1), ({'C': 257}, -1), ({'negpos_ratio': -1}, -1),
    ({'B': 8, 'P': 1 << 20, 'C': 256}, -2),                             # B P C = 2^31
    ({'conf': 20}, -2), ({'d_conf': 24}, -2), ({'ws': 8}, -2),
]


@pytest.mark.parametrize('over,code', BAD, ids=lambda v: '-'.join('%s=%s' % kv for kv in v.items()) if isinstance(v, dict) else str(v))
def test_rejects_bad_descriptors_without_a_gpu(over, code):
    from yolact_amd import _lib as L
    assert L.lib().ymi_class_loss_f32(ctypes.byref(_desc(**over)), None) == code
    assert L.lib().ymi_class_loss_f32(None, None) == -3


def test_workspace_sizes():
    from yolact_amd import _lib as L
    ws = lambda **o: L.lib().ymi_workspace_bytes(L.WS_CLASS_LOSS, ctypes.byref(_desc(**o)))
    pad = lambda n: (4 * n + 15) // 16 * 16
    T = (19248 + 127) // 128                                            # C = 81: 128 rows of stride 81 per tile
    assert ws(B=8, P=19248, C=81) == 2 * pad(8 * 19248) + 2 * pad(8 * T)
    T4 = (345 + 127) // 128
    assert ws(B=3, P=345, C=4) == 2 * pad(3 * 345) + 2 * pad(3 * T4)
    R256 = 10752 // 257                                                 # C = 256: stride 257, 41 rows per tile
    assert ws(B=1, P=1000, C=256) == 2 * pad(1000) + 2 * pad((1000 + R256 - 1) // R256)
    assert ws(P=1) == -1 and ws(B=0) == -1 and ws(C=300) == -1 and ws(B=8, P=1 << 20, C=256) == -2
    assert L.lib().ymi_workspace_bytes(L.WS_CLASS_LOSS, None) == -3


@pytest.mark.parametrize('field', ['use_focal_loss', 'use_sigmoid_focal_loss', 'use_objectness_score', 'ohem_use_most_confident',
                                   'use_class_balanced_conf'])
def test_every_unsupported_switch_names_its_field(monkeypatch, field):
    import yolact_amd
    cfg = yolact_amd.CONFIGS['yolact_base_config'].copy({field: True})
    with pytest.raises(NotImplementedError, match=field):
        CL.check_switches(cfg)
    monkeypatch.setattr(CL, 'active_cfg', lambda: cfg)
    conf, ct = case('ohemB')
    with pytest.raises(NotImplementedError, match=field):
        CL.ohem_conf_loss(conf, ct)
    with pytest.raises(NotImplementedError, match=field):
        CL.ohem_terms(conf, ct)


def test_every_shipped_config_carries_the_reference_values():
    """data/config.py:442,517,528,574."""
    import yolact_amd
    for name, cfg in yolact_amd.CONFIGS.items():
        CL.check_switches(cfg)
        assert (cfg.conf_alpha, cfg.ohem_negpos_ratio) == (1, 3), name


def test_cpu_tensors_raise(monkeypatch):
    import yolact_amd
    cfg = yolact_amd.CONFIGS['yolact_base_config'].copy()
    monkeypatch.setattr(CL, 'active_cfg', lambda: cfg)
    conf, ct = case('ohemB')
    with pytest.raises(RuntimeError):
        CL.ohem_conf_loss(conf.clone().requires_grad_(True), ct)
    with pytest.raises(RuntimeError):
        CL.ohem_terms(conf, ct)
    assert issubclass(CL.LC.LossFunction, torch.autograd.Function)
