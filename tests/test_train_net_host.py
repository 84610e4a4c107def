"""The composed training-step oracle (tests/train_net_ref.py) on the host: it is what the reference computes, its two cases are what
they claim to be, and the bars of tests/test_gpu_train_grads.py tell a right wiring from a wrong one.  No GPU.

The reference.  tests/golden/train_grads.npz (tools/make_golden_train_grads.py) holds what the reference's own train-mode Yolact and
MultiBoxLoss computed in fp64 on both cases: the losses, and numel, sum, L2 norm and 64 values of every parameter gradient and every
running statistic after the step.  Both sides are fp64 evaluations of the same formula.  Measured largest relative deviation (losses
against their value, sums against norm * sqrt(numel), norms against the norm, values against the tensor's root mean square): 2.6e-12
on 'stats', 3.7e-13 on 'frozen'.  REFERENCE_BAR = 3e-10 is 100 times the larger: under the 1e-8 it may never exceed and far under
fp32's 6e-8, so one fp32 step on either side shows.

The wrong variants (train_net_ref.WRONG).  Each is measured against the right fp64 oracle with the metric and the bar the GPU test
uses for that parameter (train_helpers.compare's max-norm rule above the backbone, rel. L2 against the section's bar in the backbone)
and in rel. L2 as well; on at least one parameter the smaller of the two must be at least 4 times the bar.  Every variant clears that
(the figures: test_the_bars_tell_right_from_wrong).  The two that show in the backbone only, 'lateral' and 'bn_xhat', do so by 9 to
18 times the bar, not by thousands: the backbone's bars are 0.04 to 0.07, four times what ReLU and max-pool flips make two fp32
evaluations differ by, and a wiring error that changes a stage's gradients by less than about a quarter would pass there.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heads_train_ref as H  # noqa: E402
import helpers  # noqa: E402
import train_net_ref as N  # noqa: E402
import train_step_ref as T  # noqa: E402
import yolact_amd  # noqa: E402

REFERENCE_BAR = 3e-10
EXACT_BAR = 8e-6                 # tests/train_helpers.EXACT_BAR (that module needs the GPU library to import)
F64, F32 = torch.float64, torch.float32


@pytest.fixture(scope='module', autouse=True)
def _cfg():
    saved = yolact_amd.config.cfg.copy()
    yield
    yolact_amd.config.cfg.replace(saved)


@functools.lru_cache(maxsize=None)
def report(name):
    return T.grads_case_report(name)


def param_bars(name):
    """{parameter: (metric, bar)} as tests/test_gpu_train_grads.py sets them, from the two oracles alone."""
    rep = report(name)
    g64, g32 = rep['res'][F64]['grads'], rep['res'][F32]['grads']
    noise = N.section_noise(g32, g64)
    bars = {}
    for n in g64:
        s = N.section_of(n)
        if s is None:
            bars[n] = (helpers.rel_err, max(4 * helpers.rel_err(g32[n], g64[n]), EXACT_BAR))
        else:
            bars[n] = (N.rel_l2, max(4 * noise[s], EXACT_BAR))
    return bars


@pytest.mark.parametrize('name', T.GRADS_CASES)
def test_the_case_is_what_the_search_asked_for(name):
    rep = report(name)
    print(rep['line'])
    assert min(rep['pos_per_level']) >= 1, rep['pos_per_level']                     # a positive prior on each of P3 .. P7 (match_ref)
    grads = rep['res'][F64]['grads']
    assert rep['zero'] == []
    for n in ('fpn.downsample_layers.0.weight', 'fpn.downsample_layers.0.bias', 'fpn.downsample_layers.1.weight',
              'fpn.downsample_layers.1.bias'):
        assert bool(grads[n].ne(0).any()), n
    trained = [n for n, p in T.build_grads_case('cpu', name)[0].named_parameters() if p.requires_grad]
    assert sorted(trained) == sorted(grads)
    affine = [n for n in rep['inputs']['state'] if N.is_bn_affine(n)]
    assert len(affine) == 2 * 53 and all((n in grads) == (name == 'stats') for n in affine)
    assert len(rep['margins']) == 3 + 5 + 5                                          # FPN, protonet, the head on five levels
    H.assert_margins(rep['margins'], factor=16)
    assert rep['gap'] >= 1e-3                                                        # as tests/test_gpu_multibox.py asks
    assert rep['same_match'] and rep['same_neg']
    assert 'failed []' in rep['line'] and rep['failed'] == []


def test_frozen_is_stats_with_the_batch_s_own_statistics():
    a, b = report('stats')['inputs'], report('frozen')['inputs']
    assert a['batch_stats'] is True and b['batch_stats'] is False and b['train_bn_affine'] is False
    for n, t in a['state'].items():
        if N.is_stat(n):
            assert not torch.equal(t, b['state'][n]), n
        else:
            assert torch.equal(t, b['state'][n]), n
    new = report('stats')['res'][F64]['new_stats']
    for n in new:                                  # momentum 0.1 of the way from the seeded statistic to the calibrated one
        want = 0.9 * a['state'][n].double() + 0.1 * b['state'][n].double()
        assert helpers.rel_err(new[n], want) <= 1e-6, n
    assert sorted(new) == sorted(n for n in a['state'] if N.is_stat(n))
    for n, t in report('frozen')['res'][F64]['new_stats'].items():
        assert torch.equal(t, b['state'][n].double()), n


def deviations(name):
    """The fp64 oracle against the reference's digest -> [(relative deviation, what)]."""
    meta, z = helpers.load_golden('train_grads')
    res = report(name)['res'][F64]
    out = []
    for i, k in enumerate('BMCS'):
        want = float(z[name + '_losses'][i])
        out.append((abs(float(res['losses'][k]) - want) / abs(want), 'loss ' + k))
    names = meta['cases'][name]['names']
    assert sorted(n for kind, n in names if kind == 'grad') == sorted(res['grads'])
    assert sorted(n for kind, n in names if kind == 'stat') == sorted(res['new_stats'])
    for row, (kind, n) in enumerate(names):
        t = (res['grads'] if kind == 'grad' else res['new_stats'])[n].double().reshape(-1)
        numel, s, l2 = z[name + '_rows'][row]
        assert t.numel() == int(numel) and l2 > 0, n
        rms = l2 / numel ** 0.5
        v = t[torch.from_numpy(T.digest_indices(row, t.numel()))].numpy()
        out += [(abs(float(t.sum()) - s) / (l2 * numel ** 0.5), n + ' sum'), (abs(float(t.norm()) - l2) / l2, n + ' norm'),
                (float(np.abs(v - z[name + '_vals'][row]).max()) / rms, n + ' values')]
    return out


@pytest.mark.parametrize('name', T.GRADS_CASES)
def test_the_oracle_is_the_reference(name):
    dev = deviations(name)
    worst = max(dev)
    print('%s: the largest relative deviation from the reference in fp64 is %.3e (%s), the bar %.1e' % (name, worst[0], worst[1],
                                                                                                       REFERENCE_BAR))
    assert REFERENCE_BAR <= 1e-8
    for e, what in dev:
        assert e <= REFERENCE_BAR, (what, e)
    meta, z = helpers.load_golden('train_grads')
    noise = {n: float(v) for (kind, n), v in zip(meta['cases'][name]['names'], z[name + '_noise']) if kind == 'grad'}
    print('the reference\'s own fp32-versus-fp64 rel. L2: at most %.3e in the backbone, %.3e above it' % (
        max(v for n, v in noise.items() if N.section_of(n)), max(v for n, v in noise.items() if not N.section_of(n))))


VARIANTS = [(w, c) for c in T.GRADS_CASES for w in N.WRONG if not (w == 'bn_xhat' and c == 'frozen')]


@pytest.mark.parametrize('wrong,name', VARIANTS)
def test_the_bars_tell_right_from_wrong(wrong, name):
    """Measured: the ratio to the bar on the parameter that shows the variant best, and how many parameters reach 4.
    stats:  lateral 13.3 (layers.2.5.bn3.bias; 129 parameters), head4 5.1e+4 (8), p67 1.9e+4 (4), s_norm 1.0e+5 (169),
            bn_xhat 17.8 (layers.0.0.bn1.weight; 155), proto_m 1.3e+5 (21)
    frozen: lateral 9.4 (layers.2.5.conv3.weight; 43), head4 5.3e+4 (8), p67 1.3e+4 (4), s_norm 1.0e+5 (63), proto_m 1.3e+5 (18)"""
    rep = report(name)
    right = rep['res'][F64]
    res = N.train_ref(dtype=F64, wrong=wrong, **rep['inputs'])
    bars = param_bars(name)
    assert sorted(res['grads']) == sorted(bars)
    for k in 'BMC' if wrong == 's_norm' else 'BMCS':                     # every variant is a wiring error: the forward is right
        assert float(res['losses'][k]) == float(right['losses'][k]), k
    ratios = {}
    for n, (metric, bar) in bars.items():
        ratios[n] = min(metric(res['grads'][n], right['grads'][n]), N.rel_l2(res['grads'][n], right['grads'][n])) / bar
    best = max(ratios, key=ratios.get)
    print('%s %s: %d of %d parameters at 4 x their bar or more; the clearest %s at %.3e x its bar %.3e' % (
        name, wrong, sum(r >= 4 for r in ratios.values()), len(ratios), best, ratios[best], bars[best][1]))
    assert ratios[best] >= 4, (best, ratios[best])
