"""The merged P4..P7 prediction heads (ymi_wino_desc.nlev) on the host: the virtual table key, the shipped entries, and the op-list
surgery of PlanTuning.install_level_merge on a dry CPU plan.  No GPU."""
import ctypes

import pytest
import torch

from yolact_amd import _lib as L
from yolact_amd import tune_table as TT


def _plan(config='yolact_resnet50_config', B=2, size=550):
    import yolact_amd
    yolact_amd.set_cfg(config)
    from yolact_amd.engine import Plan
    from yolact_amd.yolact import Yolact
    return Plan(Yolact(), B, size, size, torch.device('cpu'))


def _heads(plan):
    return [(fn if isinstance(fn, str) else fn.__name__, name) for fn, _, name, _ in plan.ops if name.startswith('head')]


def test_virtual_key_round_trips():
    key = TT.level_key(8, 119, 256, 360, L.ACT_NONE, 3, 'h2')
    assert key == 'wino(8, 476, 4, 256, 360, 0, 3, (4,))|h2'
    assert TT.parse(key) == ('wino', (8, 476, 4, 256, 360, 0, 3, (4,)), 'h2')
    assert TT.format(*TT.parse(key)) == key
    assert TT.wino_parts(TT.wino_choice(L.TILE_128x128 | L.TILE_H2, planes=1)) == (L.TILE_128x128 | L.TILE_H2, 1)


# (config, batch, size, F(4x4) tiles per image over P4..P7, head Cout): the shapes bench.py can run
SHIPPED = [('yolact_resnet50_config', 8, 550, 119, 360), ('yolact_resnet50_config', 1, 550, 119, 360),
           ('yolact_base_config', 16, 550, 119, 360), ('yolact_im700_config', 8, 700, 170, 360),
           ('yolact_plus_resnet50_config', 8, 550, 119, 1080)]


@pytest.mark.parametrize('config,B,size,tiles,chead', SHIPPED, ids=['%s-b%d' % (c[0][7:-7], c[1]) for c in SHIPPED])
def test_shipped_table_holds_the_merged_entries(config, B, size, tiles, chead):
    table = TT.read_table_file(TT.os.path.join(TT.TUNE_DIR, 'gfx950.json'))
    for key in (TT.level_key(B, tiles, 256, 256, L.ACT_RELU, 0, 'h2'), TT.level_key(B, tiles, 256, chead, L.ACT_NONE, 3, 'h2')):
        assert key in table, key
        m, choice, t_levels, t_merged, _, t_f4 = table[key]
        tile, planes = TT.wino_parts(choice)
        assert m == 4 and tile & L.TILE_H2 and planes in (0, 1) and 0.0 < t_merged == t_f4 < t_levels


def test_tiles_per_image_of_the_shipped_keys_are_the_plans_own():
    plan = _plan()
    assert plan.level_merge['tiles'] == 81 + 25 + 9 + 4 == 119
    assert plan.level_merge_keys() == (TT.level_key(2, 119, 256, 256, L.ACT_RELU, 0, 'h2'), TT.level_key(2, 119, 256, 360, L.ACT_NONE, 3, 'h2'))


def test_untuned_plan_is_unchanged():
    plan = _plan()
    heads = _heads(plan)
    assert not plan.merged_levels
    assert [n for _, n in heads] == ['head0.up0+proto.0', 'head0.out'] + ['head%d.%s' % (l, w) for l in range(1, 5) for w in ('up0', 'out')]
    assert all(fn == 'ymi_conv2d_nhwc_f32' for fn, _ in heads)
    assert len([d for n, d in plan.conv_meta if n.endswith('.out')]) == 5


def test_forced_merge_leaves_nops_and_kind12_positions():
    plan = _plan()
    meta = [n for n, _ in plan.conv_meta]
    n_ops = len(plan.ops)
    assert plan.install_level_merge([TT.wino_choice(L.TILE_128x128 | L.TILE_H2, planes=1)] * 2)
    assert plan.merged_levels and len(plan.ops) == n_ops and [n for n, _ in plan.conv_meta] == meta
    heads = _heads(plan)[2:]
    assert [fn for fn, _ in heads] == ['ymi_conv3x3_winograd_f32'] * 2 + ['nop'] * 6
    assert heads[0][1].startswith('head1.up0') and heads[1][1].startswith('head1.out')
    assert [n.split('[')[0] for _, n in heads[2:]] == ['head%d.%s' % (l, w) for l in (2, 3, 4) for w in ('up0', 'out')]
    du, do = plan.level_merge['descs']
    assert (du.nlev, du.nabs, du.nseg, du.m) == (4, 0, 0, 4) and (do.nlev, do.nabs, do.nseg, do.m) == (4, 6, 3, 4)
    assert [(du.lev[q].H, du.lev[q].W) for q in range(4)] == [(35, 35), (18, 18), (9, 9), (5, 5)]
    # records map onto conv_meta by position: head1.up0 and head1.out carry the launches, the six entries behind them are the
    # absorbed layers, in conv_meta order, each with its own algorithmic FLOPs
    i = meta.index('head1.out')
    assert meta[i - 1] == 'head1.up0' and meta[i + 1:i + 7] == ['head%d.%s' % (l, w) for l in (2, 3, 4) for w in ('up0', 'out')]
    flops = [plan.lib.ymi_conv_flops(ctypes.byref(d)) for _, d in plan.conv_meta[i + 1:i + 7]]
    assert list(do.abs_flops)[:6] == flops and all(f > 0 for f in flops)
    # level l of the merged .out launch writes where head l's own launch wrote
    for q, l in enumerate((1, 2, 3, 4)):
        own = dict(plan.conv_meta)['head%d.out' % l]
        for k in range(3):
            assert do.seg[k].ptr + do.lev[q].seg_off[k] == own.seg[k].ptr
    assert plan._native_plan() is not None
    assert plan.install_level_merge() is True         # idempotent
