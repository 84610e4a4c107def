"""yolact_amd/tune_table.py (the one codec of the tile table's keys and values) and what the plan tuner of yolact_amd/plan_tune.py
would measure — no GPU needed, except for the last test, which runs the measure-on-miss path of Plan.tune() on the device.

The literal key expressions below are the SPECIFICATION of the key format: they are what engine.Plan built by string concatenation
before the codec existed, and what yolact_amd/tune/gfx950.json is keyed by.
"""
import ast
import functools
import importlib.util
import json
import os

import pytest

from yolact_amd import _lib as L
from yolact_amd import tune_table as TT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'yolact_amd')
with open(os.path.join(PKG, 'tune', 'gfx950.json')) as _f:
    SHIPPED = json.load(_f)['entries']

_spec = importlib.util.spec_from_file_location('make_golden_tune_candidates', os.path.join(ROOT, 'tools', 'make_golden_tune_candidates.py'))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)
# (config, size, batch) of the dry plans: the five configurations of tests/test_plan_schedule.py at batch 1 and 8.  On every one of
# them each convolution / DCN key is in the shipped table (checked before the codec existed; bench.py's zero-miss contract is
# yolact_resnet50_config at batch 8)
PLANS = [(config, size, B) for config, size in G.CASES for B in G.BATCHES]
ALL_IN_TABLE = list(PLANS)


@functools.lru_cache(maxsize=None)
def _plan(config, size, B):
    return G.dry_plan(config, size, B)


# ---- keys ------------------------------------------------------------------------------------------------------------------------
def test_every_shipped_key_round_trips():
    assert len(SHIPPED) >= 971
    kinds = set()
    for k in SHIPPED:
        kind, t, mode = TT.parse(k)
        assert TT.format(kind, t, mode) == k
        assert kind in TT.KINDS and mode in TT.MODES
        kinds.add(kind)
    assert kinds == {'conv', 'dcn', 'wino', 'chain', 'chain1', 'chainx'}


def test_constructors_reproduce_literal_keys():
    shape = (8, 138, 138, 256, 128, 1, 1, 1, 0, 0, 1, 256)
    assert TT.conv_key(shape) == '(8, 138, 138, 256, 128, 1, 1, 1, 0, 0, 1, 256)'
    assert TT.conv_key(shape, 'h2') == '(8, 138, 138, 256, 128, 1, 1, 1, 0, 0, 1, 256)|h2'
    assert TT.conv_key(shape, 'x3') == '(8, 138, 138, 256, 128, 1, 1, 1, 0, 0, 1, 256)|x3'
    assert TT.conv_key((1, 69, 69, 128, 128, 3, 3, 1, 1, 0, 1, 1152), 'h2', dcn=True) == "(1, 69, 69, 128, 128, 3, 3, 1, 1, 0, 1, 1152, 'dcn')|h2"
    assert TT.wino_key(8, 69, 69, 256, 256, 1, 0, (2, 4), 'h2') == 'wino(8, 69, 69, 256, 256, 1, 0, (2, 4))|h2'
    assert TT.wino_key(1, 35, 35, 256, 256, 1, 3, [4]) == 'wino(1, 35, 35, 256, 256, 1, 3, (4,))'
    assert TT.chain_key('chain', 8, 138, 138, mode='h2') == 'chain(8, 138, 138)|h2'
    assert TT.chain_key('chain1', 8, 138, 138, mode='h2') == 'chain1(8, 138, 138)|h2'
    assert TT.chain_key('chain', 8, 69, 69, 128, 'h2') == 'chain(8, 69, 69, 128)|h2'                 # (csrc/chain2.hip, opt-in: not in the shipped table)
    assert TT.chainx_key(8, 138, 138, 'h2') == 'chainx(8, 138, 138)|h2'
    assert TT.instep_key('wino(8, 69, 69, 256, 256, 1, 0, (2, 4))|h2') == 'instep|wino(8, 69, 69, 256, 256, 1, 0, (2, 4))|h2'   # (tools/instep_tune.py)
    assert TT.parse("(1, 69, 69, 128, 128, 3, 3, 1, 1, 0, 1, 1152, 'dcn')|h2") == ('dcn', (1, 69, 69, 128, 128, 3, 3, 1, 1, 0, 1, 1152, 'dcn'), 'h2')
    assert TT.parse('chain(8, 69, 69, 128)|h2') == ('chain', (8, 69, 69, 128), 'h2')
    assert TT.parse('instep|wino(8, 69, 69, 256, 256, 1, 0, (2, 4))|x3') == ('instep', (8, 69, 69, 256, 256, 1, 0, (2, 4)), 'x3')
    for k in ('chain(8, 69, 69, 128)|h2', 'instep|wino(8, 69, 69, 256, 256, 1, 0, (2, 4))|h2', 'chainx(2, 138, 138)', '(1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12)|x3'):
        assert TT.format(*TT.parse(k)) == k
    for k in SHIPPED:                                           # every constructor against every shipped key of its kind
        kind, t, mode = TT.parse(k)
        made = {'conv': lambda: TT.conv_key(t, mode), 'dcn': lambda: TT.conv_key(t[:12], mode, dcn=True), 'wino': lambda: TT.wino_key(*t, mode=mode),
                'chain': lambda: TT.chain_key('chain', *t, mode=mode), 'chain1': lambda: TT.chain_key('chain1', *t, mode=mode),
                'chainx': lambda: TT.chainx_key(*t, mode=mode)}[kind]()
        assert made == k


@pytest.mark.parametrize('key', [
    '', '()', '(1, 2)', '(1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11)|h2', '(1,2,3,4,5,6,7,8,9,10,11,12)', '(1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12)|h3',
    '(1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12)|', '(1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12)|h2 ', '(1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12.0)',
    '(1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, True)', "(1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 'dcx')|h2", "(1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 'dcn')",
    'wino(1, 2, 3)|h2', 'wino(8, 69, 69, 256, 256, 1, 0, 2)|h2', 'wino(8, 69, 69, 256, 256, 1, 0, (2, 4, 6))', 'wino(8, 69, 69, 256, 256, 1, 0, ())',
    'chain(1, 2)', 'chain(1, 2, 3, 4, 5)', 'chainx(1, 2, 3, 4)|h2', 'chain2(1, 2, 3)', 'conv(1, 2, 3)', 'instep|chain(1, 2, 3)',
    'instep|(1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12)', 'instep|instep|wino(8, 69, 69, 256, 256, 1, 0, (2, 4))', 'wino|(1, 2, 3)',
    'chain(1, 2, __import__("os"))', 'chain[1, 2, 3]', 'chain(1, 2, 3', None, 7, ('chain', 1, 2, 3)])
def test_malformed_keys_raise(key):
    with pytest.raises(ValueError):
        TT.parse(key)


def test_malformed_fields_raise():
    for call in (lambda: TT.conv_key((1, 2, 3)), lambda: TT.conv_key(tuple(range(12)), '|h2'), lambda: TT.chain_key('chainx', 1, 2, 3),
                 lambda: TT.chain_key('chain', 1, 2, 3.0), lambda: TT.wino_key(1, 2, 3, 4, 5, 6, 7, (8,), 'fp32'), lambda: TT.instep_key('chain(1, 2, 3)'),
                 lambda: TT.format('instep', (1, 2, 3)), lambda: TT.format('tile', (1, 2, 3))):
        with pytest.raises(ValueError):
            call()


# ---- values ----------------------------------------------------------------------------------------------------------------------
def test_value_codec_agrees_with_the_packing_of_the_shipped_values():
    splits, planes = set(), set()
    for k, v in SHIPPED.items():
        kind = TT.parse(k)[0]
        if kind in ('conv', 'dcn'):
            tile, S = TT.direct_parts(v)
            assert (tile, S) == (v & 255, v >> 8) and tile in L.TILE_NAMES
            assert TT.direct_choice(tile, S) == v == tile + 256 * S
            assert TT.choice_name(v) == L.TILE_NAMES[v & 255] + ('/k%d' % (v >> 8) if v >> 8 else '')
            splits.add(S)
        elif kind == 'wino':
            tile, p = TT.wino_parts(v[1])
            assert (tile, p) == (int(v[1]) & 255, 1 if int(v[1]) & L.WINO_PLANES else 0)
            assert TT.wino_choice(tile, p) == v[1]
            assert tile in L.TILE_NAMES if v[0] else v[1] == 0
            planes.add(p)
    assert splits == {0, 2, 3, 4, 5, 6, 8, 9, 12, 16} and planes == {0, 1}
    assert TT.direct_choice(3, 1) == 3 == TT.direct_choice(3, 0) and TT.direct_parts(3 + 256 * 16) == (3, 16)
    assert TT.choice_name(L.TILE_64x64 + 256 * 4) == '64x64/k4' and TT.choice_name(L.TILE_128x64 | L.TILE_H2) == '128x64h2'


# ---- the keys and candidates of dry plans ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('config,size,B', PLANS, ids=['%s-B%d' % (c, b) for c, _, b in PLANS])
def test_plan_keys_equal_the_literal_expression(config, size, B):
    plan = _plan(config, size, B)
    n = 0
    for opi, (fn, dptr, name, where) in enumerate(plan.ops):
        is_dcn = fn is plan.lib.ymi_dcn_v2_forward_f32
        if fn is not plan.lib.ymi_conv2d_nhwc_f32 and not is_dcn:
            continue
        d = dptr.contents.conv if is_dcn else dptr.contents
        for wide in (opi in plan.wide_ops, True):               # (the second: the key this layer would get under the outlier guard)
            key = (d.B, d.H, d.W, d.Cin, d.Cout, d.kh, d.kw, d.stride, d.pad, d.res_mode, d.nseg, d.Kpad) + (('dcn',) if is_dcn else ())
            h2_, split_ = plan.h2 and not wide, plan.split or (wide and not is_dcn)
            skey = str(key) + ('|x3' if split_ else '|h2' if h2_ else '')
            assert plan.direct_key(fn, d, wide) == skey, name
            assert TT.parse(skey) == ('dcn' if is_dcn else 'conv', key, skey.partition('|')[2])
        if (config, size, B) in ALL_IN_TABLE:
            assert plan.direct_key(fn, d, opi in plan.wide_ops) in SHIPPED, (name, skey)
        n += 1
    assert n >= 70


def test_tuner_candidates_reproduce_the_recorded_ones():
    """tests/golden/tune_candidates.json (tools/make_golden_tune_candidates.py) was recorded with the tuner still inside engine.Plan:
    the candidate lists of every distinct key, order included (order decides ties), and the stage-exit candidates of every plan."""
    assert TT.build_meta().get('lint', 'ok') == 'ok', 'recorded on a build whose ISA lint ran (the patch tile is a candidate)'
    with open(os.path.join(ROOT, 'tests', 'golden', 'tune_candidates.json')) as f:
        want = json.load(f)
    got = G.collect(('%s/B%d' % (c, b), _plan(c, s, b)) for c, s, b in PLANS)
    assert sorted(got['direct_candidates']) == sorted(want['direct_candidates'])
    for k in want['direct_candidates']:
        assert got['direct_candidates'][k] == want['direct_candidates'][k], k
    assert got['stage_exit_candidates'] == want['stage_exit_candidates']
    assert len(want['direct_candidates']) >= 200 and sum(len(v) for v in want['stage_exit_candidates'].values()) == 8
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'tune_candidates.json')) < 256 * 1024


def test_tuner_modules_do_not_import_the_engine():
    for mod in ('tune_table.py', 'plan_tune.py'):
        with open(os.path.join(PKG, mod)) as f:
            tree = ast.parse(f.read())
        for node in ast.walk(tree):
            names = [a.name for a in node.names] if isinstance(node, (ast.Import, ast.ImportFrom)) else []
            names += [node.module or ''] if isinstance(node, ast.ImportFrom) else []
            assert not any(n.split('.')[-1] == 'engine' for n in names), (mod, node.lineno)
    from yolact_amd.engine import Plan
    from yolact_amd.plan_tune import PlanTuning
    assert issubclass(Plan, PlanTuning)


# ---- the measure-on-miss path, on the device -------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_unknown_shapes_are_measured_persisted_and_replayed(tmp_path, monkeypatch):
    """yolact_resnet50_config at batch 3, 256 x 256: neither the batch nor the map sizes are in the shipped table, so Plan.tune()
    measures every layer, every Winograd alternative and the chain fusions, and writes them to YOLACT_AMD_TUNE_CACHE.  A second net
    and plan on the same weights in the same process finds everything in that file and computes the same bits."""
    import torch
    import yolact_amd
    from yolact_amd.utils.synth import synth_images, synth_state_dict
    from yolact_amd.yolact import Yolact
    cache = tmp_path / 'tune_cache.json'
    monkeypatch.setenv('YOLACT_AMD_TUNE_CACHE', str(cache))
    monkeypatch.setenv('YOLACT_AMD_AUTOTUNE', '1')
    yolact_amd.set_cfg('yolact_resnet50_config')
    dev = torch.device('cuda', 0)
    x = synth_images(3, 256, 256, seed=1234).to(dev)

    def run():
        net = Yolact()
        net.load_state_dict_compat(synth_state_dict([(k, tuple(v.shape)) for k, v in net.state_dict().items()], seed=0, conf_gain=0.04))
        net = net.to(dev)
        out = net.forward_raw(x)
        torch.cuda.synchronize()
        return net.plan_for(x), {k: out[k].cpu() for k in ('loc', 'conf_logits', 'mask', 'proto')}
    plan1, out1 = run()
    assert plan1.tune_misses > 0 and plan1.tune_table and plan1.wino_table
    assert cache.is_file()
    entries = TT.read_table_file(str(cache))
    new = {k: v for k, v in entries.items() if k not in SHIPPED}
    assert len(new) >= len(plan1.tune_table) > 0 and all(TT.parse(k)[1][0] == 3 for k in new)
    for k, v in entries.items():
        kind, t, mode = TT.parse(k)
        if kind in ('conv', 'dcn'):
            assert TT.direct_parts(v)[0] in L.TILE_NAMES, (k, v)
        elif kind == 'wino':
            assert len(v) == 6 and v[0] in (0,) + tuple(t[7]) and (TT.wino_parts(v[1])[0] in L.TILE_NAMES if v[0] else v[1] == 0), (k, v)
        elif kind == 'instep':
            assert v == 0, (k, v)
        else:
            assert kind in ('chain', 'chain1', 'chainx') and len(v) == 3 and v[0] in (0, 1), (k, v)
    plan2, out2 = run()
    assert plan2 is not plan1 and plan2.tune_misses == 0 and plan2.tune_table == []
    for k in out1:
        assert torch.isfinite(out1[k]).all() and torch.equal(out1[k], out2[k]), k
