#!/usr/bin/env python
"""Record what the plan tuner would measure, on dry CPU plans: tests/golden/tune_candidates.json.

    python tools/make_golden_tune_candidates.py            # no GPU needed; default environment, a build whose ISA lint ran

For the five configurations of tests/test_plan_schedule.py at batch 1 and 8 (Plan(..., torch.device('cpu'), dry_two_streams=True)):
`Plan.direct_candidates(fn, d, wide)` of every convolution / DCN launch, stored once per distinct table key (a key whose launches do
not all get the same list keeps every distinct list, in order of appearance), and `Plan.stage_exit_candidates()` per plan.  Candidate
order decides ties between equal timings, so tests/test_tune_table.py compares the lists exactly, order included.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [('yolact_resnet50_config', 550), ('yolact_base_config', 550), ('yolact_darknet53_config', 550), ('yolact_im700_config', 700),
         ('yolact_plus_resnet50_config', 550)]
BATCHES = (1, 8)
OUT = os.path.join(ROOT, 'tests', 'golden', 'tune_candidates.json')


def dry_plan(config, size, B):
    import torch
    import yolact_amd
    from yolact_amd.engine import Plan
    from yolact_amd.yolact import Yolact
    yolact_amd.set_cfg(config)
    torch.manual_seed(0)
    return Plan(Yolact(), B, size, size, torch.device('cpu'), dry_two_streams=True)


def direct_launches(plan):
    """(fn, descriptor, wide) of every launch Plan._tune_direct visits, in op order."""
    for opi, (fn, dptr, _name, _where) in enumerate(plan.ops):
        is_dcn = fn is plan.lib.ymi_dcn_v2_forward_f32
        if fn is plan.lib.ymi_conv2d_nhwc_f32 or is_dcn:
            yield fn, (dptr.contents.conv if is_dcn else dptr.contents), opi in plan.wide_ops


def collect(plans):
    """plans: iterable of ('<config>/B<batch>', plan) -> the document of tests/golden/tune_candidates.json."""
    cands, exits = {}, {}
    for tag, plan in plans:
        for fn, d, wide in direct_launches(plan):
            lists = cands.setdefault(plan.direct_key(fn, d, wide), [])
            c = [int(v) for v in plan.direct_candidates(fn, d, wide)]
            if c not in lists:
                lists.append(c)
        exits[tag] = [[i3, i1, list(downs)] for i3, i1, downs in plan.stage_exit_candidates()]
    return {'direct_candidates': cands, 'stage_exit_candidates': exits}


def all_plans():
    for config, size in CASES:
        for B in BATCHES:
            yield '%s/B%d' % (config, B), dry_plan(config, size, B)


def main():
    from yolact_amd.tune_table import build_meta
    assert build_meta().get('lint') == 'ok', 'run __graft_entry__.build() first: the patch tile is a candidate only after the ISA lint'
    doc = collect(all_plans())
    with open(OUT, 'w') as f:
        json.dump(doc, f, indent=0, separators=(',', ':'), sort_keys=True)
        f.write('\n')
    print('%d keys, %d plans, %d bytes -> %s' % (len(doc['direct_candidates']), len(doc['stage_exit_candidates']), os.path.getsize(OUT), OUT))


if __name__ == '__main__':
    main()
