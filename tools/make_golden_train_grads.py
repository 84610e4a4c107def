"""Generate tests/golden/train_grads.npz by EXECUTING THE REFERENCE's train-mode Yolact and MultiBoxLoss on the CPU (build container
only): one forward, the four losses, one backward of their sum, on the two cases of tests/train_step_ref.build_grads_case.

    python tools/make_golden_train_grads.py          # needs the reference checkout; writes tests/golden/train_grads.npz

The weights and inputs are built from seeds by this repository's own containers and loaded into the reference's Yolact through their
common state-dict names; 'frozen' calls the reference's own freeze_bn() after train().  The reference is imported with the stubs of
oracle/make_golden._shim_reference and runs once in fp64 (what is stored) and once in fp32 (for the record: its own fp32-versus-fp64
rel. L2 per parameter).  The fp64 run is net.double() on double inputs, plus two things that exist in this process only:
  * the prediction layers' priors, which the reference builds in fp32 whatever the network's dtype, are converted to double (the same
    fp32 VALUES: the matching and the box targets see the priors the fp32 network sees);
  * torch.Tensor.float is mapped to .double() for the duration of the run: the reference calls .float() on 0/1 indicator tensors, and
    binary_cross_entropy refuses the mixed dtypes otherwise.
Stored per case: the losses, and per parameter gradient and per running statistic after the step its numel, sum, L2 norm and 64 values
at the indices of tests/train_step_ref.digest_indices, all fp64.  Numbers only.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

LOSS_SEED = 100


def run_reference(ref_yolact, MultiBoxLoss, cfg, state, case, inputs, dtype):
    images, targets, masks, num_crowds = inputs
    net = ref_yolact.Yolact()
    net.load_state_dict(state)
    net.train()
    if case == 'frozen':
        net.freeze_bn()
    saved_float = torch.Tensor.float
    try:
        if dtype == torch.float64:
            net.double()
            torch.Tensor.float = lambda self, *a, **k: self.double()
            with torch.no_grad():
                net(images.double())                                 # builds the priors (fp32); the statistics are put back below
            net.load_state_dict(state)
            for pl in net.prediction_layers:
                assert pl.priors.dtype == torch.float32
                pl.priors = pl.priors.double()
        crit = MultiBoxLoss(cfg.num_classes, cfg.positive_iou_threshold, cfg.negative_iou_threshold, cfg.ohem_negpos_ratio)
        torch.manual_seed(LOSS_SEED)
        preds = net(images.to(dtype))
        assert preds['priors'].dtype == dtype and preds['loc'].dtype == dtype
        losses = crit(net, preds, [t.to(dtype) for t in targets], [m.to(dtype) for m in masks], num_crowds)
        assert sorted(losses) == ['B', 'C', 'M', 'S'] and all(v.dtype == dtype for v in losses.values())
        sum(losses.values()).backward()
    finally:
        torch.Tensor.float = saved_float
    grads = {n: (None if p.grad is None else p.grad.detach().double()) for n, p in net.named_parameters()}
    stats = {n: b.detach().double() for n, b in net.named_buffers() if 'running_' in n}
    return {k: float(v.detach()) for k, v in losses.items()}, grads, stats


def main():
    import heads_train_ref as H
    import train_net_ref as N
    import train_step_ref as T
    from oracle.make_golden import _shim_reference
    built = {}
    for case in T.GRADS_CASES:
        ours, images, targets, masks, num_crowds, batch_stats = T.build_grads_case('cpu', case)
        built[case] = ({k: v.clone() for k, v in ours.state_dict().items()}, (images, targets, masks, num_crowds), batch_stats)
    _shim_reference()
    from data import cfg, set_cfg
    set_cfg('yolact_resnet50_config')
    o = H.golden_cfg_overrides()
    o['max_size'] = T.GRADS_MAX_SIZE
    cfg.fpn = cfg.fpn.copy({'num_features': o.pop('num_features')})
    for k, v in o.items():
        setattr(cfg, k, v)
    import yolact as ref_yolact
    from layers.modules import MultiBoxLoss
    torch.set_num_threads(H.helpers.ORACLE_THREADS)
    arrays, meta = {}, dict(loss_seed=LOSS_SEED, grads_seed=T.GRADS_SEED, torch=torch.__version__, cases={})
    for case in T.GRADS_CASES:
        state, inputs, batch_stats = built[case]
        l64, g64, s64 = run_reference(ref_yolact, MultiBoxLoss, cfg, state, case, inputs, torch.float64)
        l32, g32, s32 = run_reference(ref_yolact, MultiBoxLoss, cfg, state, case, inputs, torch.float32)
        names, rows, vals, noise = [], [], [], []
        for kind, table, table32 in (('grad', g64, g32), ('stat', s64, s32)):
            for n, t in table.items():
                if t is None:
                    assert kind == 'grad' and case == 'frozen' and N.is_bn_affine(n) and table32[n] is None, n
                    continue
                flat = t.reshape(-1)
                names.append([kind, n])
                rows.append([flat.numel(), float(flat.sum()), float(flat.norm())])
                vals.append(flat[torch.from_numpy(T.digest_indices(len(names) - 1, flat.numel()))].numpy())
                noise.append(N.rel_l2(table32[n], t))
        arrays[case + '_losses'] = np.array([l64[k] for k in 'BMCS'], np.float64)
        arrays[case + '_losses32'] = np.array([l32[k] for k in 'BMCS'], np.float64)
        arrays[case + '_rows'] = np.array(rows, np.float64)
        arrays[case + '_vals'] = np.stack(vals).astype(np.float64)
        arrays[case + '_noise'] = np.array(noise, np.float32)
        meta['cases'][case] = dict(names=names, batch_stats=batch_stats)
        worst = max(zip(noise, names))
        print('%s: losses %s (fp32 run: %s); %d tensors; the reference\'s own fp32-versus-fp64 rel. L2 is at most %.3e (%s)'
              % (case, l64, l32, len(names), worst[0], worst[1][1]))
    dst = os.path.join(ROOT, 'tests', 'golden', 'train_grads.npz')
    np.savez_compressed(dst, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **arrays)
    print('wrote %s: %d bytes' % (dst, os.path.getsize(dst)))


if __name__ == '__main__':
    main()
