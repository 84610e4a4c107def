"""The whole training step's forward and backward in plain torch: images -> stem -> stages -> FPN -> heads -> MultiBoxLoss -> the
gradient of B + M + C + S in every parameter.  Nothing is restated here: stem_ref, chain_ref, fpn_ref, heads_ref and multibox_ref
(each pinned to the reference by its own host test) are composed as Yolact.forward composes the modules, and multibox_ref's gradients
in the predictions are fed back through the composed graph.  The oracle of tests/test_train_net_host.py (pinned there to what the
reference's own train-mode Yolact and MultiBoxLoss computed: tests/golden/train_grads.npz, tools/make_golden_train_grads.py) and of
tests/test_gpu_train_grads.py.

Everything works in the dtype given (fp32 or fp64) on the CPU, NCHW; the matching is decided in fp32 (multibox_ref).  The parameters
are a dict under the model's own state-dict names (backbone.conv1.weight, backbone.layers.1.0.bn2.running_var, fpn.lat_layers.0.weight,
proto_net.0.bias, prediction_layers.0.conf_layer.weight, semantic_seg_conv.bias, ..).

`wrong` switches on ONE deliberately wrong wiring; every one computes the right losses and differs in the gradients (or, for 's_norm',
in S and what comes from it) only:
    'lateral'   what the FPN's lateral sends into the output of stage WRONG_LATERAL_STAGE is dropped (that map's second consumer)
    'head4'     the shared prediction head's parameters take their gradient from four levels, not five
    'p67'       P6 and P7 are detached from P5
    's_norm'    S divided by the number of positives (multibox_ref's s_norm='num_pos')
    'bn_xhat'   BatchNorm backward without its mean(dy * xhat) * xhat term (batch statistics only)
    'proto_m'   the protonet receives nothing from M
"""
import torch

import backbone_train_ref as R
import fpn_train_ref as FR
import heads_train_ref as H
import helpers
import multibox_ref as MB
import stem_train_ref as SR

WRONG = ('lateral', 'head4', 'p67', 's_norm', 'bn_xhat', 'proto_m')
WRONG_LATERAL_STAGE = 2                     # layers.2: its output feeds layers.3 and the middle lateral
SECTIONS = ('stem', 'layers.0', 'layers.1', 'layers.2', 'layers.3')


def is_stat(name):
    return 'running_' in name


def is_bn_affine(name):
    """A BatchNorm's weight or bias, by its state-dict name (bn1 .. bn3 and a projection's downsample.1)."""
    return name.endswith(('.weight', '.bias')) and ('.bn' in name or '.downsample.1.' in name)


def section_of(name):
    """'stem', 'layers.0' .. 'layers.3' for the backbone's tensors; None for everything above it."""
    if not name.startswith('backbone.'):
        return None
    return name[len('backbone.'):len('backbone.layers.0')] if name.startswith('backbone.layers.') else 'stem'


def leaf_names(state, train_bn_affine=True):
    """The parameters that take a gradient, in state-dict order."""
    return [n for n in state if 'num_batches' not in n and not is_stat(n) and (train_bn_affine or not is_bn_affine(n))]


def stage_blocks(state):
    """[[(prefix, stride), ..] per stage] from the names: the stride sits on the first block of every stage but the first."""
    stages = []
    for s in range(4):
        n = len({k.split('.')[3] for k in state if k.startswith('backbone.layers.%d.' % s)})
        stages.append([('layers.%d.%d.' % (s, b), 2 if (b == 0 and s > 0) else 1) for b in range(n)])
    return stages


def backbone_ref(images, PB, stages, batch_stats, keep=None, new_stats=None, **bn_kw):
    """The stem and the stages on the backbone's own names (no 'backbone.' prefix) -> one output per stage.  keep: dict with 'stem'
    (stem_ref's dict) and 'backbone' (chain_ref's list)."""
    kstem, kchain = (None, None) if keep is None else (keep.setdefault('stem', {}), keep.setdefault('backbone', []))
    x = SR.stem_ref(images, PB, batch_stats, kstem, new_stats, **bn_kw)
    outs = []
    for blocks in stages:
        x = R.chain_ref(x, PB, blocks, batch_stats, kchain, new_stats, **bn_kw)[-1]
        outs.append(x)
    return outs


def train_ref(state, images, targets, masks, num_crowds, spec, batch_stats, dtype=torch.float64, train_bn_affine=True, wrong=None,
              keep=None, selected=(1, 2, 3), n_down=2, negpos_ratio=3):
    """state: name -> CPU tensor (fp32 values); spec: heads_train_ref.spec_of(cfg) -> dict(
        losses {'B','M','C','S'}, grads {name: d (B + M + C + S) / d parameter} for leaf_names(state, train_bn_affine),
        new_stats {name: running statistic after the step}, preds (detached), extras (multibox_ref's: conf_t, neg, key, n, ..)).
    keep (a dict) receives the ReLU records of the component oracles under 'stem', 'backbone', 'fpn', 'heads', and under 'act_grads' the
    gradient each recorded FPN / heads activation received (None where none arrived)."""
    assert wrong is None or wrong in WRONG, wrong
    assert wrong != 'bn_xhat' or batch_stats
    P = {n: t.detach().to(dtype) for n, t in state.items() if 'num_batches' not in n}
    names = leaf_names(P, train_bn_affine)
    for n in names:
        P[n].requires_grad_(True)
    PB = {n[len('backbone.'):]: t for n, t in P.items() if n.startswith('backbone.')}
    new_stats = {}
    with helpers.oracle_threads():                       # torch's CPU summation order depends on the thread count
        bn_kw = {'xhat_term': False} if wrong == 'bn_xhat' else {}
        stage_outs = backbone_ref(images.detach().to(dtype), PB, stage_blocks(P), batch_stats, keep, new_stats, **bn_kw)
        feats = [stage_outs[i].detach() if (wrong == 'lateral' and i == WRONG_LATERAL_STAGE) else stage_outs[i] for i in selected]
        kfpn, kheads = (None, None) if keep is None else (keep.setdefault('fpn', []), keep.setdefault('heads', []))
        maps = FR.fpn_ref(feats, P, n_down, kfpn, detach_down=wrong == 'p67')
        pred = H.heads_ref(maps, P, spec, kheads, head_grad_levels=4 if wrong == 'head4' else None)
        acts = [] if keep is None else [a for _, _, a in kfpn + kheads]
        for a in acts:
            a.retain_grad()
        detached = {k: pred[k].detach() for k in MB.NAMES}
        detached['priors'] = pred['priors']
        losses, g, extras = MB.multibox_ref(detached, targets, masks, num_crowds, dtype, negpos_ratio=negpos_ratio,
                                            s_norm='num_pos' if wrong == 's_norm' else 'batch')
        if wrong == 'proto_m':
            g = dict(g, proto=torch.zeros_like(g['proto']))              # only M reads the prototypes
        torch.autograd.backward([pred[k] for k in MB.NAMES], [g[k] for k in MB.NAMES])
    if keep is not None:
        keep['act_grads'] = [a.grad for a in acts]
    grads = {n: (torch.zeros_like(P[n]) if P[n].grad is None else P[n].grad) for n in names}
    return dict(losses=losses, grads=grads, new_stats={'backbone.' + n: t.detach() for n, t in new_stats.items()},
                preds=detached, extras=extras)


def head_margins(keep64, keep32):
    """Per ReLU above the backbone (FPN pred layers, protonet, the prediction head once per level): (name, the smallest
    |pre-activation| whose activation receives gradient, in fp64; the largest fp32-versus-fp64 deviation of that tensor): what
    heads_train_ref.assert_margins takes."""
    out = []
    rec64, rec32 = keep64['fpn'] + keep64['heads'], keep32['fpn'] + keep32['heads']
    assert [n for n, _, _ in rec64] == [n for n, _, _ in rec32]
    for i, ((n, z64, _), (_, z32, _), g) in enumerate(zip(rec64, rec32, keep64['act_grads'])):
        hit = torch.zeros_like(z64, dtype=torch.bool) if g is None else g != 0
        out.append(('%s#%d' % (n, i), z64.detach()[hit].abs().min().item() if hit.any() else float('inf'),
                    (z32.detach().double() - z64.detach()).abs().max().item()))
    return out


def calibrated_stats(state, images, momentum=1.0):
    """Every running statistic replaced by the batch's own (the mean and the unbiased variance of one batch-statistics forward in
    fp64 with momentum 1), rounded to fp32 -> name -> tensor."""
    P = {n: t.detach().double() for n, t in state.items() if 'num_batches' not in n}
    PB = {n[len('backbone.'):]: t for n, t in P.items() if n.startswith('backbone.')}
    new_stats = {}
    with torch.no_grad(), helpers.oracle_threads():
        backbone_ref(images.detach().double(), PB, stage_blocks(P), True, None, new_stats, momentum=momentum)
    return {'backbone.' + n: t.float() for n, t in new_stats.items()}


RELU_LAYERS = ('fpn.pred_layers.0', 'fpn.pred_layers.1', 'fpn.pred_layers.2', 'proto_net.0', 'proto_net.2', 'proto_net.4', 'proto_net.8',
               'proto_net.10', 'prediction_layers.0.upfeature.0')          # in an order in which each depends on the earlier ones only


def spread_biases(state, images, spec, k, seed, selected=(1, 2, 3), n_down=2):
    """The biases of every convolution above the backbone that feeds a ReLU, chosen so that its pre-activations stay away from 0:
    per channel c, bias_c = s_c * k * std_c - mean_c with s_c = +-1 from `seed` (both signs in every layer) and mean_c, std_c the
    statistics of the bias-free pre-activation over the batch (over all five levels for the shared head, whose largest level sets
    std_c).  A channel is then mostly on or mostly off, k deviations from the decision.  Layer by layer in fp64, batch statistics in
    the backbone -> name -> fp32 bias.  Why: tests/train_step_ref.py, at GRADS_BIAS_K."""
    P = {n: t.detach().double() for n, t in state.items() if 'num_batches' not in n}
    PB = {n[len('backbone.'):]: t for n, t in P.items() if n.startswith('backbone.')}
    gen = torch.Generator().manual_seed(seed)
    out = {}
    with torch.no_grad(), helpers.oracle_threads():
        stage_outs = backbone_ref(images.detach().double(), PB, stage_blocks(P), True)
        for layer in RELU_LAYERS:
            P[layer + '.bias'] = torch.zeros_like(P[layer + '.bias'])
            keep = []
            maps = FR.fpn_ref([stage_outs[i] for i in selected], P, n_down, keep)
            H.heads_ref(maps, P, spec, keep)
            zs = [z.transpose(0, 1).reshape(z.shape[1], -1) for n, z, _ in keep if n == layer]
            mean = torch.cat(zs, 1).mean(1)
            std = torch.stack([(z - mean[:, None]).pow(2).mean(1).sqrt() for z in zs]).max(0).values
            sign = torch.ones_like(mean)
            sign[torch.randperm(mean.numel(), generator=gen)[:mean.numel() // 2]] = -1
            P[layer + '.bias'] = out[layer + '.bias'] = (sign * k * std - mean).float().double()
    return {n: t.float() for n, t in out.items()}


def rel_l2(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    den = b.norm().item()
    return (a - b).norm().item() / (den if den > 0 else 1.0)


def section_noise(g32, g64):
    """Per backbone section the largest rel. L2 between the fp32 and the fp64 oracle over the section's gradients."""
    out = {s: 0.0 for s in SECTIONS}
    for n in g64:
        s = section_of(n)
        if s is not None:
            out[s] = max(out[s], rel_l2(g32[n], g64[n]))
    return out
