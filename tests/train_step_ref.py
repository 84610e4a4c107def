"""What tests/test_sgd_host.py, tests/test_gpu_sgd.py, tests/test_gpu_train_step.py and the tools that write their fixtures share: the
numpy restatement of the SGD contract, the model and inputs of the end-to-end train tests, and the backbone file of the init_weights
test.  Nothing here needs a GPU."""
import hashlib

import numpy as np
import torch

import backbone_train_ref as R
import heads_train_ref as H

F32 = np.float32


def sgd_step_np(p, g, m, lr, mom, wd):
    """One step of the contract of ymi_sgd_step_f32 (include/yolact_amd.h) on fp32 arrays: every operation rounded once to fp32.
    -> (p', m'); m' is m itself when mom == 0."""
    lr, mom, wd = F32(lr), F32(mom), F32(wd)
    p, g = p.astype(F32), g.astype(F32)
    d = g if wd == 0 else (g + (wd * p).astype(F32)).astype(F32)
    if mom == 0:
        return (p - (lr * d).astype(F32)).astype(F32), m
    m = ((mom * m.astype(F32)).astype(F32) + d).astype(F32)
    return (p - (lr * m).astype(F32)).astype(F32), m


# ---- the model and inputs of tests/test_gpu_stem_train.py test_multibox_loss_from_the_images ----------------------------------------------
CASE_SEED = 3


def build_case(device):
    """The 32-feature yolact_resnet50_config on seeded ResNet-50 stages (tests/test_gpu_backbone_train.py seeded_backbone, seed 3), two
    96 x 96 images, their targets and masks: built on the CPU from seeds, then moved to `device`.  -> (net, images, targets, masks,
    num_crowds).  Leaves yolact_amd.config.cfg at that config."""
    import yolact_amd
    from yolact_amd.yolact import Yolact
    yolact_amd.set_cfg('yolact_resnet50_config')
    torch.manual_seed(CASE_SEED)
    net = Yolact()
    gen = torch.Generator().manual_seed(CASE_SEED)
    with torch.no_grad():
        for si, layer in enumerate(net.backbone.layers):
            for bi, blk in enumerate(layer):
                prefix = 'layers.%d.%d.' % (si, bi)
                vals = R.random_block_params(gen, blk.conv1.in_channels, blk.conv1.out_channels, blk.downsample is not None, prefix)
                sd = blk.state_dict()
                for n in sd:
                    if 'num_batches' not in n:
                        sd[n].copy_(vals[prefix + n])
    cfg = yolact_amd.config.cfg
    o = H.golden_cfg_overrides()
    cfg.fpn = cfg.fpn.copy({'num_features': o.pop('num_features')})
    cfg.update(o)
    torch.manual_seed(CASE_SEED)
    head = Yolact()
    head.backbone = net.backbone
    head.invalidate_plans()
    head.to(device)
    gen = torch.Generator().manual_seed(4)
    images = torch.randn(2, 3, 96, 96, generator=gen)
    targets = [torch.tensor([[0.11, 0.13, 0.42, 0.41, 2.0], [0.52, 0.31, 0.93, 0.79, 0.0], [0.21, 0.56, 0.44, 0.81, 4.0],
                             [0.03, 0.03, 0.97, 0.96, 1.0]]),
               torch.tensor([[0.31, 0.22, 0.79, 0.71, 1.0], [0.06, 0.61, 0.29, 0.84, 3.0]])]
    masks = []
    for t in targets:
        m = torch.zeros(t.size(0), 48, 48)
        for j, (x1, y1, x2, y2) in enumerate((t[:, :4] * 48).round().long().tolist()):
            m[j, y1:y2, x1:x2] = 1
        masks.append(m)
    return head, images.to(device), [t.to(device) for t in targets], [m.to(device) for m in masks], [0, 0]


# ---- the two cases of tests/test_train_net_host.py and tests/test_gpu_train_grads.py -------------------------------------------------
# The model of build_case with other seeds, and targets that put a positive prior on every pyramid level.  With build_case's
# max_size = 96 the P6 and P7 priors (192 and 384 pixels) are two and four images wide and no box inside an image can match them, so
# here the priors are made for max_size = 384 (a cfg value that only the priors read): 1/16, 1/8, 1/4, 1/2 and 1 image wide on P3 ..
# P7, and the targets hold a box of about each size.  The seeds were chosen by tools/find_train_grads_case.py, which tries seeds in
# order until the conditions tests/test_train_net_host.py asserts hold for both cases (with twice the ReLU margin asserted there).
#
# The ReLUs above the backbone.  After 50 layers the fp32 and the fp64 oracle differ by about 1e-4 of a pre-activation's spread there,
# and about 130 000 activations receive gradient: with the modules' default biases some 120 of them lie within 16 deviations of 0
# whatever the seed, and no search finds a case that keeps the project's margin.  So the biases in front of those ReLUs are set
# (train_net_ref.spread_biases) to GRADS_BIAS_K spreads of the channel's own pre-activation, half of the channels above 0 and half
# below: a channel is mostly on or mostly off, and the few elements that cross do so far from 0.  The ReLU masks themselves are pinned
# element by element in tests/test_gpu_fpn_train.py and tests/test_gpu_heads_train.py; what these cases pin is the wiring.
GRADS_SEED = 23
GRADS_BIAS_K = 4.0
GRADS_MAX_SIZE = 384
GRADS_CASES = ('stats', 'frozen')
GRADS_BOX_SIZES = ((1.0, 0.5, 0.25, 0.125, 0.0625), (0.5, 1.0, 0.125, 0.25, 0.0625, 0.3))


def grads_targets(seed):
    """Two images' targets [n,5] and 48 x 48 box masks: per image one box of about each size of GRADS_BOX_SIZES (each side within
    +- 10 %, clipped to [0.01, 0.99]) at a seeded place, labels in 0 .. 4."""
    gen = torch.Generator().manual_seed(seed)
    targets, masks = [], []
    for sizes in GRADS_BOX_SIZES:
        rows = []
        for s in sizes:
            w, h = [min(0.98, s * (0.9 + 0.2 * float(torch.rand((), generator=gen)))) for _ in range(2)]
            x1 = 0.01 + (0.98 - w) * float(torch.rand((), generator=gen))
            y1 = 0.01 + (0.98 - h) * float(torch.rand((), generator=gen))
            rows.append([x1, y1, x1 + w, y1 + h, float(torch.randint(0, 5, (), generator=gen))])
        t = torch.tensor(rows)
        m = torch.zeros(t.size(0), 48, 48)
        for j, (x1, y1, x2, y2) in enumerate((t[:, :4] * 48).round().long().tolist()):
            m[j, y1:max(y2, y1 + 1), x1:max(x2, x1 + 1)] = 1
        targets.append(t)
        masks.append(m)
    return targets, masks


def build_grads_case(device, name, seed=GRADS_SEED):
    """name 'stats': batch statistics, every parameter trains.  'frozen': the same weights with every running statistic replaced by
    the batch's own (train_net_ref.calibrated_stats), the BatchNorm affine parameters frozen (Yolact.freeze_bn), batch_stats False.
    Built on the CPU from seeds, then moved to `device` -> (net, images, targets, masks, num_crowds, batch_stats).  Leaves
    yolact_amd.config.cfg at the case's config."""
    import train_net_ref as N
    import yolact_amd
    from yolact_amd.yolact import Yolact
    assert name in GRADS_CASES
    yolact_amd.set_cfg('yolact_resnet50_config')
    torch.manual_seed(seed)
    net = Yolact()
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for si, layer in enumerate(net.backbone.layers):
            for bi, blk in enumerate(layer):
                prefix = 'layers.%d.%d.' % (si, bi)
                vals = R.random_block_params(gen, blk.conv1.in_channels, blk.conv1.out_channels, blk.downsample is not None, prefix)
                sd = blk.state_dict()
                for n in sd:
                    if 'num_batches' not in n:
                        sd[n].copy_(vals[prefix + n])
    cfg = yolact_amd.config.cfg
    o = H.golden_cfg_overrides()
    o['max_size'] = GRADS_MAX_SIZE
    cfg.fpn = cfg.fpn.copy({'num_features': o.pop('num_features')})
    cfg.update(o)
    torch.manual_seed(seed)
    head = Yolact()
    head.backbone = net.backbone
    head.invalidate_plans()
    images = torch.randn(2, 3, 96, 96, generator=torch.Generator().manual_seed(seed + 1))
    targets, masks = grads_targets(seed + 2)
    state = head.state_dict()
    state.update(N.spread_biases(state, images, H.spec_of(cfg), GRADS_BIAS_K, seed + 3))
    if name == 'frozen':
        state.update(N.calibrated_stats(state, images))
        head.freeze_bn()
    head.load_state_dict(state)
    head.to(device)
    return head, images.to(device), [t.to(device) for t in targets], [m.to(device) for m in masks], [0, 0], name == 'stats'


def grads_oracles(name, seed=GRADS_SEED, keep=False, dtypes=(torch.float64, torch.float32)):
    """The composed oracle (train_net_ref.train_ref) on a case in each of `dtypes` -> ({dtype: result}, {dtype: keep dict}, inputs):
    inputs = dict(state, images, targets, masks, num_crowds, spec, batch_stats, train_bn_affine), all on the CPU."""
    import train_net_ref as N
    import yolact_amd
    net, images, targets, masks, num_crowds, batch_stats = build_grads_case('cpu', name, seed)
    inputs = dict(state={k: v.detach().clone() for k, v in net.state_dict().items()}, images=images, targets=targets, masks=masks,
                  num_crowds=num_crowds, spec=H.spec_of(yolact_amd.config.cfg), batch_stats=batch_stats, train_bn_affine=batch_stats)
    res, keeps = {}, {}
    for dt in dtypes:
        keeps[dt] = {} if keep else None
        res[dt] = N.train_ref(dtype=dt, keep=keeps[dt], **inputs)
    return res, keeps, inputs


def level_of_prior(sizes=(12, 6, 3, 2, 1), per_cell=3):
    """The pyramid level (0 = P3) of every prior, in prior order."""
    return torch.cat([torch.full((s * s * per_cell,), lvl, dtype=torch.long) for lvl, s in enumerate(sizes)])


def grads_case_report(name, seed=GRADS_SEED, factor=16):
    """What the search asks of a case and tests/test_train_net_host.py asserts of the chosen one -> dict(failed [names of the
    conditions that do not hold], line (one line of figures), res, keeps, inputs as grads_oracles returns them, and the figures)."""
    import class_loss_ref as CR
    import match_ref as TR
    import train_net_ref as N
    res, keeps, inputs = grads_oracles(name, seed, keep=True)
    r64, r32 = res[torch.float64], res[torch.float32]
    priors = r64['preds']['priors']
    m32 = TR.match_batch_ref(priors, inputs['targets'], inputs['num_crowds'])
    m64 = TR.match_batch_ref(priors.double(), inputs['targets'], inputs['num_crowds'])
    same_match = all(torch.equal(m32[k], m64[k]) for k in ('conf_t', 'idx_t', 'pos'))
    lvl = level_of_prior()
    assert lvl.numel() == priors.size(0)
    pos_per_level = [int(m32['pos'][:, lvl == l].sum()) for l in range(5)]
    zero = [n for n, g in r64['grads'].items() if not bool(g.ne(0).any())]
    margins = N.head_margins(keeps[torch.float64], keeps[torch.float32])
    tight = H.tightest(margins)
    gap = min(CR.cut_gaps(r64['extras']['key'], r64['extras']['n']))
    same_neg = torch.equal(r64['extras']['neg'], r32['extras']['neg'])
    failed = [what for what, ok in (('levels', min(pos_per_level) >= 1), ('zero gradients', not zero),
                                    ('margins', all(lo >= factor * dev for _, lo, dev in margins)), ('cut', gap >= 1e-3),
                                    ('matching', same_match), ('mined set', same_neg),
                                    ('masks_to_train', int(m32['num_pos'].max()) <= 100)) if not ok]
    line = 'positives per level %s, zero gradients %d, tightest margin %s %.3e / %.3e = %.1f, cut gap %.3e, failed %s' % (
        pos_per_level, len(zero), tight[0], tight[1], tight[2], tight[1] / max(tight[2], 1e-300), gap, failed)
    return dict(failed=failed, line=line, res=res, keeps=keeps, inputs=inputs, pos_per_level=pos_per_level, zero=zero,
                margins=margins, gap=gap, same_match=same_match, same_neg=same_neg)


DIGEST_VALUES = 64


def digest_indices(row, numel):
    """The DIGEST_VALUES flat indices at which tests/golden/train_grads.npz keeps tensor number `row`: plain integer arithmetic, the
    same on every host (short tensors repeat)."""
    k = np.arange(DIGEST_VALUES, dtype=np.int64)
    return (k * 2654435761 + row * 40503 + 12345) % numel


# ---- the init_weights case --------------------------------------------------------------------------------------------------------------
INIT_SEED = 0
INIT_FILE_SEED = 11
INIT_FILE_PREFIXES = ('conv1.', 'bn1.', 'layers.0.', 'layers.1.3.')      # what the small backbone file holds, under its legacy names


def backbone_file_state(backbone):
    """A small pretrained-backbone state dict for `backbone` (a ResNetBackbone of ours or of the reference: same keys), as
    torchvision names it: `layer1..4` for `layers.0..3`, plus the `fc` tensors no backbone has.  Only the stem, the first stage and
    one block of the second are in it (the load is non-strict); values from INIT_FILE_SEED."""
    gen = torch.Generator().manual_seed(INIT_FILE_SEED)
    out = {}
    for k, v in backbone.state_dict().items():
        if not k.startswith(INIT_FILE_PREFIXES) or 'num_batches' in k:
            continue
        t = torch.randn(v.shape, generator=gen) * 0.05
        if k.endswith('running_var'):
            t = t.abs() + 0.5
        if k.startswith('layers.'):
            k = 'layer%d' % (int(k[7]) + 1) + k[8:]
        out[k] = t
    out['fc.weight'] = torch.randn(10, 2048, generator=gen)
    out['fc.bias'] = torch.randn(10, generator=gen)
    return out


def init_digest_keys(net):
    """The state-dict keys the init_weights golden covers: everything outside the backbone, and the backbone tensors the file holds."""
    return [k for k in net.state_dict()
            if 'num_batches' not in k and (not k.startswith('backbone.') or k[len('backbone.'):].startswith(INIT_FILE_PREFIXES))]


def sha256(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
