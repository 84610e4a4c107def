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
