"""The training step: the reference's train.py inner loop (train.py:215-216, 290-320, 388-391) around the pieces that run on the GPU.

    lr_at(iteration, cfg)           train.py:295-301 as a pure function: the learning rate iteration `iteration` runs with
    autoscale(cfg, batch_size)      train.py:90-98: lr, max_iter and lr_steps scaled by batch_size / 8
    Trainer(net)                    forward_train -> MultiBoxLoss -> backward -> optim.SGD.step(loss), one iteration per step()

Yolact.train(True) raises, so the loop is an object of its own that drives the net in eval mode through
forward_train(images, batch_stats).  A step never reads from the device: the isfinite(loss) test of train.py:317 is the guard of
the update kernel (optim.SGD.step(loss)), and the losses come back as device tensors.
"""
from __future__ import annotations

import contextlib

import torch

from .config import active_cfg
from .layers import train_ops
from .optim import SGD


def lr_at(iteration, cfg, lr=None, gamma=None):
    """The learning rate of iteration `iteration` (train.py:295-301).  Through iteration cfg.lr_warmup_until: the linear warm-up from
    cfg.lr_warmup_init to lr; after it: lr * gamma ** (how many of cfg.lr_steps are <= iteration).  lr / gamma default to cfg's
    (train.py's args.lr / args.gamma)."""
    lr = cfg.lr if lr is None else lr
    gamma = cfg.gamma if gamma is None else gamma
    if cfg.lr_warmup_until > 0 and iteration <= cfg.lr_warmup_until:
        return (lr - cfg.lr_warmup_init) * (iteration / cfg.lr_warmup_until) + cfg.lr_warmup_init
    return lr * (gamma ** sum(1 for s in cfg.lr_steps if iteration >= s))


def autoscale(cfg, batch_size):
    """train.py:90-98: at a batch size other than 8, lr times batch_size / 8 and max_iter and every lr_step floor-divided by it,
    written into `cfg`, which is returned."""
    if batch_size != 8:
        factor = batch_size / 8
        cfg.lr *= factor
        cfg.max_iter //= factor
        cfg.lr_steps = [x // factor for x in cfg.lr_steps]
    return cfg


def set_lr(optimizer, new_lr):
    """train.py:388-391."""
    for group in optimizer.param_groups:
        group['lr'] = new_lr


class Trainer:
    """One training iteration per step().  Defaults: MultiBoxLoss, or MultiBoxLossPlus under cfg.use_maskiou, with the config's
    thresholds (train.py:217-220); optim.SGD over net.parameters() with cfg.lr, cfg.momentum and cfg.decay (train.py:215-216);
    batch_stats = not cfg.freeze_bn, and under cfg.freeze_bn the BatchNorm affine parameters stop requiring grad (yolact.py:552-553).
    The config is read when the Trainer is made and at every step.  forward: a callable (images, batch_stats) -> pred_outs, default
    net.forward_train; Trainer(net, forward=lambda x, bs: train_net.forward(net, x, bs)) trains a YOLACT++ config, whose DCN blocks
    Yolact.forward_train still refuses, and yolact_darknet53, whose DarkNetBackbone it refuses too (train_net.darknet runs it).
    wgrad: None leaves train_ops' weight-gradient mode as the caller set it; 'fp32' or 'fp16x2' runs the forward of every step under
    train_ops.wgrad_mode(wgrad), so the step's convolutions take their weight gradient from that kernel.  conv: the same for
    train_ops.conv_mode, the tiles of the convolutions' forward and data gradient; the two switches are independent."""

    def __init__(self, net, criterion=None, optimizer=None, batch_stats=None, wgrad=None, conv=None, forward=None):
        cfg = active_cfg()
        self.wgrad = None if wgrad is None else train_ops.check_wgrad_mode(wgrad)
        self.conv = None if conv is None else train_ops.check_conv_mode(conv)
        self.net = net
        if cfg.freeze_bn:
            net.freeze_bn()
        if criterion is None:
            if cfg.use_maskiou:
                from .layers.modules.multibox_loss_plus import MultiBoxLossPlus as Loss
            else:
                from .layers.modules.multibox_loss import MultiBoxLoss as Loss
            criterion = Loss(cfg.num_classes, cfg.positive_iou_threshold, cfg.negative_iou_threshold, cfg.ohem_negpos_ratio)
        self.criterion = criterion
        self.forward = forward                               # None: net.forward_train, looked up at every step
        if optimizer is None:
            optimizer = SGD(net.parameters(), lr=cfg.lr, momentum=cfg.momentum, weight_decay=cfg.decay)
            optimizer.name_parameters(net.named_parameters())
        self.optimizer = optimizer
        self.batch_stats = (not cfg.freeze_bn) if batch_stats is None else bool(batch_stats)
        self.lr = optimizer.param_groups[0]['lr']            # train.py's args.lr: what the schedule scales
        self.gamma = cfg.gamma
        self.iteration = 0

    def step(self, images, targets, masks, num_crowds):
        """images [B,3,H,W] on the GPU, the rest as detection_collate yields them -> the dict of loss tensors, on the device, not
        synchronised.  In train.py's order: the learning rate of this iteration, forward, criterion, the sum, backward, the guarded
        update (which zeroes the gradients for the next iteration), iteration += 1."""
        set_lr(self.optimizer, lr_at(self.iteration, active_cfg(), self.lr, self.gamma))
        with contextlib.nullcontext() if self.wgrad is None else train_ops.wgrad_mode(self.wgrad), \
                contextlib.nullcontext() if self.conv is None else train_ops.conv_mode(self.conv):
            preds = (self.net.forward_train if self.forward is None else self.forward)(images, self.batch_stats)
        losses = self.criterion(self.net, preds, targets, masks, num_crowds)
        loss = sum(losses.values())
        loss.backward()
        self.optimizer.step(loss)
        self.iteration += 1
        return losses

    def fit(self, batches, iterations=None):
        """The plain loop over an iterable of detection_collate output, (images, (targets, masks, num_crowds)), for `iterations` steps
        (default: until cfg.max_iter or the iterable ends) -> the losses of the last step."""
        dev = next(self.net.parameters()).device
        last = None
        done = 0
        for images, (targets, masks, num_crowds) in batches:
            if (iterations is not None and done >= iterations) or self.iteration >= active_cfg().max_iter:
                break
            if not torch.is_tensor(images):
                images = torch.stack([torch.as_tensor(i) for i in images])
            move = lambda seq: [torch.as_tensor(t).to(dev) for t in seq]
            last = self.step(images.to(dev), move(targets), move(masks), list(num_crowds))
            done += 1
        return last
