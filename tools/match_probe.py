#!/usr/bin/env python3
"""Time match_targets (csrc/match.hip: targets + box loss + d_loc for the batch in one call) against tests/match_ref.py run with
torch ops on the same GPU (the reference's algorithm: an [n_gt, P] overlap matrix per image and a loop of n_gt iterations, each
reading two indices back to the host), at batch 8 on the 550 x 550 prior set with 12 GTs and 1 crowd per image.

HIP events around each call, WARMUP warm-ups, the median of REPS, as tools/dcn_bwd_probe.py does.  `kernels_us` is the bare
ymi_match_f32 call on prepared buffers (four launches), `match_targets_us` includes the Python plumbing (concatenating the targets,
two small host-to-device copies of the offsets, allocating the outputs and the workspace).  Recorded, not gated.

    python tools/match_probe.py [--batch 8] [--gts 12] [--crowds 1] [--reps 20] [--warmup 5]
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import match_ref as R  # noqa: E402
import yolact_amd  # noqa: E402
from yolact_amd import _lib as L  # noqa: E402
from yolact_amd.layers import match as M  # noqa: E402
from dcn_bwd_probe import timed  # noqa: E402


def make_targets(g, n, n_crowd):
    size = torch.tensor([24.0, 48.0, 96.0, 192.0, 384.0])[torch.randint(0, 5, (n + n_crowd,), generator=g)] / 550
    size = size * (0.7 + 0.7 * torch.rand(n + n_crowd, generator=g))
    c = 0.05 + 0.9 * torch.rand(n + n_crowd, 2, generator=g)
    box = torch.cat([c - size[:, None] / 2, c + size[:, None] / 2], 1).clamp(0.0, 1.0)
    cls = torch.randint(0, 80, (n + n_crowd, 1), generator=g).float()
    cls[n:] = -1
    return torch.cat([box, cls], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--gts', type=int, default=12)
    ap.add_argument('--crowds', type=int, default=1)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    a = ap.parse_args()
    dev = 'cuda:0'
    g = torch.Generator().manual_seed(0)
    cfg = yolact_amd.CONFIGS['yolact_base_config'].copy()
    M.active_cfg = lambda: cfg
    priors = R.make_priors((69, 35, 18, 9, 5), 550).to(dev)
    B, P = a.batch, priors.size(0)
    targets = [make_targets(g, a.gts, a.crowds).to(dev) for _ in range(B)]
    ncs = [a.crowds] * B
    loc_data = (torch.randn(B, P, 4, generator=g) * 0.7).to(dev)
    print('device: %s  torch %s' % (torch.cuda.get_device_name(0), torch.__version__))

    def torch_ops():
        out = R.match_batch_ref(priors, targets, ncs)
        return R.box_loss_ref(loc_data, out['loc_t'], out['pos'], cfg.bbox_alpha)

    ours = M.match_targets(priors, targets, ncs, loc_data)
    ref = R.match_batch_ref(priors, targets, ncs)
    same = all(torch.equal(ours[k], ref[k]) for k in ('conf_t', 'idx_t', 'pos', 'num_pos'))

    # the bare entry on prepared buffers
    split = R.split_targets(targets, ncs)
    truth = torch.cat([t for t, _, _ in split]).contiguous()
    label = torch.cat([l for _, l, _ in split]).int()
    crowd = torch.cat([c for _, _, c in split if c is not None]).contiguous() if a.crowds else None
    off = [a.gts * b for b in range(B + 1)]
    coff = [a.crowds * b for b in range(B + 1)]
    off_h, coff_h = (C.c_int32 * (B + 1))(*off), (C.c_int32 * (B + 1))(*coff)
    off_d, coff_d = torch.tensor(off, dtype=torch.int32).to(dev), torch.tensor(coff, dtype=torch.int32).to(dev)
    new = lambda dtype, *shape: torch.empty(*shape, dtype=dtype, device=dev)
    bufs = dict(loc_t=new(torch.float32, B, P, 4), gt_box_t=new(torch.float32, B, P, 4), conf_t=new(torch.int32, B, P),
                idx_t=new(torch.int32, B, P), pos=new(torch.uint8, B, P), num_pos=new(torch.int32, B),
                d_loc=new(torch.float32, B, P, 4), loss=new(torch.float32, 1))
    d = L.MatchDesc()
    d.priors, d.truth, d.label, d.gt_off, d.gt_off_host = priors.data_ptr(), truth.data_ptr(), label.data_ptr(), off_d.data_ptr(), \
        C.cast(off_h, C.c_void_p)
    if a.crowds:
        d.crowd, d.crowd_off, d.crowd_off_host = crowd.data_ptr(), coff_d.data_ptr(), C.cast(coff_h, C.c_void_p)
    d.loc_data = loc_data.data_ptr()
    for k, v in bufs.items():
        setattr(d, k, v.data_ptr())
    d.B, d.P, d.G, d.Gc = B, P, truth.size(0), 0 if crowd is None else crowd.size(0)
    d.pos_thresh, d.neg_thresh, d.crowd_thresh, d.bbox_alpha = 0.5, 0.4, 0.7, 1.5
    ws = torch.empty(int(L.lib().ymi_workspace_bytes(L.WS_MATCH, C.byref(d))), dtype=torch.uint8, device=dev)
    d.ws = ws.data_ptr()
    bare = lambda: L.check(L.lib().ymi_match_f32(C.byref(d), L.stream_ptr()), 'ymi_match_f32')

    k_med, k_min = timed(bare, a.warmup, a.reps)
    m_med, m_min = timed(lambda: M.match_targets(priors, targets, ncs, loc_data), a.warmup, a.reps)
    t_med, t_min = timed(torch_ops, a.warmup, a.reps)
    print(json.dumps({'shape': 'B%d P%d gts %d crowds %d' % (B, P, a.gts, a.crowds), 'kernels_us': round(k_med, 1),
                      'kernels_min_us': round(k_min, 1), 'match_targets_us': round(m_med, 1), 'match_targets_min_us': round(m_min, 1),
                      'torch_ops_us': round(t_med, 1), 'torch_ops_min_us': round(t_min, 1),
                      'torch_over_match_targets': round(t_med / m_med, 1), 'targets_equal_torch_ops': bool(same),
                      'workspace_MB': round(ws.numel() / 1e6, 2)}))


if __name__ == '__main__':
    main()
