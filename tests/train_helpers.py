"""What tests/test_gpu_heads_train.py, tests/test_gpu_fpn_train.py and tests/test_gpu_backbone_train.py share: the bar of every
comparison, the run-twice check, the grids of the inputs and the NaN-filled buffers of the entries that are called directly."""
import torch

import heads_train_ref as H
from helpers import rel_err, same_bits
from yolact_amd import _lib as L
from yolact_amd.layers import train_ops as TO

DEV = 'cuda:0'
EXACT_BAR = 8e-6
STORED_SLACK = 1e-6
GUARD = 256


def compare(record, name, got, want64, want32, against=None, slack=0.0):
    """Every quantity of the fp64 oracle, and nothing else, is in `got` with the oracle's shape and rel_err <= max(4 * rel_err(fp32
    oracle, fp64 oracle), EXACT_BAR) + slack.  The bar comes from the two oracles; `against` (default: the fp64 oracle) is what `got` is
    measured against.  record[name] keeps (rel_err, bar) per quantity for the module's summary."""
    against = want64 if against is None else against
    assert sorted(got) == sorted(want64), (sorted(got), sorted(want64))
    errs = {k: (rel_err(got[k], against[k]), max(4 * rel_err(want32[k], want64[k]), EXACT_BAR) + slack) for k in want64}
    record[name] = errs
    for k, (e, bar) in errs.items():
        print('%s %s: rel_err %.3e (bar %.3e)' % (name, k, e, bar))
    for k, (e, bar) in errs.items():
        assert got[k].shape == against[k].shape, (name, k)
        assert e <= bar, (name, k, e, bar)


def twice(run):
    """run() -> dict of CPU tensors, two times on the same inputs: the same bits."""
    a, b = run(), run()
    same_bits(a, b)
    return a


def grid_randn(g, shape, step, std=1.0, lim=4.0):
    return H.grid((torch.randn(*shape, generator=g) * std).clamp(-lim, lim), step)


def down(n):
    return (n - 1) // 2 + 1          # 3x3 / pad 1 and 1x1 / pad 0 at stride 2


def guarded(n):
    return torch.full((n + GUARD,), float('nan'), device=DEV)


def unguard(buf, shape):
    """Every element written, the band behind them untouched."""
    n = 1
    for s in shape:
        n *= s
    out = buf.cpu()
    assert not torch.isnan(out[:n]).any() and torch.isnan(out[n:]).all()
    return out[:n].view(*shape)


def nan_padded(g):
    gpad = torch.full(tuple(g.shape[:3]) + (g.shape[3] + 32,), float('nan'))          # the padding channels are never read
    gpad[..., :g.shape[3]] = g
    return gpad.to(DEV)


def zero_insert_gpu(g, w, Hh, W):
    """The route of conv2d_down's data gradient (train_ops._data_grad with zero_insert), built here from its parts, and what
    ymi_conv_dgrad_s2_nhwc_f32 is compared with: g [B,Ho,Wo,Cout] spread over a zeroed H x W map, then the stride-1 data gradient
    with the flipped filter on the engine -> dx on the CPU.  The added zeros change no bit of a sum, and a pixel no window reads
    (1x1) gets an exact +0.0."""
    Cout, Cin, k, _ = w.shape
    B = g.shape[0]
    ld = (Cout + 31) // 32 * 32                      # the engine takes multiples of 32 channels: zero channels, zero filter columns
    gz = torch.zeros(B, Hh, W, ld, device=DEV)
    gz[:, ::2, ::2, :Cout] = g.to(DEV)
    dx = torch.empty(B, Hh, W, Cin, device=DEV)
    TO._engine_conv(gz, ld, TO._pack_dgrad(w.to(DEV), ld), None, ld, Cin, k, k - 1 - k // 2, [(0, Cin, L.ACT_NONE, dx)])
    torch.cuda.synchronize()
    return dx.cpu()
