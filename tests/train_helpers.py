"""What tests/test_gpu_heads_train.py, tests/test_gpu_fpn_train.py and tests/test_gpu_backbone_train.py share: the bar of every
comparison, the run-twice check, the grids of the inputs and the NaN-filled buffers of the entries that are called directly."""
import torch

import heads_train_ref as H
from helpers import rel_err, same_bits

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
