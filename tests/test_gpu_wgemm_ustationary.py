"""The U-stationary grouped GEMM of the Winograd path (csrc/wgemm.hip, wgemm_us_k: a component's filters in registers, only V
streams) against the kernel it is selected in front of (wgemm_k, forced by env YMI_WGEMM_STREAM_U=1): the same layer through
ymi_conv3x3_winograd_f32 with tile wg128x256h2 on V planes, once per kernel, in one process.  Same products, same K order, same
scaling: the layer output must be BIT-IDENTICAL (torch.equal, no tolerance).

  * the shipped shapes: proto.8 (138^2, 256 -> 256), 69^2 256 -> 256, 69^2 256 -> 512 (two column blocks), 35^2 256 -> 256, batch 8,
    F(4x4) and F(2x2);
  * T that is no multiple of 128 (ragged last row tile), T smaller than one block's share of a component (a single ragged tile,
    fewer row tiles than blocks per component), C = 128 / 64 (the shorter unrolled instances), Cout that is no multiple of 256;
  * C = 512 (U does not fit the register file), C = 96 (no unrolled instance) and Cout = 1080 at 69^2 with F(4x4) (the work split
    would be worse than the round robin's) take wgemm_k whatever the switch says, and still pass.
YMI_WGEMM_LOG=1 makes every launch name its kernel on stderr; the test reads that line."""
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from yolact_amd import _lib as L  # noqa: E402

TILE = L.TILE_WG_128x256 | L.TILE_H2


def _layer(shape, m, seed):
    B, Cin, H, W, Cout = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cin, H, W, generator=g) * torch.exp(torch.randn(B, Cin, 1, 1, generator=g))
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    return x, w, b


def _run(x, w, b, m, stream_u, capfd):
    """One launch with the switch set as asked; returns (output, the kernel the GEMM launch named)."""
    from gpu_utils import run_wino
    old = {k: os.environ.get(k) for k in ('YMI_WGEMM_STREAM_U', 'YMI_WGEMM_LOG')}
    os.environ['YMI_WGEMM_LOG'] = '1'
    if stream_u:
        os.environ['YMI_WGEMM_STREAM_U'] = '1'
    else:
        os.environ.pop('YMI_WGEMM_STREAM_U', None)
    try:
        capfd.readouterr()
        y = run_wino(x, w, b, None, L.ACT_RELU, TILE, m, v_planes=True)
        lines = [l for l in capfd.readouterr().err.splitlines() if l.startswith('wgemm: ')]
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    assert len(lines) == 1, lines
    return y, lines[0].split()[1]


SHIPPED = [(8, 256, 138, 138, 256), (8, 256, 69, 69, 256), (8, 256, 69, 69, 512), (8, 256, 35, 35, 256)]
EDGES = [(1, 256, 21, 30, 256),      # T = 48 (F(4x4)) / 165 (F(2x2)): ragged, fewer row tiles than blocks per component
         (1, 256, 5, 5, 256),        # T = 4 / 9: one ragged tile per component
         (3, 256, 37, 41, 256),      # T = 330 / 1197: no multiple of 128
         (2, 256, 35, 35, 360),      # Cout no multiple of 256 / 128: a ragged second column block
         (2, 256, 24, 24, 384),      # Ng = 256 + 128
         (2, 128, 69, 69, 128), (1, 64, 21, 30, 128), (1, 128, 9, 7, 36)]


@pytest.mark.parametrize('m', [4, 2])
@pytest.mark.parametrize('shape', SHIPPED + EDGES)
def test_u_stationary_is_bit_identical_to_the_streaming_kernel(shape, m, capfd):
    x, w, b = _layer(shape, m, 1000 + sum(shape) + m)
    y_us, k_us = _run(x, w, b, m, False, capfd)
    y_st, k_st = _run(x, w, b, m, True, capfd)
    assert (k_us, k_st) == ('u-stationary', 'u-streamed')
    assert torch.equal(y_us, y_st)
    assert torch.equal(y_us, _run(x, w, b, m, False, capfd)[0])           # and run to run
    if shape[0] * shape[2] * shape[3] <= 8 * 69 * 69:                     # fp32 torch on the CPU: the smaller layers
        ref = F.relu(F.conv2d(x, w, b, 1, 1))
        from gpu_utils import rel_err
        assert rel_err(y_us, ref) < (2e-5 if m == 2 else 5e-5)


@pytest.mark.parametrize('m', [4, 2])
@pytest.mark.parametrize('shape', [(3, 512, 18, 18, 512), (2, 96, 40, 33, 260), (8, 256, 69, 69, 1080)])
def test_layers_outside_the_register_budget_or_the_split_rule_stay_on_the_streaming_kernel(shape, m, capfd):
    """C = 512: 512 KB of planes per 256 columns; C = 96: no unrolled instance; Cout = 1080 at 69^2 and F(4x4): 180 (component, column
    block) pairs on 256 CUs leave one block per pair with all 21 row tiles against 15 items per block round robin (F(2x2): 80
    pairs, 3 blocks each — that one is taken)."""
    from gpu_utils import rel_err
    x, w, b = _layer(shape, m, 2000 + sum(shape) + m)
    y, k = _run(x, w, b, m, False, capfd)
    y_st, k_st = _run(x, w, b, m, True, capfd)
    if shape[4] == 1080 and m == 2:
        assert (k, k_st) == ('u-stationary', 'u-streamed')
    else:
        assert (k, k_st) == ('u-streamed', 'u-streamed')
    assert torch.equal(y, y_st)
    assert rel_err(y, F.relu(F.conv2d(x, w, b, 1, 1))) < (2e-5 if m == 2 else 5e-5)
