"""train_ops.conv_mode('fp16x2') on the GPU: the device-side filter pack (csrc/conv_pack_h2.hip) against its exact oracle, the forward and
the data gradient of train_ops.Conv on the fp16x2 tiles against fp64, and a whole training step.  Every case runs twice and must give
the same bits.

The cases, their inputs and the oracles are tests/conv_h2_ref.py's; tests/test_conv_h2_host.py shows on the CPU that each bar below is
met by the mode's arithmetic and missed without the x_l w_h product or without one block of 32 input channels.

Pack: planes and winv equal engine.split2_planes_f16 of the torch packing (train_ops._pack_forward / _pack_dgrad) bit for bit.

Shape cases: rel_err (tests/gpu_utils.py) of y, dx and, with wgrad_mode('fp16x2') too, dw and db against fp64
<= max(4 * rel_err(CPU fp32, fp64), 8e-6), the project's bar (tests/test_gpu_class_loss.py).

Range cases (a plain 3x3 on 2 x 5 x 7 x 64 -> 40, K = k k Cin = 576), elementwise |got - fp64| <= E with
    E[m,co] = (3 * 2^-22 + K * 2^-24) * sum |x| |w|  +  2^-38 * (amax_x * sum |w[co]| + rowmax_w[co] * sum |x|),
every sum in fp64 over what the output reads.  Derived from the tiles as shipped (csrc/gemm_h2.h split8h for x, csrc/conv_pack_h2.hip for
w, v_mfma_f32_32x32x16_f16 in csrc/conv_igemm.hip and csrc/dcn.hip):
  * the split.  t = v s is exact (s is a power of two).  h = fp16(t): |t - h| <= 2^-11 |t|.  l = fp16(t - h): |t - h - l| <= 2^-22 |t|
    while l is a normal fp16, and <= 2^-25 absolutely (half the subnormal spacing 2^-24) below that: d <= 2^-22 |t| + 2^-25 per operand.
  * the products.  t_x t_w - (hh + hl + lh) = l_x l_w + the two split errors times the other operand: |l_x l_w| <= 2^-22 |t_x t_w|, and
    d_x |t_w| + d_w |t_x| <= 2 * 2^-22 |t_x t_w| + 2^-25 (|t_x| + |t_w|).  Undoing the scales divides by s_x s_w[co]: the first three
    terms become 3 * 2^-22 |x w|.  The filter scale is PER ROW: s_w[co] >= 2^13 / rowmax_w[co] (the rule puts the row's maximum at or
    above 2^13), so 2^-25 |t_x| / (s_x s_w[co]) = 2^-25 |x| / s_w[co] <= 2^-38 rowmax_w[co] |x|; the activation scale is per tensor,
    s_x >= 2^13 / amax_x, so the other term is <= 2^-38 amax_x |w|.  Summed over the taps: the first and the last term of E.
  * the additions.  A product is rounded at most 16 times inside its own MFMA (16 products per instruction), then once by each later
    MFMA on the accumulator: 3 per 16 of K, 3 K / 16 in all; the K-split tiles add the partial sums of 4 waves (3 more) and the
    epilogue's scale is a power of two (exact) with no bias here: 16 + 3 K / 16 + 3 roundings of 2^-24 relative each, on partial sums
    bounded by sum |x| |w|.  At K = 576 that is 127 <= K, and 16 + 3 K / 16 + 3 <= K from K = 24 on (the smallest K is 32): the issue's
    K * 2^-24 stands as the looser, shape-independent form.
  * undoing the scales multiplies by powers of two, one after the other: exact unless the result is a subnormal fp32 (no case here).
The same E holds for dx, which is the same launch on g with the flipped, transposed filters (rows = input channels, K = k k Cout: zero
padding columns add nothing).

Which convolutions the mode moves is train_ops' static rule (_h2_pays: the 3x3 ones; _h2_tile: their tile).  TILES below states, per
case, the tile of every ymi_conv2d_nhwc_f32 launch, read from the descriptor by a spy on the binding: the cases hit the pipelined
tile above and below M = 16384, the engine's own choice, its 128x32 mapped to 64x32k2, and the classes that stay on the fp32 tiles
(1x1: tile 0, the parent's bits, no pack launch).

Measured on the MI355X: the pack equals the torch packing bit for bit in all 18 (case, layout) pairs; shape cases 9e-8 .. 6e-7 against
fp64 (bar 8e-6); largest |error| / E of the range cases 8.7e-3 (y) and 2.3e-2 (dx) on 2^U(-20,20), 1.3e-3 / 2.9e-3 at 2^-60,
1.5e-3 / 3.3e-3 at 2^50; pred_outs of the whole-step cases against the fp64 oracle, fp32 tiles / fp16x2 tiles: conf 5.9e-6 / 5.5e-6,
loc 3.5e-6 / 3.5e-6, mask 1.5e-5 / 1.4e-5, proto 3.0e-6 / 3.0e-6, segm 1.2e-5 / 1.3e-5 (batch statistics).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_h2_ref as R  # noqa: E402
import train_step_ref as T  # noqa: E402
from gpu_utils import rel_err  # noqa: E402
from helpers import same_bits  # noqa: E402
from train_helpers import DEV, GUARD, guarded, twice  # noqa: E402
import yolact_amd  # noqa: E402
from yolact_amd import _lib as L  # noqa: E402
from yolact_amd.layers import train_ops as TO  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = 0x5a5a


@pytest.fixture(autouse=True)
def _restore():
    saved = yolact_amd.config.cfg.copy()
    yield
    yolact_amd.config.cfg.replace(saved)
    assert TO.get_wgrad_mode() == 'fp32' and TO.get_conv_mode() == 'fp32'


class EntrySpy:
    """Records every call of one entry of the binding while a body runs: .calls holds the fields of interest of each call's descriptor."""

    def __init__(self, name, fields):
        self.name, self.fields, self.calls = name, fields, []

    def __enter__(self):
        lib = L.lib()
        self.orig = getattr(lib, self.name)

        def spy(dref, stream):
            self.calls.append(tuple(getattr(dref._obj, f) for f in self.fields))
            return self.orig(dref, stream)
        setattr(lib, self.name, spy)
        return self

    def __exit__(self, *exc):
        setattr(L.lib(), self.name, self.orig)


# ---- 1. the pack against the exact oracle ----------------------------------------------------------------------------------------------
def run_pack(ws, mode, ld, shift=0):
    """ymi_conv_pack_h2_f32 on the CPU tensors ws -> (planes int16 [2][RowsPad][Kp], winv [RowsPad], w32 [RowsPad][Kp]) as numpy, from
    guarded buffers.  shift: every source starts that many floats behind a 16-byte boundary."""
    wd = [torch.cat([torch.zeros(shift), w.reshape(-1)]).to(DEV)[shift:].view(w.shape) for w in ws]
    assert all(t.data_ptr() % 16 == 4 * shift % 16 and t.is_contiguous() for t in wd)
    Cin, k = ws[0].shape[1], ws[0].shape[2]
    rows = sum(w.shape[0] for w in ws) if mode == 0 else Cin
    rows_pad, Kp = (rows + 127) // 128 * 128, k * k * (Cin if mode == 0 else ld)
    planes = torch.full((2 * rows_pad * Kp + GUARD,), SENTINEL, dtype=torch.int16, device=DEV)
    winv, w32 = guarded(rows_pad), guarded(rows_pad * Kp)
    d = L.ConvPackDesc()
    for i, t in enumerate(wd):
        d.w[i], d.cout[i] = t.data_ptr(), t.shape[0]
    d.planes, d.winv, d.w32 = planes.data_ptr(), winv.data_ptr(), w32.data_ptr()
    d.n, d.Cin, d.k, d.mode, d.ld = len(wd), Cin, k, mode, ld
    L.check(L.lib().ymi_conv_pack_h2_f32(C.byref(d), L.stream_ptr()), 'ymi_conv_pack_h2_f32')
    torch.cuda.synchronize()
    planes, winv, w32 = planes.cpu(), winv.cpu(), w32.cpu()
    assert bool(planes[2 * rows_pad * Kp:].eq(SENTINEL).all()) and bool(torch.isnan(winv[rows_pad:]).all())
    assert bool(torch.isnan(w32[rows_pad * Kp:]).all())
    return dict(planes=planes[:2 * rows_pad * Kp].view(2, rows_pad, Kp), winv=winv[:rows_pad], w32=w32[:rows_pad * Kp].view(rows_pad, Kp))


@pytest.mark.parametrize('mode', [0, 1], ids=['forward', 'dgrad'])
@pytest.mark.parametrize('name', list(R.PACK_CASES))
def test_the_pack_is_the_torch_packing_bit_for_bit(name, mode):
    ws, ld = R.pack_inputs(name), R.PACK_CASES[name][1]
    got = twice(lambda: run_pack(ws, mode, ld))
    planes, winv = R.pack_torch(ws, mode, ld)
    assert np.array_equal(got['planes'].numpy(), planes), name
    assert np.array_equal(got['winv'].numpy().view(np.int32), winv.view(np.int32)), name
    assert np.array_equal(got['w32'].numpy().view(np.int32), R.packing_np([w.numpy() for w in ws], mode, ld).view(np.int32)), name
    # sources 4 and 12 bytes off a 16-byte boundary: the same bits
    for shift in (1, 3):
        same_bits(run_pack(ws, mode, ld, shift=shift), got)


def test_the_pack_without_w32_and_through_train_ops():
    ws = R.pack_inputs('head3')
    want = R.pack_torch(ws, 1, 352)
    planes, winv = TO._pack_h2([w.to(DEV) for w in ws], 32, 3, 1, 352)
    torch.cuda.synchronize()
    assert np.array_equal(planes.cpu().numpy(), want[0]) and np.array_equal(winv.cpu().numpy().view(np.int32), want[1].view(np.int32))


def test_non_finite_rows_get_scale_one():
    """The helper's rule, stated in the header: a row maximum of Inf or NaN (a NaN anywhere in the row) gives s = 1."""
    w = R.pack_inputs('1x1_5')[0].clone()
    w[1, 3], w[2, 4] = float('inf'), float('nan')
    got = run_pack([w], 0, 0)
    assert got['winv'][1] == 1 and got['winv'][2] == 1 and got['winv'][0] != 1
    h = got['planes'][0].view(torch.float16)
    assert bool(torch.isinf(h[1, 3])) and bool(torch.isnan(h[2, 4])) and bool(torch.isfinite(h[0]).all())
    assert torch.equal(h[1, :3].float(), w[1, :3, 0, 0].half().float())       # s = 1: plane 0 is fp16(w) itself


# ---- 2. the shape cases through the public interface -----------------------------------------------------------------------------------
def call_op(name, x, params):
    op, xs, layers, stride = R.CASES[name]
    k = layers[0][0][2]
    if op == 'conv2d_act':
        return (TO.conv2d_act(x, params[0][0], params[0][1], k // 2, layers[0][2]),)
    if op == 'conv2d_down':
        return (TO.conv2d_down(x, params[0][0], params[0][1], layers[0][2]),)
    if op == 'conv2d_plain':
        return (TO.conv2d_plain(x, params[0][0], stride),)
    return TO.conv2d_multi(x, [(w, b, act) for (w, b), (_, _, act) in zip(params, layers)], k // 2)


def run_case(name, conv, wgrad='fp32', backward_inside=True, tiles=None, inputs=None):
    """The case's public function under the two modes (conv None: no context at all) -> dict of CPU tensors named as R.oracle names
    them.  tiles (a list) receives ymi_conv_desc.tile of every ymi_conv2d_nhwc_f32 launch."""
    import contextlib
    x, params, gys = R.inputs(name) if inputs is None else inputs
    xd = x.to(DEV).requires_grad_(True)
    pd = [(w.to(DEV).requires_grad_(True), None if b is None else b.to(DEV).requires_grad_(True)) for w, b in params]
    gd = [g.to(DEV) for g in gys]
    with EntrySpy('ymi_conv2d_nhwc_f32', ('tile',)) as spy:
        with contextlib.nullcontext() if conv is None else TO.conv_mode(conv), TO.wgrad_mode(wgrad):
            ys = call_op(name, xd, pd)
            if backward_inside:
                torch.autograd.backward(ys, gd)
        if not backward_inside:
            torch.autograd.backward(ys, gd)
        torch.cuda.synchronize()
    if tiles is not None:
        tiles += [t for (t,) in spy.calls]
    out = {'dx': xd.grad.cpu()}
    for i, (y, (w, b)) in enumerate(zip(ys, pd)):
        out['y%d' % i], out['w%d' % i] = y.detach().cpu(), w.grad.cpu()
        if b is not None:
            out['b%d' % i] = b.grad.cpu()
    return out


H2, PIPE = L.TILE_H2, L.TILE_H2 | L.TILE_DCNP
PIPE_SMALL, PIPE_BIG, K4, MAPPED = PIPE | L.DCNP_32x128, PIPE | L.DCNP_64x128_W8, H2 | L.TILE_32x32_K4, H2 | L.TILE_64x32_K2
# case -> the tiles of its launches in order: the forward, then dx (none where the tap-exact stride-2 kernel computes it)
FP32 = L.TILE_AUTO                              # the class stays on the exact-fp32 tiles: the descriptor of the default path
TILES = {
    'act_tanh': [K4, K4],                       # tanh: not the pipelined kernel's; dx 64 -> 64 does not fill 128 columns
    'down': [K4, K4],                           # dx by the zero-insert route: a stride-1 launch
    'plain_s2': [FP32],                         # 1x1: stays (Kpad / 32 = 1 besides); dx is ymi_conv_dgrad_s2_nhwc_f32
    'head3': [K4, K4],                          # three outputs; dx 352 -> 32
    '1x1_cin32': [FP32, FP32],                  # 1x1: stays, both ways
    'big_m': [PIPE_BIG, K4],                    # M = 16384 and 128 columns; dx 128 -> 32
    'wide': [PIPE_SMALL, PIPE_SMALL],
    'narrow_big_m': [MAPPED, MAPPED],           # the engine's 128x32, which has no fp16x2 variant (dx: 32 -> 32)
    'plain3_s2': [K4],                          # dx is ymi_conv_dgrad_s2_nhwc_f32: no second launch
}
ROUTED = {name: [t != FP32 for t in (ts + [False])[:2]] for name, ts in TILES.items()}       # (forward, dx) on the fp16x2 tiles


def test_every_branch_of_the_rule_is_in_the_cases():
    assert sorted(TILES) == sorted(R.CASES)
    assert {t for ts in TILES.values() for t in ts} == {FP32, K4, PIPE_SMALL, PIPE_BIG, MAPPED}
    assert TO._h2_pays(3) and not TO._h2_pays(1)


@pytest.mark.parametrize('name', list(R.CASES))
def test_shape_cases_meet_the_bar(name):
    o64, o32 = R.oracle(name, torch.float64), R.oracle(name, torch.float32)
    tiles = []
    got = twice(lambda: run_case(name, 'fp16x2', tiles=tiles))
    assert tiles == TILES[name] * 2, (name, tiles)
    both = twice(lambda: run_case(name, 'fp16x2', 'fp16x2'))
    assert sorted(got) == sorted(o64)
    for q in sorted(o64):
        src = both if q[0] in 'wb' else got
        e, bar = rel_err(src[q].double(), o64[q]), R.bar(o32[q], o64[q])
        print('%s %s: rel_err %.3e (bar %.3e)' % (name, q, e, bar))
        assert src[q].shape == o64[q].shape and e <= bar, (name, q, e, bar)
    for q in got:
        if q[0] not in 'wb':
            same_bits(both[q], got[q], q)       # the two switches are independent: y and dx do not read the wgrad mode


# ---- 3. the range cases ------------------------------------------------------------------------------------------------------------------
def run_plain(x, w, gy=None, conv='fp16x2'):
    xd, wd = x.to(DEV).requires_grad_(gy is not None), w.to(DEV)
    with TO.conv_mode(conv):
        y = TO.conv2d_plain(xd, wd, 1)
        if gy is not None:
            y.backward(gy.to(DEV))
    torch.cuda.synchronize()
    return {'y': y.detach().cpu()} if gy is None else {'y': y.detach().cpu(), 'dx': xd.grad.cpu()}


@pytest.mark.parametrize('kind', R.RANGE)
def test_range_cases_are_within_the_elementwise_bound(kind):
    x, w, gy = R.range_inputs(kind)
    k = w.shape[2]
    got = twice(lambda: run_plain(x, w, gy))
    for q, (a, f, pad) in (('y', (x, w, k // 2)), ('dx', R.dgrad_as_forward(gy, w, k // 2))):
        want, E = R.conv64(a, f, None, pad, 1), R.error_bound(a, f, k, pad, 1)
        assert bool(torch.isfinite(got[q]).all()) and bool(got[q].ne(0).any())
        ratio = ((got[q].double() - want).abs() / E).max().item()
        print('%s %s: largest |error| / E %.3e, largest |value| %.3e' % (kind, q, ratio, got[q].abs().max().item()))
        assert ratio <= 1.0, (kind, q, ratio)


# ---- 4. exact answers ----------------------------------------------------------------------------------------------------------------------
def test_small_integers_give_the_fp64_result_exactly():
    gen = torch.Generator().manual_seed(5)
    x = torch.randint(-8, 9, (2, 5, 7, 64), generator=gen).float()
    w = torch.randint(-8, 9, (40, 64, 3, 3), generator=gen).float()
    gy = torch.randint(-8, 9, (2, 5, 7, 40), generator=gen).float()
    got = twice(lambda: run_plain(x, w, gy))
    assert torch.equal(got['y'].double(), R.conv64(x, w, None, 1, 1))
    g, wt, pad = R.dgrad_as_forward(gy, w, 1)
    assert torch.equal(got['dx'].double(), R.conv64(g, wt, None, pad, 1))


def test_a_power_of_two_on_x_comes_out_bit_for_bit():
    x, w = R.inputs('act_tanh')[0], R.inputs('act_tanh')[1][0][0]
    same_bits(run_plain(x * 128, w)['y'], run_plain(x, w)['y'] * 128)


def test_a_zero_input_gives_positive_zero_or_exactly_the_bias():
    x, ((w, b),), _ = R.inputs('act_tanh')
    y = twice(lambda: run_plain(torch.zeros_like(x), w))['y']
    assert bool(y.view(torch.int32).eq(0).all())
    with TO.conv_mode('fp16x2'), torch.no_grad():
        yb = TO.conv2d_act(torch.zeros_like(x).to(DEV), w.to(DEV), b.to(DEV), 1, None).cpu()
    same_bits(yb, b.view(1, 1, 1, -1).expand_as(yb).contiguous())


def test_an_inf_in_x_reaches_every_output_that_reads_it():
    x, w = R.inputs('act_tanh')[0].clone(), R.inputs('act_tanh')[1][0][0]
    x[1, 2, 3, 7] = float('inf')
    reads = R.conv64(torch.isinf(x).float(), torch.ones_like(w), None, 1, 1) > 0
    a, b = run_plain(x, w)['y'], run_plain(x, w)['y']
    assert int(reads.sum()) == 9 * 40 and not bool(torch.isfinite(a[reads]).any())
    same_bits(a.nan_to_num(7.0, 8.0, 9.0), b.nan_to_num(7.0, 8.0, 9.0))


# ---- 5. the switch ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['act_tanh', 'down', 'plain3_s2', 'plain_s2', '1x1_cin32'])
def test_the_switch(name):
    fwd, dx = ROUTED[name]
    with EntrySpy('ymi_conv_pack_h2_f32', ('mode',)) as packs:
        TO._conv.__dict__.pop('mode', None)                                   # a thread that never set the mode
        never = run_case(name, None)
        tiles = []
        base = run_case(name, 'fp32', tiles=tiles)
        assert packs.calls == [] and set(tiles) == {L.TILE_AUTO}
        got = run_case(name, 'fp16x2')
        assert [m for (m,) in packs.calls] == [0] * fwd + [1] * dx
    same_bits(base, never)
    # the classes the rule routes get other tiles, hence other bits; the 1x1 convolutions and the tap-exact stride-2 dx keep theirs
    assert torch.equal(got['y0'], base['y0']) != fwd
    assert torch.equal(got['dx'], base['dx']) != dx
    if not fwd:
        same_bits(got, base)
    # dw and db never read the mode: they keep their bits wherever their operands do.  Without an activation g is dy itself; under
    # tanh g = dy * (1 - y^2) follows the forward's y, so there the bits move with y, not with the weight-gradient kernel
    if name != 'act_tanh':
        for q in got:
            if q[0] in 'wb':
                same_bits(got[q], base[q], q)
    # the backward uses the mode its forward saw, wherever it runs
    same_bits(run_case(name, 'fp16x2', backward_inside=False), got)
    same_bits(run_case(name, 'fp32', backward_inside=False), base)


def test_deform_conv_follows_the_mode():
    """deform_conv's GEMM is Conv as a 1 x 1 convolution and has no code of its own for the mode: it follows the rule, which leaves
    the pointwise class on the fp32 tiles, so under the mode it meets tests/test_gpu_dcn_train.py's own bars with its own bits."""
    import dcn_train_ref as D
    import test_gpu_dcn_train as G
    case = D.op_case(D.SMALL)
    g64, g32 = G.oracles(D.SMALL, case)
    base = G.gpu_op(case)

    def run():
        with TO.conv_mode('fp16x2'):
            return G.gpu_op(case)
    with EntrySpy('ymi_conv_pack_h2_f32', ('mode',)) as packs:
        got = twice(run)
    assert packs.calls == []
    G.compare(D.SMALL + ' conv fp16x2', got, g64, g32)
    same_bits(got, base)


# ---- 6. the whole step -------------------------------------------------------------------------------------------------------------------------
_ORACLES = {}


def cached_oracles(name, *a, **kw):
    """train_step_ref.grads_oracles once per case for every test of this module (the tests only read it)."""
    key = (name, a, tuple(sorted(kw.items())))
    if key not in _ORACLES:
        _ORACLES[key] = _GRADS_ORACLES(name, *a, **kw)
    return _ORACLES[key]


_GRADS_ORACLES = T.grads_oracles


def preds_deviation(name):
    """The largest rel_err of forward_train's outputs against the fp64 oracle's, per mode."""
    res, _, inputs = cached_oracles(name)
    want = res[torch.float64]['preds']
    net, images, targets, masks, num_crowds, batch_stats = T.build_grads_case(DEV, name)
    state = {k: v.detach().clone() for k, v in net.state_dict().items()}
    out = {}
    for mode in TO.CONV_MODES:
        net.load_state_dict(state)
        with torch.no_grad(), TO.conv_mode(mode):
            got = net.forward_train(images, batch_stats)
        torch.cuda.synchronize()
        out[mode] = {k: rel_err(got[k].detach().cpu().double(), want[k].double())
                     for k in want if k in got and k != 'priors' and got[k].shape == want[k].shape}
    return out


@pytest.mark.parametrize('wgrad', ['fp32', 'fp16x2'])
@pytest.mark.parametrize('name', T.GRADS_CASES)
def test_losses_and_gradients_of_a_step_under_the_mode(name, wgrad, monkeypatch):
    """tests/test_gpu_train_grads.py's own test, its oracle (train_net_ref.train_ref through train_step_ref.grads_oracles) and its own
    bars, with every forward inside conv_mode('fp16x2'), alone and with wgrad_mode('fp16x2') too.  The cases keep 16 times the fp32
    deviation as margin on their discrete decisions; the printed deviation of pred_outs shows the mode's is of the same class."""
    import test_gpu_train_grads as G
    monkeypatch.setattr(T, 'grads_oracles', cached_oracles)
    if wgrad == 'fp32':
        dev = preds_deviation(name)
        assert dev['fp32'] and sorted(dev['fp32']) == sorted(dev['fp16x2'])
        for k in sorted(dev['fp32']):
            print('%s pred_outs %s: rel_err against fp64: fp32 tiles %.3e, fp16x2 tiles %.3e' % (name, k, dev['fp32'][k], dev['fp16x2'][k]))
    try:
        with EntrySpy('ymi_conv_pack_h2_f32', ('mode',)) as packs, TO.conv_mode('fp16x2'), TO.wgrad_mode(wgrad):
            G.test_losses_statistics_and_gradients(name)
    finally:
        G.RECORD.clear()
    modes = [m for (m,) in packs.calls]
    assert modes.count(0) > 40 and modes.count(1) > 25        # the 3x3 convolutions of two runs of the step


from test_gpu_train_step import case  # noqa: E402,F401  (the module's fixture: the net, its state, the inputs)


def test_it_trains_under_the_mode(case, monkeypatch):
    """tests/test_gpu_train_step.py::test_it_trains, its criterion unchanged, with Trainer(net, conv='fp16x2', wgrad='fp16x2')."""
    import test_gpu_train_step as S
    from yolact_amd.training import Trainer
    made = []

    def trainer(net):
        made.append(Trainer(net, conv='fp16x2', wgrad='fp16x2'))
        return made[-1]
    monkeypatch.setattr(S, 'Trainer', trainer)
    with EntrySpy('ymi_conv_pack_h2_f32', ('mode',)) as packs:
        S.test_it_trains(case)
    assert len(made) == 1 and made[0].conv == 'fp16x2' and made[0].wgrad == 'fp16x2' and made[0].iteration >= 7
    assert len(packs.calls) > 200 and TO.get_conv_mode() == 'fp32' and TO.get_wgrad_mode() == 'fp32'
