"""ymi_conv_wgrad_nhwc_h2 (csrc/conv_wgrad_h2.hip) on the GPU: the entry called directly, through train_ops.Conv under
wgrad_mode('fp16x2'), and through a whole training step, against fp64.  Every case runs twice and must give the same bits.

The cases, their inputs and the oracles are tests/wgrad_h2_ref.py's; tests/test_wgrad_h2_host.py shows on the CPU that each bar below
is met by the kernel's arithmetic and missed without the x_l g_h product or without one block of 32 channels of g.

Shape cases: rel_err (tests/gpu_utils.py) of dw and db against fp64 <= max(4 * rel_err(CPU fp32, fp64), 8e-6), the project's bar
(tests/test_gpu_class_loss.py).

Range cases, elementwise |got - fp64| <= E with
    E[k,co] = (3 * 2^-22 + P * 2^-24) * sum |a| |g|  +  2^-38 * (amax_x * sum |g| + amax_g * sum |a|),
every sum in fp64 over the positions the element reads.  Derived from the kernel as built:
  * the split.  t = v s is exact (s is a power of two; where v s underflows fp32, below 2^-126 in scaled units, the loss is far under
    the next term).  h = fp16(t): |t - h| <= 2^-11 |t|.  l = fp16(t - h): |t - h - l| <= 2^-11 |t - h| <= 2^-22 |t| while l is a
    normal fp16, and <= 2^-25 absolutely (half the subnormal spacing 2^-24) below that.  So each operand carries
    d <= 2^-22 |t| + 2^-25.
  * the products.  t_x t_g - (hh + hl + lh) = l_x l_g + the two split errors times the other operand:
    |l_x l_g| <= 2^-22 |t_x t_g|, and d_x |t_g| + d_g |t_x| <= 2 * 2^-22 |t_x t_g| + 2^-25 (|t_x| + |t_g|).  Undoing the scales divides
    by s_x s_g: the first three terms become 3 * 2^-22 |x g|; 2^-25 |t_x| / (s_x s_g) = 2^-25 |x| / s_g <= 2^-38 amax_g |x| because
    s_g >= 2^13 / amax_g (the rule puts the maximum at or above 2^13), and likewise for the other.  Summed over the positions: the
    first and the last term of E.
  * the additions.  A product passes through at most 16 roundings inside its MFMA, the 3 MFMAs of each of the chunk's K-steps
    (the 5 x 7 shape: chunks of 32 positions, 2 K-steps) and the 3 chunk partials: 16 + 6 + 3 = 25 <= P = 70 roundings of 2^-24
    relative each, on partial sums bounded by sum |a| |g|.  The issue's P * 2^-24 stands as the looser, shape-independent form.
  * undoing the scales multiplies by powers of two: exact, unless the result is a subnormal fp32 (2^-150 absolutely, far under E in
    the 2^-60 case, whose E is about 2^-132).
"""
import ctypes as C
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wgrad_h2_ref as R  # noqa: E402
from gpu_utils import rel_err  # noqa: E402
from helpers import same_bits  # noqa: E402
from train_helpers import DEV, guarded, twice  # noqa: E402
import yolact_amd  # noqa: E402
from yolact_amd import _lib as L  # noqa: E402
from yolact_amd.layers import train_ops as TO  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _restore():
    saved = yolact_amd.config.cfg.copy()
    yield
    yolact_amd.config.cfg.replace(saved)
    assert TO.get_wgrad_mode() == 'fp32'


def describe(x, gpad, Cout, k, stride):
    d = L.ConvWgradDesc()
    B, H, W, Cin = x.shape
    d.x, d.g = x.data_ptr(), gpad.data_ptr()
    d.B, d.H, d.W, d.Cin, d.Cout, d.ldg, d.kh, d.kw, d.pad, d.stride = B, H, W, Cin, Cout, gpad.shape[3], k, k, k // 2, stride
    return d


def chunk_count(d):
    """From the fp32 entry's workspace, chunks * (K * Cout + Cout) floats when Cout % 4 == 0."""
    assert d.Cout % 4 == 0
    return L.lib().ymi_workspace_bytes(L.WS_CONV_WGRAD, C.byref(d)) // (4 * (d.kh * d.kw * d.Cin * d.Cout + d.Cout))


def run_entry(x, g, ldg, k, stride, fill=0.0, want=(True, True), shift=0):
    """ymi_conv_wgrad_nhwc_h2 on x [B,H,W,Cin] and g [B,Ho,Wo,Cout] (CPU fp32), g's rows padded to ldg channels holding `fill` ->
    dict(dw [k*k*Cin, Cout], db [Cout]) on the CPU, what `want` leaves out missing.  The outputs sit in NaN-guarded buffers.  shift: x and
    g start that many floats behind a 16-byte boundary."""
    Cout = g.shape[3]
    gpad = torch.full(tuple(g.shape[:3]) + (ldg,), fill)
    gpad[..., :Cout] = g
    xd, gd = (torch.cat([torch.zeros(shift), t.reshape(-1)]).to(DEV)[shift:].view(t.shape) for t in (x, gpad))
    assert xd.data_ptr() % 16 == 4 * shift % 16 and gd.data_ptr() % 16 == 4 * shift % 16 and xd.is_contiguous()
    d = describe(xd, gd, Cout, k, stride)
    K = k * k * x.shape[3]
    dw, db = guarded(K * Cout), guarded(Cout)
    d.dw, d.db = (dw.data_ptr() if want[0] else None), (db.data_ptr() if want[1] else None)
    nbytes = L.lib().ymi_workspace_bytes(L.WS_CONV_WGRAD_H2, C.byref(d))
    assert nbytes > 0
    ws = torch.full((nbytes // 4,), float('nan'), device=DEV)
    d.ws, d.ws_bytes = ws.data_ptr(), nbytes
    L.check(L.lib().ymi_conv_wgrad_nhwc_h2(C.byref(d), L.stream_ptr()), 'ymi_conv_wgrad_nhwc_h2')
    torch.cuda.synchronize()
    out = {}
    if want[0]:
        out['dw'] = unguard_any(dw, (K, Cout))
    else:
        assert bool(torch.isnan(dw).all())
    if want[1]:
        out['db'] = unguard_any(db, (Cout,))
    else:
        assert bool(torch.isnan(db).all())
    return out


def unguard_any(buf, shape):
    """train_helpers.unguard for results that may hold NaN themselves: only the band behind them is checked."""
    n = 1
    for s in shape:
        n *= s
    out = buf.cpu()
    assert bool(torch.isnan(out[n:]).all())
    return out[:n].view(*shape)


def run_case(name, **kw):
    B, H, W, Cin, Cout, ldg, k, stride, kind = R.CASES[name]
    x, g = R.inputs(name)
    return twice(lambda: run_entry(x, g, ldg, k, stride, **kw))


SHAPE_CASES = [n for n, c in R.CASES.items() if c[8] == 'shape']


@pytest.mark.parametrize('name', SHAPE_CASES)
def test_shape_cases_meet_the_bar(name):
    got, ref = run_case(name), R.references(name)
    for q in ('dw', 'db'):
        assert not bool(torch.isnan(got[q]).any())
        e, bar = rel_err(got[q].double(), ref[q + '64']), R.bar(ref[q + '32'], ref[q + '64'])
        print('%s %s: rel_err %.3e (bar %.3e)' % (name, q, e, bar))
        assert e <= bar, (name, q, e, bar)


def test_the_padding_channels_of_g_are_never_part_of_a_sum():
    zeros = run_case('3x3_5x7')
    same_bits(zeros, run_case('3x3_5x7', fill=1e30))
    same_bits(zeros, run_case('3x3_5x7', fill=float('nan')))


def test_operands_off_a_16_byte_boundary_give_the_same_bits():
    """The bound pass reads 16 bytes per load only from aligned operands; the maximum has no order, so the bits cannot differ."""
    same_bits(run_case('3x3_5x7'), run_case('3x3_5x7', shift=1))
    same_bits(run_case('chunks'), run_case('chunks', shift=3))


def test_the_chunk_case_has_an_ordered_second_pass_to_run():
    B, H, W, Cin, Cout, ldg, k, stride, _ = R.CASES['chunks']
    x, g = R.inputs('chunks')
    d = describe(x, g, Cout, k, stride)
    n = chunk_count(d)
    assert n == 4 and B * H * W == 99                       # 32 + 32 + 32 + 3 positions
    part = lambda e: (4 * e + 15) // 16 * 16
    assert L.lib().ymi_workspace_bytes(L.WS_CONV_WGRAD_H2, C.byref(d)) == \
        part(n * Cin * Cout) + part(n * Cout) + 2 * part(n * 32 + 64) + part(2048)


@pytest.mark.parametrize('name', ['3x3_5x7', 'cout160'])
def test_a_null_output_leaves_the_other_ones_bits(name):
    full = run_case(name)
    only_b, only_w = run_case(name, want=(False, True)), run_case(name, want=(True, False))
    assert sorted(only_b) == ['db'] and sorted(only_w) == ['dw']
    same_bits(only_b['db'], full['db'], 'db')
    same_bits(only_w['dw'], full['dw'], 'dw')


@pytest.mark.parametrize('name', [n for n, c in R.CASES.items() if c[8] in R.RANGE_FINITE])
def test_range_cases_are_within_the_elementwise_bound(name):
    k, stride = R.CASES[name][6:8]
    x, g = R.inputs(name)
    got, ref = run_case(name), R.references(name)
    E = R.error_bound(x, g, k, stride)
    assert bool(torch.isfinite(got['dw']).all()) and bool(got['dw'].ne(0).any())
    ratio = ((got['dw'].double() - ref['dw64']).abs() / E).max().item()
    print('%s: largest |error| / E %.3e, largest |dw| %.3e' % (name, ratio, got['dw'].abs().max().item()))
    assert ratio <= 1.0, (name, ratio)
    e, bar = rel_err(got['db'].double(), ref['db64']), R.bar(ref['db32'], ref['db64'])
    assert e <= bar, (name, 'db', e, bar)


def positive_zero(t):
    return bool(t.view(torch.int32).eq(0).all())


def test_zero_operands_give_positive_zeros():
    got = run_case('range_g_zero')
    assert positive_zero(got['dw']) and positive_zero(got['db'])
    got = run_case('range_x_zero')
    assert positive_zero(got['dw'])
    ref = R.references('range_x_zero')
    assert rel_err(got['db'].double(), ref['db64']) <= R.bar(ref['db32'], ref['db64'])


def test_an_inf_in_g_reaches_its_whole_column():
    x, g = R.inputs('range_inf')
    B, H, W, Cin, Cout, ldg, k, stride, _ = R.CASES['range_inf']
    a, b = (run_entry(x, g, ldg, k, stride) for _ in range(2))
    col = R.INF_AT[3]
    for got in (a, b):
        assert not bool(torch.isfinite(got['dw'][:, col]).any()) and not bool(torch.isfinite(got['db'][col]))
    same_bits({k_: v.nan_to_num(7.0, 8.0, 9.0) for k_, v in a.items()}, {k_: v.nan_to_num(7.0, 8.0, 9.0) for k_, v in b.items()})


# ---- through the public interface ----------------------------------------------------------------------------------------------------
def conv_case(op):
    """-> (run(mode, backward_inside) -> dict of CPU tensors, fp64 and fp32 oracles of the parameter gradients)."""
    gen = torch.Generator().manual_seed(7)
    if op == 'conv2d_act':
        x, w, b = torch.randn(2, 5, 7, 64, generator=gen), torch.randn(40, 64, 3, 3, generator=gen) * 0.05, torch.randn(40, generator=gen)
        call = lambda x_, w_, b_: TO.conv2d_act(x_, w_, b_, 1, 'tanh')
        ref = lambda x_, w_, b_: torch.tanh(F.conv2d(x_, w_, b_, padding=1))
    elif op == 'conv2d_down':
        x, w, b = torch.randn(2, 7, 6, 32, generator=gen), torch.randn(48, 32, 3, 3, generator=gen) * 0.05, torch.randn(48, generator=gen)
        call = lambda x_, w_, b_: TO.conv2d_down(x_, w_, b_)
        ref = lambda x_, w_, b_: F.conv2d(x_, w_, b_, stride=2, padding=1)
    else:
        x, w, b = torch.randn(2, 6, 7, 32, generator=gen), torch.randn(64, 32, 1, 1, generator=gen) * 0.05, None
        call = lambda x_, w_, b_: TO.conv2d_plain(x_, w_, 2)
        ref = lambda x_, w_, b_: F.conv2d(x_, w_, None, stride=2)
    with torch.no_grad():
        shape = ref(x.permute(0, 3, 1, 2), w, b).shape
    gy = torch.randn(*shape, generator=gen)                                   # NCHW

    def oracle(dtype):
        leaves = [t if t is None else t.detach().to(dtype).clone().requires_grad_(True) for t in (x.permute(0, 3, 1, 2), w, b)]
        ref(*leaves).backward(gy.to(dtype))
        out = {'weight': leaves[1].grad.double()}
        if b is not None:
            out['bias'] = leaves[2].grad.double()
        return out

    def run(mode, backward_inside=True):
        leaves = [t if t is None else t.detach().to(DEV).requires_grad_(True) for t in (x, w, b)]
        gyd = gy.permute(0, 2, 3, 1).contiguous().to(DEV)
        with TO.wgrad_mode(mode):
            y = call(*leaves)
            if backward_inside:
                y.backward(gyd)
        if not backward_inside:
            y.backward(gyd)
        torch.cuda.synchronize()
        out = {'y': y.detach().cpu(), 'dx': leaves[0].grad.cpu(), 'weight': leaves[1].grad.cpu()}
        if b is not None:
            out['bias'] = leaves[2].grad.cpu()
        return out
    return run, oracle(torch.float64), oracle(torch.float32)


@pytest.mark.parametrize('op', ['conv2d_act', 'conv2d_down', 'conv2d_plain'])
def test_the_convolutions_follow_the_mode(op):
    run, o64, o32 = conv_case(op)
    got = twice(lambda: run('fp16x2'))
    base = run('fp32')
    for q in o64:
        e, bar = rel_err(got[q].double(), o64[q]), R.bar(o32[q], o64[q])
        print('%s %s: rel_err %.3e (bar %.3e)' % (op, q, e, bar))
        assert e <= bar, (op, q, e, bar)
    same_bits(got['y'], base['y'], 'y')
    same_bits(got['dx'], base['dx'], 'dx')
    assert not torch.equal(got['weight'], base['weight'])                     # another kernel: other bits
    # the backward uses the mode its forward saw, wherever it runs
    same_bits(run('fp16x2', backward_inside=False), got)
    same_bits(run('fp32', backward_inside=False), base)
    with TO.wgrad_mode('fp16x2'):                                             # and a forward outside is not touched by a backward inside
        pass
    assert TO.get_wgrad_mode() == 'fp32'


def test_deform_conv_follows_the_mode():
    import dcn_train_ref as D
    from test_gpu_dcn_train import gpu_op
    case = D.op_case(D.SMALL)
    g64, g32 = D.op_grads(case, torch.float64), D.op_grads(case, torch.float32)
    base = gpu_op(case)

    def run():
        with TO.wgrad_mode('fp16x2'):
            return gpu_op(case)
    got = twice(run)
    for q in ('weight', 'bias'):
        if q in g64:
            e, bar = rel_err(got[q].double(), g64[q].double()), R.bar(g32[q].double(), g64[q].double())
            print('deform_conv %s: rel_err %.3e (bar %.3e)' % (q, e, bar))
            assert e <= bar, (q, e, bar)
    for q in ('y', 'x', 'om'):
        same_bits(got[q], base[q], q)
    assert not torch.equal(got['weight'], base['weight'])


# ---- the whole step --------------------------------------------------------------------------------------------------------------------
class Spy:
    """Counts train_ops._weight_grad's calls per mode while a body runs."""

    def __enter__(self):
        self.modes, self.orig = [], TO._weight_grad

        def spy(*a, **kw):
            self.modes.append(a[10] if len(a) > 10 else kw.get('mode', 'fp32'))
            return self.orig(*a, **kw)
        TO._weight_grad = spy
        return self

    def __exit__(self, *exc):
        TO._weight_grad = self.orig


import train_step_ref as T  # noqa: E402


@pytest.mark.parametrize('name', T.GRADS_CASES)
def test_losses_and_gradients_of_a_step_under_the_mode(name):
    """tests/test_gpu_train_grads.py's own test, its oracle (train_net_ref.train_ref through train_step_ref.grads_oracles) and its own
    bars, with every forward inside wgrad_mode('fp16x2')."""
    import test_gpu_train_grads as G
    try:
        with Spy() as spy, TO.wgrad_mode('fp16x2'):
            G.test_losses_statistics_and_gradients(name)
    finally:
        G.RECORD.clear()
    assert len(spy.modes) > 100 and set(spy.modes) == {'fp16x2'}


from test_gpu_train_step import case  # noqa: E402,F401  (the module's fixture: the net, its state, the inputs)


def test_it_trains_under_the_mode(case, monkeypatch):
    """tests/test_gpu_train_step.py::test_it_trains, its criterion unchanged, with Trainer(net, wgrad='fp16x2')."""
    import test_gpu_train_step as S
    from yolact_amd.training import Trainer
    made = []

    def trainer(net):
        made.append(Trainer(net, wgrad='fp16x2'))
        return made[-1]
    monkeypatch.setattr(S, 'Trainer', trainer)
    with Spy() as spy:
        S.test_it_trains(case)
    assert len(made) == 1 and made[0].wgrad == 'fp16x2' and made[0].iteration >= 7
    assert set(spy.modes) == {'fp16x2'} and TO.get_wgrad_mode() == 'fp32'
