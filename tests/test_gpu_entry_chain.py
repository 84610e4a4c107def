"""The ENTRY form of ymi_pointwise_chain_f32 on the GPU (csrc/chain.hip, chain_h2_k<64, true>): layer0.0's projection shortcut
(1x1, 64 -> 256, no activation) computed inside the layer0.0.conv3 + layer0.1.conv1 launch instead of being written by a launch of
its own and read back as the residual.

Kernel level: y, z and both magnitude bounds against fp64 at the bars of test_pointwise_chain_matches_fp64 (y: that test's 5e-7 once
for each of the two K = 64 sums), y no worse than twice the error of the two-launch form on the same inputs (the shortcut through
ymi_conv2d_nhwc_f32 on the shipped tile, then the chain with `res`: the same products in another order), bit-reproducible, rows
beyond M untouched, and a descriptor whose new fields are zero is the launch it always was.  Plan level: the form installs (forced at
batch 2, from the shipped table at batch 8) and the network's outputs agree with the plan that keeps the shortcut launch."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from yolact_amd import _lib as L  # noqa: E402
from yolact_amd import tune_table as TT  # noqa: E402
from yolact_amd.engine import Packed  # noqa: E402
from yolact_amd.utils.synth import synth_images, synth_state_dict  # noqa: E402

DEV = torch.device('cuda', 0)
SENTINEL = -12345.5
PAD_ROWS = 40            # rows allocated beyond M: no launch may touch them

# (B, H, W): one pixel | 70 rows = three tiles, ragged tail | 106 tiles, fewer than the number of blocks | 520 tiles > 2 x 256: both
# register sets, both LDS buffers and the extra GEMM-2 iteration
SHAPES = [(1, 1, 1), (2, 5, 7), (3, 33, 34), (1, 131, 127)]


@functools.lru_cache(maxsize=None)
def _inputs(B, H, W):
    M = B * H * W
    g = torch.Generator().manual_seed(7300 + M)
    t = torch.randn(M, 64, generator=g) * 3
    x0 = torch.randn(M, 64, generator=g).relu_() * 2
    wa = torch.randn(256, 64, generator=g) / 8
    ba = torch.randn(256, generator=g) * 0.3
    wd = torch.randn(256, 64, generator=g) / 8
    bd = torch.randn(256, generator=g) * 0.3
    wb = torch.randn(64, 256, generator=g) / 16
    bb = torch.randn(64, generator=g) * 0.1
    return t, x0, wa, ba, wd, bd, wb, bb


def _act(v, act):
    return torch.relu(v) if act == L.ACT_RELU else F.leaky_relu(v, 0.1)


@functools.lru_cache(maxsize=None)
def _fp64(B, H, W, act, st=1.0, s0=1.0):
    t, x0, wa, ba, wd, bd, wb, bb = _inputs(B, H, W)
    r = (x0.double() * s0) @ wd.double().t() + bd.double()
    yr = _act((t.double() * st) @ wa.double().t() + ba.double() + r, act)
    return yr, _act(yr @ wb.double().t() + bb.double(), act)


@functools.lru_cache(maxsize=None)
def _filters(B, H, W):
    t, x0, wa, ba, wd, bd, wb, bb = _inputs(B, H, W)
    pa = Packed(wa.view(256, 64, 1, 1), ba, None, 1, 0, None, DEV)
    pd = Packed(wd.view(256, 64, 1, 1), bd, None, 1, 0, None, DEV)
    pb = Packed(wb.view(64, 256, 1, 1), bb, None, 1, 0, None, DEV)
    return pa, pd, pb


def _shipped_shortcut_tile():
    """The tile the shipped table runs layer0.0.down on at batch 8 (a pipelined fp16x2 tile)."""
    v = TT.load_tune_table(DEV)[TT.conv_key((8, 138, 138, 64, 256, 1, 1, 1, 0, 0, 1, 64), 'h2')]
    tile, split = TT.direct_parts(v)
    assert split == 0 and tile & L.TILE_H2
    return tile


def _launch(B, H, W, act, form, with_z=True, ldx0=64, in_place=None, st=1.0, s0=1.0, zero_new=False):
    """form 'entry': one launch with x0 | 'two': the shortcut through ymi_conv2d_nhwc_f32 on the shipped tile, then the chain with
    `res` | 'plain': the chain with a given residual tensor (the fp32 shortcut of torch) and, with zero_new, every new field written
    as zero explicitly.  in_place 'x' / 'x0': z is written over that input (same base, same row stride).
    Returns (y, z or None, y_amax, z_amax, sentinels_ok) on the CPU."""
    t, x0, wa, ba, wd, bd, wb, bb = _inputs(B, H, W)
    M = B * H * W
    pa, pd, pb = _filters(B, H, W)
    pla, sca, _ = pa.h2()
    pld, scd, winvd = pd.h2()
    plb, scb, _ = pb.h2()
    lib, s = L.lib(), L.stream_ptr()
    td = (t * st).contiguous().to(DEV)
    x0d = torch.full((M, ldx0), float('nan'), device=DEV)          # (channels [64, ldx0) are never read: NaN would show)
    x0d[:, :64] = (x0 * s0).to(DEV)
    y = torch.full((M + PAD_ROWS, 256), SENTINEL, device=DEV)
    amax = torch.zeros(5 * 1024, device=DEV)
    L.check(lib.ymi_amax_f32(td.data_ptr(), td.numel(), amax.data_ptr(), s), 'amax')
    x0c = x0d[:, :64].contiguous()
    L.check(lib.ymi_amax_f32(x0c.data_ptr(), x0c.numel(), amax.data_ptr() + 12288, s), 'amax')
    d = L.ChainDesc()
    d.x, d.y, d.M, d.ldx, d.ldy = td.data_ptr(), y.data_ptr(), M, 64, 256
    d.w_a_h2, d.scale_a_h2, d.bias_a, d.cout_pad_a = pla.data_ptr(), sca.data_ptr(), pa.bias.data_ptr(), pa.CoutPad
    d.k_a, d.n_a, d.n_b, d.act_a, d.act_b = 64, 256, 64, act, act
    d.x_amax, d.y_amax, d.z_amax = amax.data_ptr(), amax.data_ptr() + 4096, amax.data_ptr() + 8192
    z = None
    if with_z:
        if in_place == 'x':
            z, ldz = td, 64
        elif in_place == 'x0':
            z, ldz = x0d, ldx0
        else:
            z, ldz = torch.full((M + PAD_ROWS, 64), SENTINEL, device=DEV), 64
        d.z, d.ldz, d.w_b_h2, d.scale_b_h2, d.bias_b, d.cout_pad_b = z.data_ptr(), ldz, plb.data_ptr(), scb.data_ptr(), pb.bias.data_ptr(), pb.CoutPad
    keep = []
    if form == 'entry':
        d.x0, d.ldx0, d.x0_amax = x0d.data_ptr(), ldx0, amax.data_ptr() + 12288
        d.w_d_h2, d.scale_d_h2, d.bias_d, d.cout_pad_d = pld.data_ptr(), scd.data_ptr(), pd.bias.data_ptr(), pd.CoutPad
    else:
        if form == 'two':
            r = torch.full((M, 256), float('nan'), device=DEV)
            cd = L.ConvDesc()
            cd.x, cd.w, cd.bias = x0d.data_ptr(), pd.w.data_ptr(), pd.bias.data_ptr()
            cd.scale = pd.scale.data_ptr() if pd.scale is not None else None
            cd.B, cd.H, cd.W, cd.Cin, cd.ldx, cd.Ho, cd.Wo, cd.Cout = B, H, W, 64, ldx0, H, W, 256
            cd.kh, cd.kw, cd.stride, cd.pad, cd.Kpad = 1, 1, 1, 0, pd.Kpad
            cd.nseg, cd.tile = 1, _shipped_shortcut_tile()
            cd.seg[0] = L.ConvSeg(0, 256, L.ACT_NONE, 256, H * W * 256, r.data_ptr())
            cd.x_amax, cd.y_amax = amax.data_ptr() + 12288, amax.data_ptr() + 16384
            cd.w_h2, cd.scale_h2, cd.winv_h2 = pld.data_ptr(), scd.data_ptr(), winvd.data_ptr()
            L.check(lib.ymi_conv2d_nhwc_f32(C.byref(cd), s), 'shortcut')
        else:
            r = ((x0 * s0) @ wd.t() + bd).contiguous().to(DEV)
        keep.append(r)
        d.res, d.res_ld = r.data_ptr(), 256
        if zero_new:
            d.x0, d.x0_amax, d.w_d_h2, d.scale_d_h2, d.bias_d, d.ldx0, d.cout_pad_d = None, None, None, None, None, 0, 0
    L.check(lib.ymi_pointwise_chain_f32(C.byref(d), s), 'chain')
    torch.cuda.synchronize()
    am = amax.view(5, 1024).amax(1).cpu().tolist()
    ok = bool((y[M:] == SENTINEL).all())
    zc = None
    if z is not None:
        if in_place is None:
            ok = ok and bool((z[M:] == SENTINEL).all())
        zc = z[:M, :64].cpu()
        if in_place == 'x0' and ldx0 > 64:
            ok = ok and bool(torch.isnan(z[:, 64:]).all())          # the padding channels of the in-place rows stay what they were
    return y[:M].cpu(), zc, am[1], am[2], ok


def _rel(a, ref):
    return ((a.double() - ref).abs().max() / ref.abs().max()).item()


def _check(B, H, W, act, got, st=1.0, s0=1.0, two=None, tag=''):
    """The fp64 bars; `two`: the two-launch form's outputs on the same inputs (the reference of the factor-2 bar)."""
    y, z, ya, za, ok = got
    yr, zr = _fp64(B, H, W, act, st, s0)
    ey = _rel(y, yr)
    line = 'entry chain %dx%dx%d%s: y %.3e of max' % (B, H, W, tag, ey)
    if two is not None:
        e2 = _rel(two[0], yr)
        line += ' (two launches %.3e)' % e2
    if z is not None:
        line += ', z %.3e' % _rel(z, zr)
    print(line)
    assert ok, 'rows beyond M were written'
    assert ey < 1e-6
    assert abs(ya - yr.abs().max().item()) <= 1e-6 * yr.abs().max().item()
    if z is not None:
        assert _rel(z, zr) < 1e-6
        assert abs(za - zr.abs().max().item()) <= 2e-6 * zr.abs().max().item()
    if two is not None:
        assert ey <= 2 * e2, (ey, e2)


@pytest.mark.parametrize('act', [L.ACT_RELU, L.ACT_LEAKY01], ids=['relu', 'leaky'])
@pytest.mark.parametrize('B,H,W', SHAPES, ids=['%dx%dx%d' % s for s in SHAPES])
def test_entry_chain_kernel(B, H, W, act):
    """Every shape, both activations, with z: fp64 bars, the factor-2 bar against the two-launch form, two runs bit-equal, sentinel
    rows; and the same launch without z writes the same y."""
    got = _launch(B, H, W, act, 'entry')
    two = _launch(B, H, W, act, 'two')
    _check(B, H, W, act, got, two=two)
    again = _launch(B, H, W, act, 'entry')
    assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1]) and got[2:4] == again[2:4]
    y1, z1, ya1, _, ok1 = _launch(B, H, W, act, 'entry', with_z=False)
    assert z1 is None and ok1 and torch.equal(y1, got[0]) and ya1 == got[2]


@pytest.mark.parametrize('B,H,W', SHAPES[1:], ids=['%dx%dx%d' % s for s in SHAPES[1:]])
@pytest.mark.parametrize('variant', ['ldx0_80', 'z_over_x', 'z_over_x0', 'z_over_x0_ldx0_80'])
def test_entry_chain_pitch_and_in_place(B, H, W, variant):
    """A wider row pitch of x0 (the padding channels hold NaN) and z written in place over x — as the plan produces it — or over x0:
    bit-equal to the plain arrangement of the same inputs."""
    base = _launch(B, H, W, L.ACT_RELU, 'entry')
    kw = {'ldx0_80': dict(ldx0=80), 'z_over_x': dict(in_place='x'), 'z_over_x0': dict(in_place='x0'),
          'z_over_x0_ldx0_80': dict(in_place='x0', ldx0=80)}[variant]
    got = _launch(B, H, W, L.ACT_RELU, 'entry', **kw)
    _check(B, H, W, L.ACT_RELU, got, tag=' ' + variant)
    assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]) and got[2:4] == base[2:4]


@pytest.mark.parametrize('st,s0', [(1.0, 4096.0), (4096.0, 1.0)], ids=['x0_times_4096', 't_times_4096'])
def test_entry_chain_scales_its_two_inputs_independently(st, s0):
    """x0 2^12 larger than t, and t 2^12 larger than x0: each input is split into fp16 planes with the power-of-two scale of ITS OWN
    bound (a shared scale would overflow fp16 on one side or drop the other's low plane)."""
    B, H, W = SHAPES[2]
    got = _launch(B, H, W, L.ACT_RELU, 'entry', st=st, s0=s0)
    two = _launch(B, H, W, L.ACT_RELU, 'two', st=st, s0=s0)
    _check(B, H, W, L.ACT_RELU, got, st, s0, two=two, tag=' t x %g, x0 x %g' % (st, s0))


@pytest.mark.parametrize('B,H,W', SHAPES, ids=['%dx%dx%d' % s for s in SHAPES])
def test_zeroed_new_fields_are_the_launch_without_them(B, H, W):
    """A descriptor whose new fields are written as zero gives the bits of gpu_utils.run_chain, which has never heard of them."""
    from gpu_utils import run_chain
    t, x0, wa, ba, wd, bd, wb, bb = _inputs(B, H, W)
    y, z, ya, za, ok = _launch(B, H, W, L.ACT_RELU, 'plain', zero_new=True)
    y0, z0 = run_chain(t, wa, ba, (x0 @ wd.t() + bd).contiguous(), wb, bb)
    assert ok and torch.equal(y, y0) and torch.equal(z, z0)
    assert [ya, za] == run_chain.last_amax


def _build(config='yolact_resnet50_config', seed=0, gain=0.04):
    import yolact_amd
    yolact_amd.set_cfg(config)
    from yolact_amd.yolact import Yolact
    net = Yolact()
    net.load_state_dict_compat(synth_state_dict([(k, tuple(v.shape)) for k, v in net.state_dict().items()], seed=seed, conf_gain=gain))
    net.detect.use_fast_nms = True
    return net.to(DEV)


def test_forced_plan_installs_the_entry_form_and_matches_the_plan_without_it(monkeypatch):
    """B = 2 at 550 x 550 with YOLACT_AMD_CHAIN_ENTRY=force: the first pair's descriptor carries x0, the shortcut's op is a nop, its
    conv_meta entry sits right behind conv3's, the head tensors agree with YOLACT_AMD_CHAIN_ENTRY=0 within 2e-5 of max (the bar of
    the chain-versus-two-launches test), and the same plan through BatchPipeline (four slots) gives the single-plan path's records."""
    from yolact_amd import parallel
    from yolact_amd.pipeline import BatchPipeline
    x = synth_images(2, 550, 550, seed=4321).to(DEV)
    monkeypatch.setenv('YOLACT_AMD_CHAIN_ENTRY', 'force')
    net = _build()
    plan = net.plan_for(x)
    lib = plan.lib
    chains = {op[2]: op[1].contents for op in plan.ops if op[0] is lib.ymi_pointwise_chain_f32}
    assert 'layer0.0.conv3+layer0.1.conv1' in chains
    cd = chains['layer0.0.conv3+layer0.1.conv1']
    assert cd.x0 and not cd.res and cd.w_d_h2 and cd.x0_amax and cd.ldx0 >= 64
    assert all(not c.x0 for n, c in chains.items() if n != 'layer0.0.conv3+layer0.1.conv1')
    assert [op[0] for op in plan.ops if op[2] == 'layer0.0.down[fused into layer0.0.conv3]'] == ['nop']
    # (the side stream's record / wait markers of that name stay; the launch is gone)
    assert all(isinstance(op[0], str) for op in plan.ops if op[2] == 'layer0.0.down')
    names = [n for n, _ in plan.conv_meta]
    assert names.index('layer0.0.down') == names.index('layer0.0.conv3') + 1          # profile records map onto conv_meta by position
    with torch.no_grad():
        a = {k: v.clone() for k, v in net.forward_raw(x).items() if k in ('loc', 'conf_logits', 'mask', 'proto')}
        ref = parallel.pack_records(net.forward_device(x)).clone()
        torch.cuda.synchronize()
        pipe = BatchPipeline(net, 4)
        pipe.warm(x)
        outs = [pipe.submit(x) for _ in range(5)]
        for o in outs:
            o['done'].synchronize()
            assert torch.equal(parallel.pack_records(o), ref)
        pipe.synchronize()
        for k in range(4):
            assert any(op[0] is lib.ymi_pointwise_chain_f32 and op[1].contents.x0 for op in net.plan_for(x, k).ops)
    monkeypatch.setenv('YOLACT_AMD_CHAIN_ENTRY', '0')
    net2 = _build()
    plan2 = net2.plan_for(x)
    assert not any(op[0] is lib.ymi_pointwise_chain_f32 and op[1].contents.x0 for op in plan2.ops)
    assert any(op[2] == 'layer0.0.down' and op[0] is lib.ymi_conv2d_nhwc_f32 for op in plan2.ops)
    with torch.no_grad():
        b = net2.forward_raw(x)
    for k in a:
        err = ((a[k] - b[k]).abs().max() / b[k].abs().max()).item()
        print('entry form vs shortcut launch, %s: %.2e of max' % (k, err))
        assert err < 2e-5, k


def test_batch8_default_plan_installs_the_entry_form_from_the_shipped_table():
    """configs[1] at batch 8 (what bench.py times): the shipped table's 'chain(8, 138, 138, 64)|h2' decision installs the form, and
    the plan measures nothing itself."""
    x = synth_images(8, 550, 550, seed=1234).to(DEV)
    net = _build()
    plan = net.plan_for(x)
    assert plan.tune_misses == 0
    ent = TT.load_tune_table(DEV)[TT.chain_key('chain', 8, 138, 138, 64, 'h2')]
    assert ent[0] == 1, ent
    (cd,) = [op[1].contents for op in plan.ops if op[0] is plan.lib.ymi_pointwise_chain_f32 and op[2] == 'layer0.0.conv3+layer0.1.conv1']
    assert cd.x0 and not cd.res, plan.chaine_table
    assert any(op[0] == 'nop' and op[2] == 'layer0.0.down[fused into layer0.0.conv3]' for op in plan.ops)
