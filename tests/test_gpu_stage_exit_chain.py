"""ymi_stage_exit_chain_f32 on the GPU (csrc/chain.hip, chain_h2_k<128>): layer0.2.conv3 + shortcut + ReLU and layer1.0.conv1
(256 -> 128) in one launch, y stored only where the stride-2 projection shortcut reads it.

Kernel level: y (kept pixels) and y_amax bit-equal to the shipped GEMM 1 (ymi_pointwise_chain_f32 with z = NULL), untouched
sentinel elsewhere, z against fp64 at the bars of test_pointwise_chain_matches_fp64, bit-reproducible.  Plan level: the launch
installs (forced at batch 2, from the shipped table at batch 8) and the network's outputs agree with the two-launch plan."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from yolact_amd import _lib as L  # noqa: E402
from yolact_amd.engine import Packed  # noqa: E402
from yolact_amd.utils.synth import synth_images, synth_state_dict  # noqa: E402

DEV = torch.device('cuda', 0)
SENTINEL = -12345.5

# (B, H, W): one ragged tile | 70 rows = three tiles, odd H and W, tiles crossing image rows and images | ~106 tiles, fewer than one
# per block on some CUs | 520 tiles > 2 x 256: several trips of the two-iteration loop plus the extra GEMM-2 iteration
SHAPES = [(1, 1, 1), (2, 5, 7), (3, 33, 34), (1, 131, 127)]


@functools.lru_cache(maxsize=None)
def _inputs(B, H, W):
    M = B * H * W
    g = torch.Generator().manual_seed(7100 + M)
    x = torch.randn(M, 64, generator=g) * 3
    wa = torch.randn(256, 64, generator=g) / 8
    ba = torch.randn(256, generator=g) * 0.3
    res = torch.randn(M, 256, generator=g) * 2
    wb = torch.randn(128, 256, generator=g) / 16
    bb = torch.randn(128, generator=g) * 0.1
    return x, wa, ba, res, wb, bb


def _act(t, act):
    return torch.relu(t) if act == L.ACT_RELU else F.leaky_relu(t, 0.1)


@functools.lru_cache(maxsize=None)
def _fp64(B, H, W, with_res, act):
    x, wa, ba, res, wb, bb = _inputs(B, H, W)
    yr = x.double() @ wa.double().t() + ba.double()
    yr = _act(yr + res.double() if with_res else yr, act)
    return yr, _act(yr @ wb.double().t() + bb.double(), act)


def _launch(B, H, W, with_res, act, y_stride=None):
    """y_stride None: ymi_pointwise_chain_f32 with z = NULL (the shipped GEMM 1); 1 / 2: ymi_stage_exit_chain_f32.
    Returns (y, z or None, y_amax, z_amax) on the CPU; y and z are pre-filled with SENTINEL."""
    x, wa, ba, res, wb, bb = _inputs(B, H, W)
    M = B * H * W
    pa, pb = Packed(wa.view(256, 64, 1, 1), ba, None, 1, 0, None, DEV), Packed(wb.view(128, 256, 1, 1), bb, None, 1, 0, None, DEV)
    pla, sca, _ = pa.h2()
    plb, scb, _ = pb.h2()
    xd, rd = x.to(DEV), res.to(DEV)
    y = torch.full((M, 256), SENTINEL, device=DEV)
    z = torch.full((M, 128), SENTINEL, device=DEV)
    amax = torch.zeros(3 * 1024, device=DEV)
    lib, s = L.lib(), L.stream_ptr()
    L.check(lib.ymi_amax_f32(xd.data_ptr(), xd.numel(), amax.data_ptr(), s), 'amax')
    e = L.StageExitDesc()
    d = e.chain
    d.x, d.y, d.M, d.ldx, d.ldy = xd.data_ptr(), y.data_ptr(), M, 64, 256
    d.w_a_h2, d.scale_a_h2, d.bias_a, d.cout_pad_a = pla.data_ptr(), sca.data_ptr(), pa.bias.data_ptr(), pa.CoutPad
    d.k_a, d.n_a, d.n_b, d.act_a, d.act_b = 64, 256, 64, act, act
    d.x_amax, d.y_amax = amax.data_ptr(), amax.data_ptr() + 4096
    if with_res:
        d.res, d.res_ld = rd.data_ptr(), 256
    if y_stride is None:
        L.check(lib.ymi_pointwise_chain_f32(C.byref(d), s), 'chain')
    else:
        d.n_b, d.z, d.ldz, d.z_amax = 128, z.data_ptr(), 128, amax.data_ptr() + 8192
        d.w_b_h2, d.scale_b_h2, d.bias_b, d.cout_pad_b = plb.data_ptr(), scb.data_ptr(), pb.bias.data_ptr(), pb.CoutPad
        e.B, e.H, e.W, e.y_stride = B, H, W, y_stride
        L.check(lib.ymi_stage_exit_chain_f32(C.byref(e), s), 'stage exit')
    torch.cuda.synchronize()
    am = amax.view(3, 1024).amax(1).cpu().tolist()
    return y.cpu(), (z.cpu() if y_stride is not None else None), am[1], am[2]


@functools.lru_cache(maxsize=None)
def _shipped_gemm1(B, H, W, with_res, act):
    y, _, ya, _ = _launch(B, H, W, with_res, act, None)
    return y, ya


@pytest.mark.parametrize('act', [L.ACT_RELU, L.ACT_LEAKY01], ids=['relu', 'leaky'])
@pytest.mark.parametrize('with_res', [True, False], ids=['res', 'nores'])
@pytest.mark.parametrize('y_stride', [1, 2])
@pytest.mark.parametrize('B,H,W', SHAPES, ids=['%dx%dx%d' % s for s in SHAPES])
def test_stage_exit_chain_kernel(B, H, W, y_stride, with_res, act):
    M = B * H * W
    y0, ya0 = _shipped_gemm1(B, H, W, with_res, act)
    assert not (y0 == SENTINEL).any()
    y, z, ya, za = _launch(B, H, W, with_res, act, y_stride)
    m = torch.arange(M)
    keep = ((m // W) % H % y_stride == 0) & (m % W % y_stride == 0)
    assert keep.sum().item() == B * ((H + y_stride - 1) // y_stride) * ((W + y_stride - 1) // y_stride)
    assert torch.equal(y[keep], y0[keep])                       # the shipped GEMM 1, bit for bit, where y is kept
    assert (y[~keep] == SENTINEL).all()                         # ... and not written at all elsewhere
    assert ya == ya0                                            # the bound covers EVERY pixel, kept or not
    yr, zr = _fp64(B, H, W, with_res, act)
    ez = ((z.double() - zr).abs().max() / zr.abs().max()).item()
    ea = abs(za - zr.abs().max().item()) / zr.abs().max().item()
    print('stage exit %s stride %d: z error %.2e of max, z_amax off by %.2e' % ((B, H, W), y_stride, ez, ea))
    assert ez < 1e-6
    assert ea <= 2e-6
    y2, z2, ya2, za2 = _launch(B, H, W, with_res, act, y_stride)
    assert torch.equal(y, y2) and torch.equal(z, z2) and (ya2, za2) == (ya, za)


def _build(config='yolact_resnet50_config', seed=0, gain=0.04):
    import yolact_amd
    yolact_amd.set_cfg(config)
    from yolact_amd.yolact import Yolact
    net = Yolact()
    net.load_state_dict_compat(synth_state_dict([(k, tuple(v.shape)) for k, v in net.state_dict().items()], seed=seed, conf_gain=gain))
    net.detect.use_fast_nms = True
    return net.to(DEV)


def test_forced_plan_installs_the_launch_and_matches_the_two_launch_plan(monkeypatch):
    """B = 2 at 550 x 550 with YOLACT_AMD_CHAIN_EXIT=force: exactly one op on the new entry, the pair entry keeps its two pairs, the
    head tensors agree with YOLACT_AMD_CHAIN_EXIT=0 within 2e-5 of max (the bar of the chain-versus-two-launches test), and the same
    plan through BatchPipeline (four slots, un-forked) gives the single-plan path's records."""
    from yolact_amd import parallel
    from yolact_amd.pipeline import BatchPipeline
    x = synth_images(2, 550, 550, seed=4321).to(DEV)
    monkeypatch.setenv('YOLACT_AMD_CHAIN_EXIT', 'force')
    net = _build()
    plan = net.plan_for(x)
    lib = plan.lib
    assert [op[2] for op in plan.ops if op[0] is lib.ymi_stage_exit_chain_f32] == ['layer0.2.conv3+layer1.0.conv1']
    assert [op[2] for op in plan.ops if op[0] is lib.ymi_pointwise_chain_f32] == ['layer0.0.conv3+layer0.1.conv1', 'layer0.1.conv3+layer0.2.conv1']
    (xop,) = [op for op in plan.ops if op[0] is lib.ymi_stage_exit_chain_f32]
    assert xop[1].contents.y_stride == 2
    names = [n for n, _ in plan.conv_meta]
    assert names.index('layer1.0.conv1') == names.index('layer0.2.conv3') + 1          # profile records map onto conv_meta by position
    with torch.no_grad():
        a = {k: v.clone() for k, v in net.forward_raw(x).items() if k in ('loc', 'conf_logits', 'mask', 'proto')}
        ref = parallel.pack_records(net.forward_device(x)).clone()
        torch.cuda.synchronize()
        pipe = BatchPipeline(net, 4)
        assert pipe.fork is False
        pipe.warm(x)
        outs = [pipe.submit(x) for _ in range(5)]
        for o in outs:
            o['done'].synchronize()
            assert torch.equal(parallel.pack_records(o), ref)
        pipe.synchronize()
        for k in range(4):
            assert any(op[0] is lib.ymi_stage_exit_chain_f32 for op in net.plan_for(x, k).ops)
    monkeypatch.setenv('YOLACT_AMD_CHAIN_EXIT', '0')
    net2 = _build()
    plan2 = net2.plan_for(x)
    assert not any(op[0] is lib.ymi_stage_exit_chain_f32 for op in plan2.ops)
    with torch.no_grad():
        b = net2.forward_raw(x)
    for k in a:
        err = ((a[k] - b[k]).abs().max() / b[k].abs().max()).item()
        print('stage exit vs two launches, %s: %.2e of max' % (k, err))
        assert err < 2e-5, k


def test_batch8_default_plan_installs_the_launch_from_the_shipped_table():
    """configs[1] at batch 8 (what bench.py times): the shipped table's 'chainx(8, 138, 138)|h2' decision installs the launch, and
    the plan measures nothing itself."""
    x = synth_images(8, 550, 550, seed=1234).to(DEV)
    net = _build()
    plan = net.plan_for(x)
    assert plan.tune_misses == 0
    assert [op[2] for op in plan.ops if op[0] is plan.lib.ymi_stage_exit_chain_f32] == ['layer0.2.conv3+layer1.0.conv1'], plan.chainx_table
    assert not any(op[2] == 'layer0.2.conv3' for op in plan.ops if op[0] is plan.lib.ymi_pointwise_chain_f32)
