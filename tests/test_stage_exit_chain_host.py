"""ymi_stage_exit_chain_f32 (csrc/chain.hip, chain_h2_k<128>: the last first-stage conv3 + the next stage's conv1 in one launch)
without a GPU: the descriptor validation, the layout of ymi_stage_exit_desc against its ctypes mirror, and the plan-level
eligibility predicate on dry CPU plans."""
import ctypes
import os
import subprocess

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _valid_desc(L, p16):
    d = L.StageExitDesc()
    c = d.chain
    c.x, c.res, c.y, c.z, c.w_a_h2, c.w_b_h2, c.scale_a_h2, c.scale_b_h2, c.x_amax = (p16,) * 9
    c.M, c.ldx, c.res_ld, c.ldy, c.ldz = 70, 64, 256, 256, 128
    c.k_a, c.n_a, c.n_b, c.cout_pad_a, c.cout_pad_b = 64, 256, 128, 256, 128
    c.act_a, c.act_b = L.ACT_RELU, L.ACT_RELU
    d.B, d.H, d.W, d.y_stride = 2, 5, 7, 2
    return d


def test_stage_exit_entry_validates_its_descriptor_before_any_launch():
    """The documented codes (-3 null, -1 argument, -2 shape), each from a descriptor that is valid but for ONE field; validation
    precedes every HIP call, so this runs without a GPU.  (A fully valid descriptor is never submitted here: it would launch.)"""
    from yolact_amd import _lib as L
    lib = L.lib()
    assert lib.ymi_stage_exit_chain_f32(None, None) == -3
    buf = (ctypes.c_float * 64)()
    p16 = (ctypes.addressof(buf) + 15) & ~15
    assert lib.ymi_stage_exit_chain_f32(ctypes.byref(L.StageExitDesc()), None) == -3       # every pointer NULL
    for name in ('x', 'y', 'z', 'w_a_h2', 'w_b_h2', 'scale_a_h2', 'scale_b_h2', 'x_amax'):   # z and its filters are REQUIRED here
        d = _valid_desc(L, p16)
        setattr(d.chain, name, None)
        assert lib.ymi_stage_exit_chain_f32(ctypes.byref(d), None) == -3, name
    for field, val in (('k_a', 128), ('n_a', 512), ('n_b', 64), ('n_b', 256), ('M', 71), ('M', 0), ('act_a', 7), ('act_b', -1)):
        d = _valid_desc(L, p16)
        setattr(d.chain, field, val)
        assert lib.ymi_stage_exit_chain_f32(ctypes.byref(d), None) == -1, (field, val)
    for field, val in (('y_stride', 0), ('y_stride', 3), ('B', 3), ('H', 0), ('W', -7)):
        d = _valid_desc(L, p16)
        setattr(d, field, val)
        assert lib.ymi_stage_exit_chain_f32(ctypes.byref(d), None) == -1, (field, val)
    for field, val in (('ldx', 60), ('ldy', 250), ('ldz', 64), ('ldz', 130), ('res_ld', 128), ('cout_pad_a', 128), ('cout_pad_b', 64),
                       ('z', p16 + 4), ('x', p16 + 8), ('w_b_h2', p16 + 2)):
        d = _valid_desc(L, p16)
        setattr(d.chain, field, val)
        assert lib.ymi_stage_exit_chain_f32(ctypes.byref(d), None) == -2, (field, val)
    d = _valid_desc(L, p16)                                # 32-bit buffer offsets: M * ldy * 4 must stay below 2^31
    d.chain.M, d.B, d.H, d.W = 1 << 21, 1 << 7, 1 << 7, 1 << 7
    assert lib.ymi_stage_exit_chain_f32(ctypes.byref(d), None) == -2
    # the row -> (h, w) decode of the kernel is exact only while M * max(H, W) < 2^32: wider / taller maps are refused, not mis-stored
    for B, H, W in ((1, 10, 100000), (1, 100000, 10), (2, 1000000, 1)):
        d = _valid_desc(L, p16)
        d.chain.M, d.B, d.H, d.W = B * H * W, B, H, W
        assert d.chain.M * d.chain.ldy < (1 << 29)          # (passes the 32-bit offset check: this limit is what refuses it)
        assert B * H * W * max(H, W) >= (1 << 32)
        assert lib.ymi_stage_exit_chain_f32(ctypes.byref(d), None) == -2, (B, H, W)
    # the pair entry accepts no more than before: the 128-wide second layer is NOT reachable through it
    c = _valid_desc(L, p16).chain
    assert lib.ymi_pointwise_chain_f32(ctypes.byref(c), None) == -1
    assert lib.ymi_abi_version() == L.ABI_VERSION == 9      # additive: no ABI bump


def test_stage_exit_desc_layout_matches_c_compiler(tmp_path):
    from yolact_amd import _lib as L
    src = tmp_path / 'sz.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu %%zu %%zu %%zu %%zu %%zu %%d\\n",'
                   'sizeof(ymi_stage_exit_desc),offsetof(ymi_stage_exit_desc,chain),offsetof(ymi_stage_exit_desc,B),'
                   'offsetof(ymi_stage_exit_desc,H),offsetof(ymi_stage_exit_desc,W),offsetof(ymi_stage_exit_desc,y_stride),'
                   '(int)YMI_OP_STAGE_EXIT);return 0;}' % os.path.join(ROOT, 'include', 'yolact_amd.h'))
    exe = tmp_path / 'sz'
    subprocess.run(['gcc', str(src), '-o', str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    D = L.StageExitDesc
    want = [ctypes.sizeof(D), D.chain.offset, D.B.offset, D.H.offset, D.W.offset, D.y_stride.offset, L.OP_STAGE_EXIT]
    assert got == want, (got, want)
    assert ctypes.sizeof(D) == ctypes.sizeof(L.ChainDesc) + 16 and D.chain.offset == 0


def _dry_plan(config, **kw):
    import yolact_amd
    from yolact_amd.engine import Plan
    yolact_amd.set_cfg(config)
    from yolact_amd.yolact import Yolact
    return Plan(Yolact(), 2, 550, 550, torch.device('cpu'), **kw)


def test_eligibility_predicate_finds_exactly_the_first_stage_exit():
    """On a dry CPU plan: ResNet-50 has ONE stage exit the launch can take — layer0.2.conv3 / layer1.0.conv1, with
    layer1.0.down as the only other (stride-2) reader — in the one-stream and in the two-stream op order (where the shortcut sits
    between the two layers); the later exits feed the FPN or have 128+ planes; DarkNet has none."""
    for kw in ({}, {'dry_two_streams': True}):
        plan = _dry_plan('yolact_resnet50_config', **kw)
        cands = plan.stage_exit_candidates()
        names = [(plan.ops[a][2], plan.ops[b][2], [plan.ops[j][2] for j in downs]) for a, b, downs in cands]
        assert names == [('layer0.2.conv3', 'layer1.0.conv1', ['layer1.0.down'])], names
        # the arena keeps conv3's input and the residual alive until conv1's output exists: z overlaps none of its operands
        (a, b, _), = cands
        d3, d1 = plan.ops[a][1].contents, plan.ops[b][1].contents
        M = d3.B * d3.Ho * d3.Wo
        z = (d1.seg[0].ptr, d1.seg[0].ptr + 4 * M * d1.seg[0].row_stride)
        for ptr, ld in ((d3.x, d3.ldx), (d3.res, d3.res_ld), (d3.seg[0].ptr, d3.seg[0].row_stride)):
            assert not (z[0] < ptr + 4 * M * ld and ptr < z[1])
    assert _dry_plan('yolact_darknet53_config').stage_exit_candidates() == []
