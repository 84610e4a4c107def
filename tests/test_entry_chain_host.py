"""The ENTRY form of ymi_pointwise_chain_f32 (csrc/chain.hip, chain_h2_k<64, true>: layer0.0's projection shortcut computed inside the
layer0.0.conv3 + layer0.1.conv1 launch) without a GPU: the descriptor validation, both descriptor layouts against the C compiler,
the plan-level eligibility predicate on dry CPU plans and the table key of the decision."""
import ctypes
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _valid_desc(L, p16):
    d = L.ChainDesc()
    d.x, d.y, d.z, d.w_a_h2, d.w_b_h2, d.scale_a_h2, d.scale_b_h2, d.x_amax = (p16,) * 8
    d.x0, d.x0_amax, d.w_d_h2, d.scale_d_h2, d.bias_d = (p16,) * 5
    d.M, d.ldx, d.ldy, d.ldz, d.ldx0 = 70, 64, 256, 64, 64
    d.k_a, d.n_a, d.n_b, d.cout_pad_a, d.cout_pad_b, d.cout_pad_d = 64, 256, 64, 256, 128, 256
    d.act_a, d.act_b = L.ACT_RELU, L.ACT_RELU
    return d


def test_entry_form_validates_its_descriptor_before_any_launch():
    """The documented codes (-3 null, -1 argument, -2 shape), each from a descriptor that is valid but for ONE field; validation
    precedes every HIP call, so this runs without a GPU.  (A fully valid descriptor is never submitted here: it would launch.)"""
    from yolact_amd import _lib as L
    lib = L.lib()
    buf = (ctypes.c_float * 64)()
    p16 = (ctypes.addressof(buf) + 15) & ~15
    for name in ('w_d_h2', 'scale_d_h2', 'x0_amax'):
        d = _valid_desc(L, p16)
        setattr(d, name, None)
        assert lib.ymi_pointwise_chain_f32(ctypes.byref(d), None) == -3, name
    d = _valid_desc(L, p16)                                # a residual next to x0: the launch computes it OR reads it
    d.res, d.res_ld = p16, 256
    assert lib.ymi_pointwise_chain_f32(ctypes.byref(d), None) == -1
    for field, val in (('k_a', 32), ('n_a', 128), ('n_b', 128), ('M', 0), ('act_a', 9)):
        d = _valid_desc(L, p16)
        setattr(d, field, val)
        assert lib.ymi_pointwise_chain_f32(ctypes.byref(d), None) == -1, (field, val)
    for field, val in (('ldx0', 60), ('ldx0', 66), ('x0', p16 + 4), ('w_d_h2', p16 + 8), ('cout_pad_d', 128), ('ldx0', (1 << 29) // 70 + 4)):
        d = _valid_desc(L, p16)
        setattr(d, field, val)
        assert lib.ymi_pointwise_chain_f32(ctypes.byref(d), None) == -2, (field, val)
    # the 128 / 256-plane path and the stage exit have no entry form
    for P in (128, 256):
        d = _valid_desc(L, p16)
        d.k_a, d.n_a, d.n_b, d.ldx, d.ldy, d.ldz = P, 4 * P, P, P, 4 * P, P
        assert lib.ymi_pointwise_chain_f32(ctypes.byref(d), None) == -1, P
    e = L.StageExitDesc()
    e.chain = _valid_desc(L, p16)
    e.chain.n_b, e.chain.ldz = 128, 128
    e.B, e.H, e.W, e.y_stride = 2, 5, 7, 2
    assert lib.ymi_stage_exit_chain_f32(ctypes.byref(e), None) == -1
    e.chain.x0 = None                                      # (... and that was the only thing wrong with it: now the residual is missing nothing)
    e.chain.res, e.chain.res_ld, e.chain.M = p16, 250, 70
    assert lib.ymi_stage_exit_chain_f32(ctypes.byref(e), None) == -2
    assert lib.ymi_abi_version() == L.ABI_VERSION == 9      # additive: no ABI bump


def test_chain_desc_layouts_match_c_compiler(tmp_path):
    from yolact_amd import _lib as L
    fields = ('x0', 'x0_amax', 'w_d_h2', 'scale_d_h2', 'bias_d', 'ldx0', 'cout_pad_d', 'res_amax', 'gain_a', 'bias_max_a', 'M', 'act_a')
    src = tmp_path / 'sz.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu %%zu %%zu %s\\n",'
                   'sizeof(ymi_chain_desc),sizeof(ymi_stage_exit_desc),offsetof(ymi_stage_exit_desc,B),%s);return 0;}'
                   % (os.path.join(ROOT, 'include', 'yolact_amd.h'), ' '.join('%zu' for _ in fields),
                      ','.join('offsetof(ymi_chain_desc,%s)' % f for f in fields)))
    exe = tmp_path / 'sz'
    subprocess.run(['gcc', str(src), '-o', str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = [ctypes.sizeof(L.ChainDesc), ctypes.sizeof(L.StageExitDesc), L.StageExitDesc.B.offset] + [getattr(L.ChainDesc, f).offset for f in fields]
    assert got == want, (got, want)
    assert L.ChainDesc.x0.offset == L.ChainDesc.bias_max_a.offset + 4        # the new fields TRAIL the ABI-8 ones
    assert ctypes.sizeof(L.ChainDesc) == L.ChainDesc.cout_pad_d.offset + 4
    d = L.ChainDesc()                                                        # all zero = the launch without them
    assert not any((d.x0, d.x0_amax, d.w_d_h2, d.scale_d_h2, d.bias_d, d.ldx0, d.cout_pad_d))


def _dry_plan(config, B, size=550, **kw):
    import yolact_amd
    from yolact_amd.engine import Plan
    yolact_amd.set_cfg(config)
    from yolact_amd.yolact import Yolact
    return Plan(Yolact(), B, size, size, torch.device('cpu'), **kw)


@pytest.mark.parametrize('config,size', [('yolact_resnet50_config', 550), ('yolact_base_config', 550), ('yolact_im700_config', 700),
                                         ('yolact_plus_resnet50_config', 550)])
def test_eligibility_predicate_finds_exactly_the_first_block(config, size):
    """On dry CPU plans, batch 1 and 8, one-stream and two-stream op order: the only pair whose residual is a stride-1 64 -> 256
    projection shortcut nothing else reads is layer0.0.conv3 + layer0.1.conv1 with layer0.0.down (the later stages' shortcuts are
    stride 2 or wider; the other first-stage blocks have identity shortcuts)."""
    from yolact_amd import plan_tune as PT
    for B in (1, 8):
        for kw in ({}, {'dry_two_streams': True}):
            plan = _dry_plan(config, B, size, **kw)
            cands = plan.entry_chain_candidates()
            assert [tuple(plan.ops[i][2] for i in c) for c in cands] == [('layer0.0.down', 'layer0.0.conv3', 'layer0.1.conv1')], (B, kw)
            (idn, i3, i1), = cands
            assert i1 == i3 + 1 and idn < i3
            dd, d3, d1 = (plan.ops[i][1].contents for i in (idn, i3, i1))
            assert int(d3.res) == int(dd.seg[0].ptr) and d3.res_ld == dd.seg[0].row_stride
            # the aliasing contract on the buffers the arena really hands out: y apart from x0; z apart from it or exactly in place
            M = d3.B * d3.Ho * d3.Wo
            assert not PT._rows_overlap(M, d3.seg[0].ptr, d3.seg[0].row_stride, dd.x, dd.ldx)
            z, ldz = d1.seg[0].ptr, d1.seg[0].row_stride
            assert not PT._rows_overlap(M, z, ldz, dd.x, dd.ldx) or (int(z) == int(dd.x) and ldz == dd.ldx)
            assert plan.stage_exit_candidates() and all(c[0] != i3 for c in plan.stage_exit_candidates())


def test_darknet_has_no_entry_chain():
    for B in (1, 8):
        assert _dry_plan('yolact_darknet53_config', B).entry_chain_candidates() == []


def test_entry_chain_table_key_round_trips():
    """The decision lives under the free four-element spelling of a `chain` key (P is never written for the 64-plane pair itself)."""
    from yolact_amd import tune_table as TT
    key = TT.chain_key('chain', 8, 138, 138, 64, 'h2')
    assert key == 'chain(8, 138, 138, 64)|h2'
    assert TT.parse(key) == ('chain', (8, 138, 138, 64), 'h2')
    assert TT.format(*TT.parse(key)) == key
    kind, t, mode = TT.parse(key)
    assert TT.chain_key(kind, *t, mode) == key
    assert TT.chain_key('chain', 8, 138, 138, mode='h2') != key             # the pair's own decision keeps its three-element key
