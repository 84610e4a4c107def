"""The chunk plan of the weight-gradient kernels (csrc/grad_common.h ymi_chunk_plan, ymi_wgrad_nt), seen through the workspace sizes that
ymi_workspace_bytes answers on the host: the rule is written out again here in Python and the library has to agree on every shape.

    mb = ceil(P / 32)    sp = clamp(ceil(T / other_blocks), 1, mb)    per = ceil(mb / sp) * 32    nchunks = ceil(P / per)

ymi_conv_wgrad_nhwc_f32: P = B Ho Wo positions of g, T = 1024, other_blocks = kh kw (Cin / 32) * gz with nt = 1, 2, 4 column tiles per
wave for up to 4, 8, more 32-channel tiles of Cout and gz = ceil(Cout / (128 nt)); part(nchunks K Cout) + part(nchunks Cout) bytes.
ymi_stem_wgrad_nhwc_f32: P = B ceil(H / 2) ceil(W / 2), T = 512, other_blocks = ceil(Cout / 64); part(nchunks 147 Cout) bytes.
part(n) = ceil(4 n / 16) * 16.
"""
import ctypes as C

import pytest

from yolact_amd import _lib as L

ENULL, EARG, ESHAPE = -3, -1, -2


def ceil_div(a, b):
    return -(-a // b)


def part(n):
    return ceil_div(4 * n, 16) * 16


def chunk_plan(P, target_blocks, other_blocks):
    mb = ceil_div(P, 32)
    sp = min(max(ceil_div(target_blocks, other_blocks), 1), mb)
    per = ceil_div(mb, sp) * 32
    return per, ceil_div(P, per), sp, mb


def wgrad_nt(Cout):
    tiles = ceil_div(Cout, 32)
    nt = 1 if tiles <= 4 else (2 if tiles <= 8 else 4)
    return nt, ceil_div(Cout, nt * 128)


def conv_positions(B, H, W, k, stride):
    out = lambda n: (n + 2 * (k // 2) - k) // 2 + 1 if stride == 2 else n
    return B * out(H) * out(W)


# (B, H, W, Cin, Cout, k, stride): what the case is there for
CONV_SHAPES = [
    (1, 3, 5, 32, 32, 3, 1),          # P = 15 < 32: one chunk, sp clamped to mb = 1
    (1, 5, 13, 32, 33, 3, 1),         # P = 65 = 32 * 2 + 1: sp clamped to mb = 3, a last chunk of one position
    (3, 5, 1, 32, 32, 3, 1),          # a map one pixel wide
    (2, 9, 7, 64, 129, 1, 1),         # 1x1, nt = 2
    (2, 9, 7, 64, 257, 3, 1),         # nt = 4
    (2, 9, 7, 64, 257, 3, 2),         # stride 2 on odd H and W: 2 * 5 * 4 positions
    (2, 9, 7, 64, 129, 1, 2),         # 1x1 / stride 2 on odd H and W
    (8, 69, 69, 256, 256, 3, 1),      # 38 088 positions, sp = 15 inside (1, mb): chunks of 2 560, the last not full
    (2, 40, 40, 3648, 32, 3, 1),      # 1 026 blocks without the positions: sp = 1, one chunk of all 3 200 positions
    (1, 1, 33, 32, 33, 1, 1),         # 1x1, P = 33, other_blocks = 1: sp clamped to mb = 2
]
# (B, H, W, Cout)
STEM_SHAPES = [(1, 7, 7, 32), (2, 7, 7, 64), (1, 550, 550, 64), (8, 550, 550, 64), (8, 550, 550, 96), (1, 9, 9, 32), (3, 1, 129, 32)]


def conv_desc(B, H, W, Cin, Cout, k, stride):
    d = L.ConvWgradDesc()
    d.B, d.H, d.W, d.Cin, d.Cout, d.ldg, d.kh, d.kw, d.pad, d.stride = B, H, W, Cin, Cout, Cout, k, k, k // 2, stride
    return d


def stem_desc(B, H, W, Cout):
    d = L.StemWgradDesc()
    d.B, d.H, d.W, d.Cout, d.ldg = B, H, W, Cout, Cout
    return d


@pytest.mark.parametrize('shape', CONV_SHAPES, ids=lambda s: 'b%d_%dx%d_%dto%d_k%d_s%d' % s)
def test_conv_wgrad_workspace_follows_the_chunk_plan(shape):
    B, H, W, Cin, Cout, k, stride = shape
    nt, gz = wgrad_nt(Cout)
    K = k * k * Cin
    per, nchunks, sp, mb = chunk_plan(conv_positions(B, H, W, k, stride), 1024, k * k * (Cin // 32) * gz)
    print('P %d nt %d gz %d mb %d sp %d per %d nchunks %d' % (conv_positions(B, H, W, k, stride), nt, gz, mb, sp, per, nchunks))
    assert L.lib().ymi_workspace_bytes(L.WS_CONV_WGRAD, C.byref(conv_desc(*shape))) == part(nchunks * K * Cout) + part(nchunks * Cout)


@pytest.mark.parametrize('shape', STEM_SHAPES, ids=lambda s: 'b%d_%dx%d_to%d' % s)
def test_stem_wgrad_workspace_follows_the_chunk_plan(shape):
    B, H, W, Cout = shape
    P = B * ceil_div(H, 2) * ceil_div(W, 2)
    per, nchunks, sp, mb = chunk_plan(P, 512, ceil_div(Cout, 64))
    print('P %d mb %d sp %d per %d nchunks %d' % (P, mb, sp, per, nchunks))
    assert L.lib().ymi_workspace_bytes(L.WS_STEM_WGRAD, C.byref(stem_desc(*shape))) == part(nchunks * 147 * Cout)


def test_the_shape_lists_hit_the_edges_of_the_plan():
    plans = [(s, wgrad_nt(s[4]), chunk_plan(conv_positions(*s[:3], s[5], s[6]), 1024, s[5] * s[5] * (s[3] // 32) * wgrad_nt(s[4])[1]))
             for s in CONV_SHAPES]
    P = lambda s: conv_positions(*s[:3], s[5], s[6])
    assert {(s[4], nt) for s, (nt, gz), _ in plans} >= {(32, 1), (33, 1), (129, 2), (257, 4)}
    assert all(gz == 1 for _, (nt, gz), _ in plans)
    assert any(P(s) < 32 for s, _, _ in plans) and any(P(s) > 32 and P(s) % 32 == 1 for s, _, _ in plans)
    assert any(sp == 1 and mb > 1 for _, _, (per, n, sp, mb) in plans)                  # sp at its lower end: one chunk of everything
    assert any(sp == mb and mb > 1 for _, _, (per, n, sp, mb) in plans)                 # sp clamped to mb: chunks of 32
    assert any(1 < sp < mb and n > 1 and P(s) % per for s, _, (per, n, sp, mb) in plans)    # in between, the last chunk not full
    assert {s[5] for s in CONV_SHAPES} == {1, 3}
    assert any(s[6] == 2 and s[1] % 2 and s[2] % 2 for s in CONV_SHAPES) and any(s[2] == 1 for s in CONV_SHAPES)
    assert {(1, 7, 7, 32), (8, 550, 550, 64)} <= set(STEM_SHAPES)


def test_documented_error_codes():
    lib = L.lib()
    assert lib.ymi_workspace_bytes(L.WS_CONV_WGRAD, None) == ENULL
    assert lib.ymi_workspace_bytes(L.WS_STEM_WGRAD, None) == ENULL
    for Cin in (48, 31, 1):
        assert lib.ymi_workspace_bytes(L.WS_CONV_WGRAD, C.byref(conv_desc(2, 9, 7, Cin, 32, 3, 1))) == ESHAPE, Cin
    assert lib.ymi_workspace_bytes(L.WS_CONV_WGRAD, C.byref(conv_desc(2, 9, 7, 0, 32, 3, 1))) == EARG
