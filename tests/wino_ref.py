"""Independent fp64 reference of the Winograd convolution path (csrc/winograd.hip, csrc/wgemm.hip, the grouped GEMM of
csrc/conv_igemm.hip), built from torch alone: no engine code, no oracle.

  conv3x3_ref       F.conv2d in float64 (3x3, stride 1, pad 1), the BatchNorm folded in fp64 from its own parameters, then
                    ReLU / LeakyReLU(0.1) / tanh / sigmoid
  band_ref          the same on sets of output rows: the input rows come from the real neighbouring rows, zero padding only at
                    the true image edges (so the large shipped shapes stay cheap on the CPU)
  upsample2x_ref    2x bilinear, align_corners=False, optional ReLU (protonet's interpolate + ReLU)
  proj_ref          conv -> act -> 1x1 -> act2 (the fused last projection of protonet)
  head_scatter_ref  the segmented prediction-head output written into level-concatenated [B, P, k] tensors at a prior offset
  BT / G / AT       the Lavin & Gray matrices for F(2x2,3x3) and F(4x4,3x3); winograd_ref restates the algorithm in fp64, or,
                    with fp32=True, emulates it with every stage rounded to fp32 (the error the algorithm itself adds)
  max_gain_input    an input whose V component (i, j) reaches exactly gain * A on every interior tile (gain 4 / 100): the worst
                    case of the |B^T d B| <= gain max|d| bound the fp16x2 V planes are scaled by
  h2_scale / split_h2  the power-of-two scale rule of ymi_h2_scale (csrc/common.h) and the two-piece fp16 split
"""
import numpy as np
import torch
import torch.nn.functional as F

ACT_NONE, ACT_RELU, ACT_LEAKY01, ACT_TANH, ACT_SIGMOID = 0, 1, 2, 3, 4

_D = torch.float64
BT = {2: torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=_D),
      4: torch.tensor([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0],
                       [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]], dtype=_D)}
G = {2: torch.tensor([[1, 0, 0], [1 / 2, 1 / 2, 1 / 2], [1 / 2, -1 / 2, 1 / 2], [0, 0, 1]], dtype=_D),
     4: torch.tensor([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6],
                      [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]], dtype=_D)}
AT = {2: torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=_D),
      4: torch.tensor([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], dtype=_D)}
GAIN = {m: float(BT[m].abs().sum(1).max() ** 2) for m in (2, 4)}          # max over (i, j) of |B^T|_i,1 |B^T|_j,1: 4 and 100


def act_ref(y, act):
    if act == ACT_RELU:
        return torch.relu(y)
    if act == ACT_LEAKY01:
        return torch.where(y > 0, y, 0.1 * y)
    if act == ACT_TANH:
        return torch.tanh(y)
    if act == ACT_SIGMOID:
        return torch.sigmoid(y)
    assert act == ACT_NONE, act
    return y


def epilogue(bias, bn, cout):
    """(scale, shift) in fp64 of conv + bias followed by an eval-mode BatchNorm: y = conv * scale + shift."""
    b = torch.zeros(cout, dtype=_D) if bias is None else bias.detach().double().cpu()
    if bn is None:
        return torch.ones(cout, dtype=_D), b
    sc = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    return sc, (b - bn.running_mean.detach().double()) * sc + bn.bias.detach().double()


def _finish(y, bias, bn, act):
    sc, sh = epilogue(bias, bn, y.shape[1])
    return act_ref(y * sc.to(y.device).view(1, -1, 1, 1) + sh.to(y.device).view(1, -1, 1, 1), act)


def conv3x3_ref(x, w, bias=None, bn=None, act=ACT_NONE):
    """x [B,C,H,W], w [Cout,C,3,3] -> act(BN(conv(x, w) + bias)) [B,Cout,H,W] in fp64."""
    return _finish(F.conv2d(x.double(), w.double(), None, 1, 1), bias, bn, act)


def band_ref(x, w, bias, bn, act, bands):
    """conv3x3_ref restricted to output rows: bands = [(r0, r1), ...] half-open row ranges.  Returns one [B,Cout,r1-r0,W]
    tensor per band; band k equals conv3x3_ref(x, ...)[:, :, r0:r1] (tests/test_winograd_kat_host.py)."""
    H = x.shape[2]
    out = []
    for r0, r1 in bands:
        assert 0 <= r0 < r1 <= H, (r0, r1, H)
        xs = x[:, :, max(r0 - 1, 0):min(r1 + 1, H)].double()
        xs = F.pad(xs, (0, 0, 1 if r0 == 0 else 0, 1 if r1 == H else 0))      # zero rows only at the true image edges
        out.append(_finish(F.conv2d(xs, w.double(), None, 1, (0, 1)), bias, bn, act))
    return out


def upsample2x_ref(lo, relu=False):
    """2x bilinear (align_corners=False) of [B,C,h,w] in fp64, then ReLU if `relu` (protonet: F.interpolate + ReLU)."""
    up = F.interpolate(lo.double(), size=(2 * lo.shape[2], 2 * lo.shape[3]), mode='bilinear', align_corners=False)
    return torch.relu(up) if relu else up


def proj_ref(y3, pw, pb=None, act2=ACT_NONE):
    """The 1x1 that consumes a 3x3's activated output: act2(conv1x1(y3, pw) + pb), fp64."""
    return act_ref(F.conv2d(y3.double(), pw.double(), None if pb is None else pb.double()), act2)


def head_scatter_ref(y, segs, P, off):
    """The segmented output of a prediction-head conv.  y [B,Cout,H,W] (conv + bias, before any activation), segs = [(n0, n1,
    act), ...].  A segment's row is one pixel (its A priors side by side), so the level-concatenated [B, P*A, k] tensor is
    [B, P, n1 - n0] here: returns one such buffer per segment with the level at rows [off, off + H*W) (off = the level's prior
    offset / A) and NaN in every other row."""
    B, _, H, W = y.shape
    out = []
    for n0, n1, act in segs:
        buf = torch.full((B, P, n1 - n0), float('nan'), dtype=_D)
        buf[:, off:off + H * W] = act_ref(y[:, n0:n1].double(), act).permute(0, 2, 3, 1).reshape(B, H * W, n1 - n0)
        out.append(buf)
    return out


# ---- the algorithm itself --------------------------------------------------------------------------------------------------------
def _tiles(x, m):
    B, C, H, W = x.shape
    a = m + 2
    th, tw = -(-H // m), -(-W // m)
    xp = F.pad(x, (1, tw * m + 1 - W, 1, th * m + 1 - H))
    return xp.unfold(2, a, m).unfold(3, a, m), th, tw                   # [B,C,th,tw,a,a]


def input_transform(x, m):
    """V [a*a, B, th, tw, C] = B^T d B of every tile (fp64)."""
    d, th, tw = _tiles(x.double(), m)
    a = m + 2
    return torch.einsum('ij,bcyxjk,lk->ilbyxc', BT[m], d, BT[m]).reshape(a * a, *d.shape[:1], th, tw, d.shape[1])


def winograd_ref(x, w, m, fp32=False, swap=None):
    """3x3 / stride 1 / pad 1 convolution as Winograd F(m x m, 3 x 3): U = G g G^T, V = B^T d B, M = sum_c V U, Y = A^T M A.
    fp32=True rounds the input, U, V, every M and Y to fp32 (the algorithm's own rounding, no GEMM-order effects).
    swap = e: component e of M is replaced by component e + 1 (a wrong-variant model)."""
    B, C, H, W = x.shape
    a = m + 2
    r = (lambda t: t.float().double()) if fp32 else (lambda t: t)
    U = r(torch.einsum('ai,ncij,bj->abnc', G[m], w.double(), G[m]).reshape(a * a, -1, C))
    V = r(input_transform(r(x.double()), m))                               # [a*a, B, th, tw, C]
    Mg = r(torch.einsum('ebyxc,enc->ebyxn', V, U))
    if swap is not None:
        Mg = Mg.clone()
        Mg[swap] = Mg[(swap + 1) % (a * a)]
    _, _, th, tw, N = Mg.shape
    Y = torch.einsum('ij,jkbyxn,lk->bnyixl', AT[m], Mg.reshape(a, a, B, th, tw, N), AT[m]).reshape(B, N, th * m, tw * m)
    return r(Y[:, :, :H, :W])


# ---- fp16x2 numerics of the V planes ---------------------------------------------------------------------------------------------
def h2_scale(amax):
    """ymi_h2_scale (csrc/common.h): the power of two s with amax * s in [2^13, 2^14) (1 for 0 / inf / NaN)."""
    a = np.float32(amax)
    if not np.isfinite(a) or a == 0:
        return 1.0
    _, e = np.frexp(a)                                   # a = f 2^e, 0.5 <= f < 1
    return float(2.0 ** int(np.clip(14 - e, -125, 125)))


def split_h2(v, s):
    """v (fp64 values of fp32 numbers) -> (h, l) as fp64: t = fp32(v s), h = fp16(t), l = fp16(t - h) (numpy: overflow -> inf)."""
    t = (v.numpy() * s).astype(np.float32)
    with np.errstate(over='ignore'):
        h = t.astype(np.float16)
        l = (t - h.astype(np.float32)).astype(np.float16)
    return torch.from_numpy(h.astype(np.float64)), torch.from_numpy(l.astype(np.float64))


def winograd_h2_emul(x, w, m, gain, amax=None):
    """The fp16x2 grouped GEMM of the Winograd path on the CPU: V (fp32) scaled by h2_scale(amax * gain) and split into fp16
    planes (the kernels' V planes / on-the-fly split), U split per (component, filter row) as engine.split2_planes_f16 does, the
    three kept piece products hh + hl + lh summed in fp64.  `gain` is the bound under test (shipped: 4 / 100)."""
    B, C, H, W = x.shape
    a = m + 2
    amax = float(x.abs().max()) if amax is None else amax
    x32 = x.float().double()
    U = torch.einsum('ai,ncij,bj->abnc', G[m], w.double(), G[m]).reshape(a * a, -1, C).float().double()
    su = torch.tensor([[h2_scale(float(v)) for v in row] for row in U.abs().amax(-1)], dtype=_D)       # [a*a, N]
    uh, ul = split_h2(U * su.unsqueeze(-1), 1.0)
    V = input_transform(x32, m).float().double()
    s = h2_scale(amax * gain)
    vh, vl = split_h2(V, s)
    Mg = (torch.einsum('ebyxc,enc->ebyxn', vh, uh) + torch.einsum('ebyxc,enc->ebyxn', vh, ul)
          + torch.einsum('ebyxc,enc->ebyxn', vl, uh)) / (s * su.view(a * a, 1, 1, 1, -1))
    _, _, th, tw, N = Mg.shape
    Y = torch.einsum('ij,jkbyxn,lk->bnyixl', AT[m], Mg.reshape(a, a, B, th, tw, N), AT[m]).reshape(B, N, th * m, tw * m)
    return Y[:, :, :H, :W], bool(torch.isfinite(vh).all() and torch.isfinite(vl).all())


def _phase_signs(n, m, i):
    """Signs r[y], y = 0 .. n-1, with r[m t - 1 + p] = sign(B^T[i, p]) for every tile t and every p with B^T[i, p] != 0."""
    r = {}
    for t in range(-(-n // m) + 1):
        for p in range(m + 2):
            c = float(BT[m][i, p])
            y = m * t - 1 + p
            if c != 0 and 0 <= y < n:
                sg = 1.0 if c > 0 else -1.0
                assert r.setdefault(y, sg) == sg, 'component %d of F(%d) has no tile-consistent sign pattern' % (i, m)
    return torch.tensor([r.get(y, 1.0) for y in range(n)], dtype=_D)


def max_gain_input(B, C, H, W, m, ij, A=1.0, seed=0):
    """[B,C,H,W] fp64 input with |x| = A everywhere whose V component (i, j) equals +-gain * A on every interior tile (patch
    rows m t - 1 .. m t + m and columns likewise inside the image), gain = |B^T_i|_1 |B^T_j|_1 (100 for i, j in {0, 1, 2, 5}
    of F(4x4), 4 for i, j in {1, 2} of F(2x2)).  Each (image, channel) carries its own random overall sign."""
    i, j = ij
    g = torch.Generator().manual_seed(seed)
    eps = torch.where(torch.rand(B, C, 1, 1, generator=g) < 0.5, -1.0, 1.0).double()
    return A * eps * _phase_signs(H, m, i).view(1, 1, H, 1) * _phase_signs(W, m, j).view(1, 1, 1, W)


def interior_tiles(H, W, m):
    """(ty, tx) index ranges of the tiles whose whole (m+2)^2 patch lies inside an H x W image."""
    ty = [t for t in range(-(-H // m)) if m * t - 1 >= 0 and m * t + m < H]
    tx = [t for t in range(-(-W // m)) if m * t - 1 >= 0 and m * t + m < W]
    return ty, tx
