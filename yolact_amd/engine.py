"""Execution plan for the HIP forward pass: weight packing, activation arena, op list.

A plan is built once per (batch, height, width): every convolution becomes one `ymi_conv_desc` with all
pointers/strides resolved, activations live in a small arena of reusable device buffers (NHWC), and the
forward pass is a flat loop of C-ABI calls on the current HIP stream — no Python tensor math, no host
synchronisation.  PyTorch is used for device memory only.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional

import torch
import torch.nn as nn

from . import _lib as L
from .config import act_name, make_priors_host
from . import modules as M
from .plan_tune import PlanTuning, _ceil


SPLIT_DEFAULT = '2'   # default of YOLACT_AMD_SPLIT (see Plan.__init__): 0 exact-fp32 MFMA, 1 bf16x3, 2 fp16x2


def split3_planes(w: torch.Tensor) -> torch.Tensor:
    """fp32 [..., R, K] -> bf16 bit patterns int16 [..., 3, R, K]: plane 0 = the top 8 significant bits of every value (its
    upper 16 bits, i.e. truncation to bf16), plane 1 = the top 8 bits of the exact remainder, plane 2 = what is left (at most
    8 bits, exactly a bf16).  plane0 + plane1 + plane2 == w bit for bit (csrc/conv_igemm.hip split8 does the same to the
    activations on the fly); used as `ymi_conv_desc.w_x3` by the bf16x3 tiles."""
    w = w.detach().to(torch.float32).contiguous()
    mask = -65536                                    # 0xFFFF0000 as int32

    def hi(t):                                       # (truncated value as fp32, its upper 16 bits as int16)
        u = t.view(torch.int32) & mask
        return u.view(torch.float32), (u >> 16).to(torch.int16)
    h, hb = hi(w)
    r = w - h
    m, mb = hi(r)
    r2 = r - m
    l, lb = hi(r2)
    # exact for every normal fp32 value; a subnormal input (|w| < 1.2e-38) keeps its top 7 mantissa bits only (error < 1e-40)
    assert bool(((h + m + l - w).abs() <= 1e-38).all()) or not torch.isfinite(w).all()
    return torch.stack([hb, mb, lb], dim=-3).contiguous()


def split2_planes_f16(w: torch.Tensor):
    """fp32 [..., R, K] -> (fp16 bit patterns int16 [..., 2, R, K], inverse row scales fp32 [..., R]) for the fp16x2 tiles
    (csrc/conv_igemm.hip split8h does the same to the activations on the fly): row r is scaled by the power of two s_r that maps
    max|w[r, :]| into [2^13, 2^14) (all-zero rows: 1); plane 0 = fp16(w s) by round to nearest, plane 1 = fp16(w s - plane 0)
    (the difference is exact in fp32).  11 + 11 significant bits + two signs: about two thirds of all fp32 values are represented
    exactly, the rest to one fp32 ulp, unbiased.  The second result is 1 / s_r (exact), folded into the epilogue's per-channel
    scale by the callers."""
    w = w.detach().to(torch.float32).contiguous()
    amax = w.abs().amax(dim=-1)
    _, e = torch.frexp(amax)                                   # amax = m * 2^e with 0.5 <= m < 1, i.e. amax < 2^e
    s = torch.ldexp(torch.ones_like(amax), 14 - e)
    s = torch.where(amax > 0, s, torch.ones_like(s))
    t = w * s.unsqueeze(-1)                                    # exact: a power-of-two scale
    h = t.to(torch.float16)
    l = (t - h.to(torch.float32)).to(torch.float16)
    assert bool(torch.isfinite(h.float()).all()), 'fp16x2 filter planes overflowed'
    planes = torch.stack([h, l], dim=-3).contiguous().view(torch.int16)
    return planes, (1.0 / s).contiguous()


class Packed:
    """A convolution's filters in the engine layout [CoutPad][Kpad] (k = (ky*kw+kx)*Cin + c) + folded epilogue."""

    def __init__(self, weight, bias=None, bn: Optional[nn.BatchNorm2d] = None, stride=1, pad=0, cin_pad=None,
                 device=None):
        weight = weight.detach().to(torch.float32)
        Cout, Cin, kh, kw = weight.shape
        cin_p = cin_pad or Cin
        w = weight.permute(0, 2, 3, 1)
        if cin_p != Cin:
            w = torch.nn.functional.pad(w, (0, cin_p - Cin))
        K = kh * kw * cin_p
        self.Kpad, self.CoutPad = _ceil(K, 32), _ceil(Cout, 128)
        wp = torch.zeros(self.CoutPad, self.Kpad, dtype=torch.float32, device=weight.device)
        wp[:Cout, :K] = w.reshape(Cout, K)
        self.w = wp.to(device).contiguous()
        self._wp_host, self._w3, self._h2 = wp, None, None
        self.weight_oihw = weight if (kh == 3 and kw == 3) else None     # Winograd transform source
        self.Cin, self.Cout, self.kh, self.kw, self.stride, self.pad = cin_p, Cout, kh, kw, stride, pad
        self.cin_alg = Cin
        self.cout_alg = Cout           # real output channels when Cout carries zero-filter padding (FLOP accounting)
        scale = shift = None
        if bn is not None:
            # torch's eval BatchNorm: alpha = gamma * rsqrt(var + eps); y = x*alpha + (beta - mean*alpha), fp32
            invstd = 1.0 / torch.sqrt(bn.running_var.detach().float() + bn.eps)
            scale = bn.weight.detach().float() * invstd
            shift = bn.bias.detach().float() - bn.running_mean.detach().float() * scale
            if bias is not None:
                shift = shift + bias.detach().float() * scale
        elif bias is not None:
            shift = bias.detach().float()
        self.scale = scale.to(device).contiguous() if scale is not None else None
        self.bias = shift.to(device).contiguous() if shift is not None else None

    def tiny_columns(self, binades=10, in_gain=None):
        """True when this layer looks like the CONSUMER OF COMPENSATED OUTLIER CHANNELS: some input channel is weighted >= 2^binades
        less than the typical one (column maximum over filters and taps against the median column maximum; all-zero padding columns
        ignored) AND — `in_gain`, the per-channel gain of the launches that PRODUCE the input tensor (Packed.out_gain, carried on
        engine.T) — that very channel is amplified by its producer >= 2^(binades - 4) over the typical channel.  Both halves are the
        signature of a BN-folded checkpoint with outlier channels (a huge gamma / sigma on the producer, the inverse folded into the
        consumer's filters): the typical channels then sit that many binades below the tensor's magnitude bound, and the fp16x2
        tiles — ONE power-of-two scale per activation tensor — keep the low piece of a value normal only 15 binades below the bound
        (tests/test_gpu_batch_parity.py test_outlier_channels_end_to_end_at_batch8: 2^12 outliers 9e-6, 2^14 3e-5, 2^16
        1.3e-4 of the head tensors).  Such layers run on the bf16x3 tiles instead (bf16 has the fp32 exponent range: no scale, no
        dependence on the bound).
        Tiny columns ALONE are not enough (round-4 advisor): weight decay drives the filters of DEAD input channels to zero in real
        checkpoints — same column signature, ordinary activations, no precision problem — and demoting those layers would silently
        cost them the fp16x2 tiles, Winograd and every fusion.  Without producer information (in_gain None) the weights-only test is
        kept, conservatively."""
        memo = getattr(self, '_tiny_memo', None)
        if memo is None:
            memo = self._tiny_memo = {}
        mkey = (binades, None if in_gain is None else (id(in_gain), int(in_gain.numel())))
        if mkey in memo and (in_gain is None or memo[mkey][1] is in_gain):      # (the gain tensor is kept: its id cannot be reused)
            return memo[mkey][0]
        r = self._tiny_columns(binades, in_gain)
        memo[mkey] = (r, in_gain)
        return r

    def _tiny_columns(self, binades, in_gain):
        w = self._wp_host[:self.Cout, :self.kh * self.kw * self.Cin].abs().float().cpu()
        col = w.view(self.Cout, self.kh * self.kw, self.Cin).amax(dim=(0, 1))
        nzm = col > 0
        if int(nzm.sum()) <= 8:
            return False
        tiny = nzm & (col * float(2 ** binades) < col[nzm].median())
        if not bool(tiny.any()):
            return False
        if in_gain is None:
            return True
        g = in_gain.detach().float().cpu().flatten()
        if g.numel() < self.Cin:                                     # (channel padding of the consumer: padded channels carry no data)
            g = torch.nn.functional.pad(g, (0, self.Cin - g.numel()))
        g = g[:self.Cin]
        pos = g[g > 0]
        if pos.numel() == 0:
            return True
        return bool((tiny & (g >= pos.median() * float(2 ** max(binades - 4, 1)))).any())

    def out_gain(self):
        """[Cout] per-output-channel gain of this layer: max|w[n, :]| x |folded BN scale[n]| (1 without BN) + |folded shift[n]| — how
        large the launch can make each channel it writes relative to the others.  Consumers compare it across channels
        (tiny_columns): an outlier channel of a BN-folded checkpoint shows up as a gain far above the median, whether it comes from a
        huge gamma / sigma or from a huge beta / mean shift (round-5 advisor: the shift used to be ignored; adding it is the
        conservative fold — ordinary checkpoints have |shift| = O(1), which moves no channel 2^6 above the median)."""
        if getattr(self, '_out_gain', None) is None:
            g = self._wp_host[:self.Cout].abs().amax(dim=1).float().cpu()
            if self.scale is not None:
                g = g * self.scale.detach().abs().float().cpu()
            if self.bias is not None:
                g = g + self.bias.detach().abs().float().cpu()[:self.Cout]
            self._out_gain = g
        return self._out_gain

    def _invalidate(self):
        self._w3 = self._h2 = None
        self._out_gain = self._l1_gain = None
        self._tiny_memo = {}

    def scale_out_channels(self, f: torch.Tensor):
        """Multiply output channel n of this layer by f[n] (host tensor [Cout], exact powers of two: Plan._rebalance_outliers): the
        folded scale and shift carry it, the filters are untouched."""
        f = f.detach().float().cpu()
        dev = self.w.device
        sc = self.scale.detach().float().cpu() if self.scale is not None else torch.ones(self.Cout)
        self.scale = (sc * f).to(dev).contiguous()
        if self.bias is not None:
            self.bias = (self.bias.detach().float().cpu() * f).to(dev).contiguous()
        self._invalidate()

    def scale_in_channels(self, f: torch.Tensor):
        """Multiply the filters of INPUT channel c (every tap, every filter) by f[c] (host tensor [Cin], exact powers of two)."""
        f = f.detach().float().cpu()
        taps = self.kh * self.kw
        assert self.Kpad == taps * self.Cin and f.numel() == self.Cin
        wp = self._wp_host.detach().float().cpu().clone()
        wp.view(self.CoutPad, taps, self.Cin).mul_(f.view(1, 1, -1))
        self._wp_host = wp
        self.w = wp.to(self.w.device).contiguous()
        if self.weight_oihw is not None:
            self.weight_oihw = self.weight_oihw.detach().float().cpu() * f.view(1, -1, 1, 1)
        self._invalidate()

    def in_column_max(self):
        """[Cin] max |w| over filters and taps per input channel (host)."""
        w = self._wp_host[:self.Cout, :self.kh * self.kw * self.Cin].detach().abs().float().cpu()
        return w.view(self.Cout, self.kh * self.kw, self.Cin).amax(dim=(0, 1))

    def l1_gain(self):
        """(max_n(|folded BN scale_n| * sum_k |w[n, k]|), max_n |folded shift_n|): |y_n| <= amax(x) * gain + shift_max for every
        output of this layer before the residual / activation — the rigorous bound csrc/chain2.hip scales its y slices by
        (ymi_chain_desc.gain_a / bias_max_a)."""
        if getattr(self, '_l1_gain', None) is None:
            g = self._wp_host[:self.Cout].detach().cpu().abs().double().sum(dim=1)
            if self.scale is not None:
                g = g * self.scale.detach().abs().double().cpu()
            b = float(self.bias.detach().abs().max().cpu()) if self.bias is not None else 0.0
            self._l1_gain = (float(g.max()) * (1.0 + 2.0 ** -20), b)       # (a hair above the fp64 sum: fp32 evaluation on the device)
        return self._l1_gain

    def w3(self):
        """[3][CoutPad][Kpad] bf16 planes of the same filters for the bf16x3 tiles (built on first use)."""
        if self._w3 is None:
            self._w3 = split3_planes(self._wp_host.cpu()).to(self.w.device)
        return self._w3


    def h2(self):
        """(planes [2][CoutPad][Kpad] fp16, scale_h2 [CoutPad] = folded-BN scale / the row's filter scale, winv_h2 [CoutPad] =
        1 / the row's filter scale) for the fp16x2 tiles (ymi_conv_desc.w_h2 / scale_h2 / winv_h2); built on first use."""
        if self._h2 is None:
            planes, winv = split2_planes_f16(self._wp_host.cpu())
            sc = torch.ones(self.CoutPad, dtype=torch.float32, device='cpu')    # (explicit: eval.py:1080 makes CUDA the default tensor type)
            if self.scale is not None:
                sc[:self.Cout] = self.scale.detach().float().cpu()
            dev = self.w.device
            self._h2 = (planes.to(dev), (sc * winv).contiguous().to(dev), winv.to(dev))
        return self._h2


class WinoPacked:
    """Winograd filters U = G g G^T in fp64 -> fp32, layout [(m+2)^2][CoutPad][C] (csrc/winograd.hip); m = 2: F(2x2,3x3),
    m = 4: F(4x4,3x3) (matrices of Lavin & Gray, interpolation points 0, +-1, +-2, inf)."""

    G2 = torch.tensor([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]], dtype=torch.float64)
    G4 = torch.tensor([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6],
                       [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]], dtype=torch.float64)

    def __init__(self, weight, device, m=2):
        w = weight.detach().to(torch.float64).cpu()                 # [Cout, Cin, 3, 3]
        Cout, Cin = w.shape[:2]
        G = self.G4 if m == 4 else self.G2
        a = m + 2
        u = torch.einsum('ai,ncij,bj->abnc', G, w, G)                # [a,a,Cout,Cin]
        self.m = m
        self.CoutPad = _ceil(Cout, 128)
        up = torch.zeros(a * a, self.CoutPad, Cin, dtype=torch.float32)
        up[:, :Cout] = u.reshape(a * a, Cout, Cin).to(torch.float32)
        self.u = up.to(device).contiguous()
        self._up_host, self._u3, self._uh2 = up, None, None

    def u3(self):
        """[G][3][CoutPad][C] bf16 planes of U for the bf16x3 GEMM tiles."""
        if self._u3 is None:
            self._u3 = split3_planes(self._up_host).to(self.u.device)
        return self._u3


def _wino_h2(self):
    """([G][2][CoutPad][C] fp16 planes of U, [G][CoutPad] inverse row scales) for the fp16x2 GEMM tiles."""
    if self._uh2 is None:
        planes, uinv = split2_planes_f16(self._up_host)
        self._uh2 = (planes.to(self.u.device), uinv.to(self.u.device))
    return self._uh2


WinoPacked.h2 = _wino_h2


def wino_eligible(pk, res, segs, act, x_C):
    if not (pk.kh == 3 and pk.kw == 3 and pk.stride == 1 and pk.pad == 1 and pk.Cin % 32 == 0
            and pk.cin_alg == pk.Cin and x_C == pk.Cin and res is None):
        return False
    if segs is not None:                       # segmented scatter (prediction heads): any Cout / activation
        return len(segs) <= 3
    return pk.Cout % 4 == 0 and act in (L.ACT_NONE, L.ACT_RELU, L.ACT_LEAKY01)


def pack_offmask(conv: nn.Conv2d, device, interleave: bool) -> Packed:
    """conv_offset_mask of a DCN layer (dcn_v2.py:107-112: 27 filters = 18 offsets | 9 mask logits) with its filter ROWS zero-padded
    to 32 — a full 128-byte line per pixel, and Cout % 4 == 0 admits the pipelined kernel and its 32-column tiles (YMI_DCNP_*x32) —
    and, `interleave`, permuted to [dh_k, dw_k, mask_k] per tap (ymi_dcn_desc.om_layout = 1: one 12-byte load per tap in the gather
    kernel).  The arithmetic of the 27 real channels is untouched: same filters, same order of accumulation."""
    w, b = conv.weight.detach().float(), conv.bias.detach().float()
    assert w.shape[0] == 27 and conv.stride[0] == conv.stride[1] and conv.padding == (1, 1), 'conv_offset_mask of a 3x3 one-group DCN'
    order = [c for k in range(9) for c in (2 * k, 2 * k + 1, 18 + k)] if interleave else list(range(27))
    wp, bp = w.new_zeros((32,) + tuple(w.shape[1:])), b.new_zeros(32)
    wp[:27], bp[:27] = w[order], b[order]
    pk = Packed(wp, bp, None, conv.stride[0], 1, None, device)
    pk.cout_alg = 27
    return pk


def pack_module(conv: nn.Conv2d, bn=None, device=None, cin_pad=None) -> Packed:
    assert conv.dilation == (1, 1) and conv.groups == 1
    assert conv.stride[0] == conv.stride[1] and conv.padding[0] == conv.padding[1]
    return Packed(conv.weight, conv.bias, bn, conv.stride[0], conv.padding[0], cin_pad, device)


class T:
    """An NHWC activation living in an arena buffer."""
    __slots__ = ('buf', 'B', 'H', 'W', 'C', 'slot', 'gain')

    def __init__(self, buf, B, H, W, C, slot=None, gain=None):
        self.buf, self.B, self.H, self.W, self.C = buf, B, H, W, C
        self.slot = slot          # index of the tensor's magnitude bound in Plan.amax (fp16x2 tiles), None: not tracked
        self.gain = gain          # [C] per-channel gain of the launches that write this tensor (Packed.out_gain; host tensor), None: unknown

    @property
    def ptr(self):
        return self.buf.data_ptr()

    def view(self):
        return self.buf[: self.B * self.H * self.W * self.C].view(self.B, self.H, self.W, self.C)


class Arena:
    """Best-fit reuse of device buffers; ops run in program order on one stream so reuse is race-free.
    Keeps the working set small enough to sit in the 256 MB Infinity Cache between layers."""

    def __init__(self, device):
        self.device = device
        self.free_list: List[torch.Tensor] = []
        self.all: List[torch.Tensor] = []

    def alloc(self, numel) -> torch.Tensor:
        best = None
        for i, b in enumerate(self.free_list):
            if b.numel() >= numel and (best is None or b.numel() < self.free_list[best].numel()):
                best = i
        if best is not None:
            return self.free_list.pop(best)
        b = torch.empty(numel, dtype=torch.float32, device=self.device)
        self.all.append(b)
        return b

    def free(self, t):
        if isinstance(t, _Borrowed):
            return  # owned by someone else (a stage output the FPN still needs)
        buf = t.buf if isinstance(t, T) else t
        assert all(buf is not f for f in self.free_list)
        self.free_list.append(buf)

    def total_bytes(self):
        return sum(b.numel() * 4 for b in self.all)


def out_size(n, k, s, p):
    return (n + 2 * p - k) // s + 1


_SIDE_STREAMS = {}


def _side_stream(device):
    """The side stream of a new plan: one of a FIXED pool of YOLACT_AMD_SIDE_STREAMS (default 2) per device, handed out round robin (two: a
    caller that overlaps batches on a second main stream — bench.py --step-overlap 2 — then uses four streams in all; the FIFTH stream of a
    process was measured on the main stream's hardware queue again, session r6w).
    HIP folds the streams of a process onto GPU_MAX_HW_QUEUES (4) hardware queues in creation order; with one new torch stream per plan
    (rounds 1 - 5) the 4th plan of a process got a side stream on the MAIN stream's queue and its two-stream schedule ran 1.5x slower
    than a single stream (bench.py secondary.outlier_plan, session r6l: 1 180 - 1 260 images/s against 2 050 for the same plan on a
    stream of the pool).  YOLACT_AMD_SIDE_STREAMS=0: one new stream per plan (A/B switch)."""
    n = int(os.environ.get('YOLACT_AMD_SIDE_STREAMS', '2'))
    if n <= 0:
        return torch.cuda.Stream(device=device)
    pool = _side_pool(device, n)
    st = pool['streams'][pool['next'] % n]
    pool['next'] += 1
    return st


def _side_pool(device, n):
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    pool = _SIDE_STREAMS.get(key)
    if pool is None:
        # ALL streams of the pool are created at the first request, back to back: a stream created later — after RCCL or the caller
        # have created theirs — can land on the main stream's hardware queue again (session r6w: the third pool stream, created lazily
        # behind bench.py's second step stream and RCCL's, made the batch-1 plan 2.3x slower)
        pool = _SIDE_STREAMS[key] = {'streams': [torch.cuda.Stream(device=device) for _ in range(n)], 'next': 0}
    return pool


def side_stream_pool(device):
    """The pooled side streams of a device (created on first use; () with YOLACT_AMD_SIDE_STREAMS=0).  yolact_amd.pipeline.BatchPipeline
    runs its un-forked plan slots on them: a plan that does not fork leaves its side stream idle, and a process should not keep more than
    four streams busy (_side_stream)."""
    n = int(os.environ.get('YOLACT_AMD_SIDE_STREAMS', '2'))
    return tuple(_side_pool(device, n)['streams']) if n > 0 else ()


class _OpList(list):
    """The plan's op list: a list that counts its mutations.  The native executor's ymi_plan_op array bakes descriptor addresses and
    op kinds; it is rebuilt whenever `version` moved (round-5 advisor: the earlier key, the ids of the op tuples, could repeat once the
    tuner / the fusions had replaced a tuple and CPython reused the freed one's id)."""
    version = 0

    def _bump(self):
        self.version += 1

    def __setitem__(self, k, v):
        self._bump(); list.__setitem__(self, k, v)

    def __delitem__(self, k):
        self._bump(); list.__delitem__(self, k)

    def append(self, v):
        self._bump(); list.append(self, v)

    def insert(self, k, v):
        self._bump(); list.insert(self, k, v)

    def pop(self, *a):
        self._bump(); return list.pop(self, *a)

    def extend(self, it):
        self._bump(); list.extend(self, it)


class Plan(PlanTuning):       # (plan_tune.py: tune() and everything it needs, tile candidates and fusions included)
    def __init__(self, net, B, H, W, device, dry_two_streams=False):
        """`dry_two_streams`: emit the two-stream op list (fork / join markers, per-stream arenas) without creating HIP
        streams or events — for static checks of the schedule on a machine without a GPU (tests/test_plan_schedule.py);
        such a plan cannot be run."""
        self.net, self.B, self.H, self.W, self.device = net, B, H, W, device
        self.ops = _OpList()   # (callable, args...) executed in order; counts its mutations (native executor cache)
        self.conv_meta = []    # (name, desc) for profiling / roofline accounting
        self.arena = Arena(device)
        self.keepalive = []
        self.lib = L.lib()
        # Two HIP streams: A = the caller's current stream (backbone, P3 branch, protonet), B = a side stream for the
        # small P4..P7 FPN/head convs and Detect, which are latency-bound and leave most CUs idle when run alone
        # (profiles/r01_layers_v4.txt: 0.7 ms of < 60 TF/s layers + 0.35 ms of Detect per batch-8 step).
        self.two_streams = (device.type == 'cuda' and os.environ.get('YOLACT_AMD_STREAMS', '2') != '1') or dry_two_streams
        # ONE side stream per device for every plan of the process (round 6): each torch.cuda.Stream() is another HIP stream, HIP folds
        # streams onto GPU_MAX_HW_QUEUES (4) hardware queues, and the 4th / 5th plan of a process (other batch sizes, a second model)
        # got a side stream that shared a hardware queue with the main stream — its two-stream schedule then ran 1.5x SLOWER than
        # one stream (bench.py's outlier_plan line: 5.7 ms against 4.1 single-stream and 3.8 for the same plan built first)
        self.stream_b = _side_stream(device) if self.two_streams and device.type == 'cuda' else None
        self.overlap = True      # runtime switch: False runs the same op list on ONE stream (serialised kernels), which
                                 # is what per-kernel timing (bench.py's roofline pass) needs
        self.events = {}
        self._cur = 'A'
        # YOLACT_AMD_WINOGRAD: 0 = direct kernels only, 2 = F(2x2,3x3) only, 4 = F(4x4,3x3) only, default both (autotuned)
        wsel = os.environ.get('YOLACT_AMD_WINOGRAD', '1')
        self.use_winograd = device.type == 'cuda' and wsel != '0'
        self.wino_variants = (2,) if wsel == '2' else (4,) if wsel == '4' else (2, 4)
        # YOLACT_AMD_WINOGRAD_FORCE=1: take the Winograd path on every eligible layer even where the direct kernel
        # measured faster (parity tests of the least accurate variant; never the default)
        self.wino_force = os.environ.get('YOLACT_AMD_WINOGRAD_FORCE', '0') == '1'
        # YOLACT_AMD_SPLIT=1: the bf16x3 variants of the GEMM tiles (fp32-class products on the bf16 matrix pipe, 6 bf16
        # MFMAs per product at 16x the fp32-MFMA rate, csrc/conv_igemm.hip split8) join the candidates of every Cin % 32
        # == 0 layer and of the Winograd GEMMs; the measurement decides per shape
        # YOLACT_AMD_SPLIT=2 (default): the fp16x2 variants instead — two fp16 pieces by round to nearest, 3 fp16 MFMAs per product
        # (half the matrix-pipe work of bf16x3, no byte permutes in the split).  Activations are scaled per tensor by a power of
        # two derived from a magnitude bound that every producing launch records on the device (`self.amax`, one float per
        # tensor, zeroed at the start of a run and raised atomically by the epilogues: ymi_conv_desc.y_amax / x_amax)
        smode = os.environ.get('YOLACT_AMD_SPLIT', SPLIT_DEFAULT)
        self.split = smode == '1'
        self.h2 = smode == '2'
        self.mode = 'x3' if self.split else 'h2' if self.h2 else ''        # arithmetic of the plan as the table keys name it (tune_table.MODES)
        self.amax = torch.zeros(512 * L.AMAX_SLOT_FLOATS, dtype=torch.float32, device=device)     # 2 MB: 512 slots
        self._nslots = 0
        # YOLACT_AMD_SPLITK=0 keeps every GEMM a single pass (no split-K candidates in the tuner)
        self.splitk = os.environ.get('YOLACT_AMD_SPLITK', '1') == '1'
        # YOLACT_AMD_PIPE=0 keeps the pipelined kernel of csrc/dcn.hip out of the candidates of ORDINARY convolutions (A/B switch)
        self.pipe = os.environ.get('YOLACT_AMD_PIPE', '1') == '1'
        # YOLACT_AMD_WIDE_GUARD=0: keep fp16x2 tiles even on layers whose filters give away outlier input channels (tests of the
        # unguarded behaviour); default: such layers run on bf16x3 tiles (Packed.tiny_columns)
        self.wide_guard = os.environ.get('YOLACT_AMD_WIDE_GUARD', '1') == '1'
        # DCN layers: conv_offset_mask padded to 32 filters / tap-interleaved channel order (pack_offmask); 0 = the reference's 27 / order
        self.om_pad = os.environ.get('YOLACT_AMD_OM_PAD', '1') == '1'
        self.om_interleave = os.environ.get('YOLACT_AMD_OM_INTERLEAVE', '1') == '1'
        # YOLACT_AMD_NATIVE_EXEC=0: issue the op list from the Python loop (one ctypes call per launch) instead of csrc/plan_exec.cpp
        self.native_exec = device.type == 'cuda' and os.environ.get('YOLACT_AMD_NATIVE_EXEC', '1') == '1'
        self._native, self._native_events, self._stem_desc = None, None, None
        self.wide_ops = set()
        self.wide_layers = []       # names of the layers the outlier-channel guard took off the fp16x2 tiles (warned about once, below)
        self._sk_ws = {}
        self.down_on_side_stream = os.environ.get('YOLACT_AMD_DOWN_STREAM', 'B') == 'B'      # measured +1 %
        self.wino_alt, self._wino_packed, self._wino_ws = {}, {}, {}
        self.level_merge, self.merged_levels = None, False     # P4..P7 heads as one Winograd layer per shared conv (_build_level_merge)
        self._upsrc, self.wino_up = {}, {}     # 2x bilinear upsampling feeding a 3x3 conv: fused into its F(4x4) input transform
        self._done_event = None
        self._priors_timed = False
        self.param_stamp = None
        self.tune_misses = 0
        self._build()
        if self.wide_layers:
            import warnings
            warnings.warn('yolact_amd: %d layer(s) consume compensated OUTLIER channels (tiny filter columns on channels their producer '
                          'amplifies, Packed.tiny_columns) and run on bf16x3 / exact-fp32 tiles instead of fp16x2, without Winograd and '
                          'the fp16x2-only fusions: %s.  YOLACT_AMD_WIDE_GUARD=0 keeps fp16x2 (at reduced accuracy for such checkpoints).'
                          % (len(self.wide_layers), ', '.join(self.wide_layers[:12]) + (' ...' if len(self.wide_layers) > 12 else '')),
                          RuntimeWarning, stacklevel=2)
        self._bind_wino_workspaces()
        self.sections = [None if op[0] in ('record', 'wait', 'detect', 'nop') else self.section_of(op[2]) for op in self.ops]

    # ---- op emitters ---------------------------------------------------------------------------
    def _arena(self):
        # buffers are recycled only among ops of the SAME stream: program order on one stream makes reuse race-free,
        # across streams it would not be
        if self._cur == 'B':
            if not hasattr(self, 'arena_b'):
                self.arena_b = Arena(self.device)
            return self.arena_b
        return self.arena

    def _new(self, B, H, W, C, slot=None, gain=None) -> T:
        return T(self._arena().alloc(B * H * W * C), B, H, W, C, slot, gain)

    def _slot(self):
        """A fresh magnitude-bound slot (index into self.amax)."""
        self._nslots += 1
        assert self._nslots * L.AMAX_SLOT_FLOATS <= self.amax.numel()
        return self._nslots - 1

    def _slot_ptr(self, slot):
        return self.amax.data_ptr() + 4 * L.AMAX_SLOT_FLOATS * slot

    def bound(self, slot):
        """Host read of a slot's value (diagnostics / tests): the maximum over its sub-slots."""
        return float(self.amax[slot * L.AMAX_SLOT_FLOATS:(slot + 1) * L.AMAX_SLOT_FLOATS].max())

    def free(self, t):
        self._arena().free(t)

    def conv(self, name, x: T, pk: Packed, act=L.ACT_NONE, res: Optional[T] = None, res_mode=L.RES_NONE,
             res_after_act=0, out: Optional[T] = None, segs=None, dcn_offmask: Optional[T] = None) -> Optional[T]:
        """Emit one fused convolution. `segs`: list of (n0, n1, act, row_stride, batch_stride, ptr) overrides the
        single dense NHWC output."""
        assert x.C == pk.Cin, (name, x.C, pk.Cin)
        Ho, Wo = out_size(x.H, pk.kh, pk.stride, pk.pad), out_size(x.W, pk.kw, pk.stride, pk.pad)
        d = L.ConvDesc()
        d.x, d.w = x.ptr, pk.w.data_ptr()
        d.scale = pk.scale.data_ptr() if pk.scale is not None else None
        d.bias = pk.bias.data_ptr() if pk.bias is not None else None
        d.B, d.H, d.W, d.Cin, d.ldx = x.B, x.H, x.W, pk.Cin, x.C
        d.Ho, d.Wo, d.Cout = Ho, Wo, pk.Cout
        d.kh, d.kw, d.stride, d.pad, d.Kpad = pk.kh, pk.kw, pk.stride, pk.pad, pk.Kpad
        d.res_mode = res_mode
        d.res_after_act = res_after_act
        if res is not None:
            d.res, d.res_ld, d.res_H, d.res_W = res.ptr, res.C, res.H, res.W
            if res_mode == L.RES_ADD:
                assert (res.B, res.H, res.W, res.C) == (x.B, Ho, Wo, pk.Cout), name
        d.tile = L.TILE_AUTO
        d.cin_alg = pk.cin_alg
        d.cout_alg = pk.cout_alg
        # fp16x2 plans: a layer whose filters give away outlier input channels runs on the bf16x3 tiles (Packed.tiny_columns)
        wide = self.h2 and self.wide_guard and pk.Cin % 32 == 0 and pk.tiny_columns(in_gain=x.gain)
        pk.wide = wide
        if wide:
            self.wide_layers.append(name)
        # the gain this launch gives each channel it writes; a shortcut / FPN sum inherits the larger of its two sources
        og = pk.out_gain()
        if res is not None and res.gain is not None and res.gain.numel() == og.numel():
            og = torch.maximum(og, res.gain)
        self.last_out_gain = og
        if (self.split or wide) and dcn_offmask is None:
            d.w_x3 = pk.w3().data_ptr()
        yslot = self._slot()                    # fp16x2 plans: every launch records the magnitude bound of what it writes
        for _ in range(len(segs) - 1 if segs else 0):       # (one slot per output segment, consecutive: ABI 5)
            self._slot()
        if self.h2:                             # (csrc/common.h: one XCD-local atomic per wave at most); consumers read it as
            d.y_amax = self._slot_ptr(yslot)    # x_amax.  The bf16x3 / exact-fp32 plans need no bounds and do not pay for them
        if x.slot is not None:
            d.x_amax = self._slot_ptr(x.slot)
        if self.h2:                             # (DCN layers too: the gathered fp32 tile is split like any other A tile)
            assert x.slot is not None, name
            planes, sc2, winv = pk.h2()
            d.w_h2, d.scale_h2, d.winv_h2 = planes.data_ptr(), sc2.data_ptr(), winv.data_ptr()
        self.last_yslot = yslot
        y = None
        if segs is None:
            y = out if out is not None else self._new(x.B, Ho, Wo, pk.Cout)
            y.slot = yslot
            y.gain = og
            d.nseg = 1
            d.seg[0] = L.ConvSeg(0, pk.Cout, act, pk.Cout, Ho * Wo * pk.Cout, y.ptr)
        else:
            d.nseg = len(segs)
            for i, s in enumerate(segs):
                d.seg[i] = L.ConvSeg(*s)
        self.keepalive.append(pk)
        if not hasattr(self, '_desc_info'):
            self._desc_info = {}
        self._desc_info[C.addressof(d)] = (pk, res.slot if res is not None else None)     # (the chain fusion needs both: l1_gain, res_amax)
        wino = None
        if (self.use_winograd and dcn_offmask is None and out is None and pk.weight_oihw is not None and not wide
                and wino_eligible(pk, res, segs, act, x.C)):
            wino = [w for w in (self._wino_op(x, pk, act, y, name, segs, m) for m in self.wino_variants) if w is not None]
            wino = wino or None
        if dcn_offmask is not None:
            dd = L.DcnDesc()
            dd.conv = d
            dd.offmask, dd.ldo = dcn_offmask.ptr, dcn_offmask.C
            dd.om_layout = 1 if (self.om_pad and self.om_interleave) else 0
            self.ops.append((self.lib.ymi_dcn_v2_forward_f32, C.pointer(dd), name, self._cur))
            self.conv_meta.append((name, dd.conv))
            if wide:
                self.wide_ops.add(len(self.ops) - 1)
        else:
            self.ops.append((self.lib.ymi_conv2d_nhwc_f32, C.pointer(d), name, self._cur))
            self.conv_meta.append((name, d))
            if wide:
                self.wide_ops.add(len(self.ops) - 1)
            if wino is not None:
                self.wino_alt[len(self.ops) - 1] = wino      # op index -> alternative; autotune picks the faster one
                if id(x) in self._upsrc:
                    self.wino_up[len(self.ops) - 1] = self._upsrc[id(x)]
        return y

    def _wino_op(self, x: T, pk: Packed, act, y: Optional[T], name, segs=None, m=2):
        """Winograd alternative of a 3x3 / stride-1 conv: descriptor + per-stream workspaces (V, M)."""
        key = (id(pk), m)
        wp = self._wino_packed.get(key)
        if wp is None:
            wp = self._wino_packed[key] = WinoPacked(pk.weight_oihw, self.device, m)
        th, tw = (x.H + m - 1) // m, (x.W + m - 1) // m
        Tn = x.B * th * tw
        Ng = _ceil(pk.Cout, 4)
        if Tn * max(pk.Cin, Ng) >= (1 << 29):
            return None
        g = (m + 2) * (m + 2)
        need_v, need_m = g * Tn * pk.Cin, g * Tn * Ng
        ws = self._wino_ws.setdefault(self._cur, [None, None])
        if ws[0] is None or ws[0].numel() < need_v:
            ws[0] = torch.empty(need_v, dtype=torch.float32, device=self.device)
        if ws[1] is None or ws[1].numel() < need_m:
            ws[1] = torch.empty(need_m, dtype=torch.float32, device=self.device)
        d = L.WinoDesc()
        d.x, d.u = x.ptr, wp.u.data_ptr()
        if self.split:
            d.u_x3 = wp.u3().data_ptr()
        if self.h2:
            planes, uinv = wp.h2()
            d.u_h2, d.uinv_h2 = planes.data_ptr(), uinv.data_ptr()
        if x.slot is not None:
            d.x_amax = self._slot_ptr(x.slot)
        if self.h2:
            d.y_amax = self._slot_ptr(self.last_yslot)    # same slot as the direct descriptor of this layer
        if segs is None:
            d.y = y.ptr
        else:
            d.nseg = len(segs)
            for i, s in enumerate(segs):
                d.seg[i] = L.ConvSeg(*s)
        d.scale = pk.scale.data_ptr() if pk.scale is not None else None
        d.bias = pk.bias.data_ptr() if pk.bias is not None else None
        d.B, d.H, d.W, d.C, d.Cout, d.act, d.tile, d.m = x.B, x.H, x.W, pk.Cin, pk.Cout, act, L.TILE_AUTO, m
        d.cout_alg = pk.cout_alg
        return d

    def _bind_wino_workspaces(self):
        """Workspaces may have been re-allocated (grown) while the plan was built: point every descriptor at the final ones."""
        for idx, alts in self.wino_alt.items():
            ws = self._wino_ws[self.ops[idx][3]]
            for d in alts:
                d.V, d.M = ws[0].data_ptr(), ws[1].data_ptr()
        if self.level_merge is not None:
            ws = self._wino_ws[self.level_merge['where']]
            for d in self.level_merge['descs']:
                d.V, d.M = ws[0].data_ptr(), ws[1].data_ptr()

    # ---- the P4..P7 prediction heads as ONE Winograd layer per shared conv ---------------------------------------------------------------
    # share_prediction_module: every level applies the same up-feature conv and the same bbox | coef | conf conv, on maps of 35^2 .. 5^2
    # whose launches hold a handful of blocks each (18 launches, 7 % of a serial batch-8 step for 4 % of its FLOPs).  In the Winograd
    # domain the levels are just more rows of the grouped GEMM: ymi_wino_desc.nlev runs one input transform, one GEMM and one output
    # transform over the tiles of all of them (csrc/winograd.hip).  Built here as an ALTERNATIVE, like wino_alt: the op list stays the
    # per-level one, PlanTuning._merge_levels installs the two merged launches where they measured faster (YOLACT_AMD_MERGE_LEVELS).
    # The merged up-feature writes every level's output at once, so those get buffers of their own (the arena hands the per-level
    # launches the same buffer again and again); all levels raise ONE bound slot, which is the merged .out launch's input bound.
    def _build_level_merge(self, lev_ops, up_pk, head_pk, offs, widths, ncols, coef_act):
        self.level_merge = None
        self.merged_levels = False
        lv = sorted(l for l in lev_ops if l >= 1)
        if not (self.h2 and 2 <= len(lv) <= 5 and len(up_pk) == 1 and all(len(lev_ops[l]) == 3 for l in lv)):
            return
        pku = up_pk[0]
        if not all((pk.kh, pk.kw, pk.stride, pk.pad) == (3, 3, 1, 1) and pk.weight_oihw is not None and pk.Cin % 32 == 0
                   and not getattr(pk, 'wide', False) for pk in (pku, head_pk)) or pku.Cout % 32 != 0:
            return
        if any(i in self.wide_ops for l in lv for i in lev_ops[l][1:]):
            return
        feats = [lev_ops[l][0] for l in lv]
        B = feats[0].B
        Tn = sum(B * _ceil(f.H, 4) // 4 * (_ceil(f.W, 4) // 4) for f in feats)
        if Tn * max(pku.Cin, pku.Cout, _ceil(head_pk.Cout, 4)) >= (1 << 29):
            return
        ws = self._wino_ws.setdefault(self._cur, [None, None])
        need_v, need_m = 36 * Tn * max(pku.Cin, pku.Cout), 36 * Tn * max(pku.Cout, _ceil(head_pk.Cout, 4))
        if ws[0] is None or ws[0].numel() < need_v:
            ws[0] = torch.empty(need_v, dtype=torch.float32, device=self.device)
        if ws[1] is None or ws[1].numel() < need_m:
            ws[1] = torch.empty(need_m, dtype=torch.float32, device=self.device)
        mid = [torch.empty(B * f.H * f.W * pku.Cout, dtype=torch.float32, device=self.device) for f in feats]
        uslot, pubslot = self._slot(), self._slot()

        def base(pk, act):
            key = (id(pk), 4)
            wp = self._wino_packed.get(key)
            if wp is None:
                wp = self._wino_packed[key] = WinoPacked(pk.weight_oihw, self.device, 4)
            d = L.WinoDesc()
            d.u = wp.u.data_ptr()
            planes, uinv = wp.h2()
            d.u_h2, d.uinv_h2 = planes.data_ptr(), uinv.data_ptr()
            d.scale = pk.scale.data_ptr() if pk.scale is not None else None
            d.bias = pk.bias.data_ptr() if pk.bias is not None else None
            d.B, d.C, d.Cout, d.act, d.m, d.cout_alg = B, pk.Cin, pk.Cout, act, 4, pk.cout_alg
            d.tile, d.v_planes, d.nlev = L.TILE_128x128 | L.TILE_H2, 1, len(lv)
            for q, f in enumerate(feats):
                d.lev[q].H, d.lev[q].W = f.H, f.W
            d.H, d.W = 4 * (Tn // B), 4           # ignored by the launch: the virtual shape of its table key (tune_table.level_key)
            return d
        du = base(pku, L.ACT_RELU)
        du.lev_amax = self._slot_ptr(pubslot)
        for q, f in enumerate(feats):
            assert f.slot is not None
            du.lev[q].x, du.lev[q].x_amax = f.ptr, self._slot_ptr(f.slot)
            du.lev[q].y, du.lev[q].y_amax = mid[q].data_ptr(), self._slot_ptr(uslot)
        do = base(head_pk, L.ACT_NONE)
        d1 = self.ops[lev_ops[lv[0]][2]][1].contents            # head1.out's direct descriptor: segments and bound slots
        do.nseg, do.y_amax = d1.nseg, d1.y_amax
        off1 = offs[lv[0]]
        for k in range(d1.nseg):
            do.seg[k] = d1.seg[k]                               # (ptr = level 1's rows of the level-concatenated tensor)
        for q, l in enumerate(lv):
            do.lev[q].x, do.lev[q].x_amax = mid[q].data_ptr(), self._slot_ptr(uslot)
            for k in range(d1.nseg):
                do.lev[q].seg_off[k] = (offs[l] - off1) * widths[k] * 4
        # profile records map onto conv_meta by position: head1's two layers carry the launches, the absorbed ones follow as kind 12
        absorbed = []
        for l in lv[1:]:
            for i in lev_ops[l][1:]:
                absorbed.append(self.lib.ymi_conv_flops(C.byref(self.ops[i][1].contents)))
        do.nabs = len(absorbed)
        for q, fl in enumerate(absorbed):
            do.abs_flops[q] = fl
        self.keepalive += [mid, du, do]
        self.level_merge = {'where': self._cur, 'descs': (du, do), 'levels': lv, 'tiles': Tn // B,
                            'up': [lev_ops[l][1] for l in lv], 'out': [lev_ops[l][2] for l in lv], 'mid': mid,
                            'shape': (B, pku.Cin, pku.Cout, head_pk.Cout)}

    def call(self, fn, *args, name=''):
        self.ops.append((fn, args, name, self._cur))

    # ---- FPN laterals of the lower levels, launched EARLY on the side stream (round 5) ------------------------------------------------
    # lat_layers[i](C_j) depends only on backbone stage j (yolact.py:324-334); the top-down sum x_j = up(x_{j+1}) + lat(C_j) needs the
    # level above, i.e. the END of the backbone.  Fused in the lateral's epilogue (YMI_RES_BILINEAR) both sit on the critical path
    # behind C5; split, the lateral GEMMs of C3 / C4 run on stream B beside the later backbone stages — whose 35 x 35 / 18 x 18 launches
    # leave a fifth to a third of the CUs idle — and only ymi_bilinear_add_nhwc_f32 (a 20 us stream) stays behind C5.  Same
    # interpolation, same association (results differ only through the tile the residual-free lateral GEMM runs on).  MEASURED (session r5d, same box, alternating, profiles/r05_ab_runs.txt): 2011 - 2015
    # images/s with it against 2017 - 2028 without — the laterals slow the backbone launches they share the chip with by as much as
    # they save behind C5 (the finding of DESIGN 3.5 again: summed kernel time rises when streams overlap).  Hence OPT-IN:
    # YOLACT_AMD_EARLY_LAT=1; the default keeps the fused epilogue.
    def _stage_done(self, li, t):
        sel = self.net.backbone_selected
        if not self._early_lat_on or li not in sel or sel.index(li) >= len(sel) - 1:
            return
        self._pending_lat.append((li, t))

    def _flush_early_laterals(self):
        sel = self.net.backbone_selected
        n = len(sel)
        for li, t in self._pending_lat:
            j = sel.index(li)
            i = n - 1 - j
            # B may only start behind what A has issued SO FAR: the stage output is complete, and the projection shortcut the
            # side stream computed for the block just finished has been consumed (its buffer went back to B's pool and may be the
            # very one this lateral's output gets: tests/test_plan_schedule.py)
            self.record('latgo%d' % i)
            self.on('B')
            self.wait('latgo%d' % i)
            raw = self.conv('fpn.lat%d' % i, t, self._pack(self.net.fpn.lat_layers[i]))
            self.record('lat%d' % i)
            self.on('A')
            self.early_lat[j] = raw
        self._pending_lat = []

    # stream control (no-ops in single-stream mode): ops emitted after on('B') go to the side stream
    def on(self, which):
        self._cur = which if self.two_streams else 'A'

    def record(self, ev):
        if self.two_streams:
            self.events[ev] = torch.cuda.Event() if self.device.type == 'cuda' else None
            self.ops.append(('record', ev, ev, self._cur))

    def wait(self, ev):
        if self.two_streams:
            self.ops.append(('wait', ev, ev, self._cur))

    # ---- filters, packed once per plan -----------------------------------------------------------------------------------------
    def _pack(self, conv, bn=None, cin_pad=None) -> Packed:
        """pack_module, memoised per (conv, bn): Plan._rebalance_outliers edits the Packed objects of a stage BEFORE the op emitters ask
        for them."""
        key = (id(conv), id(bn), cin_pad)
        pk = self._pk_cache.get(key)
        if pk is None:
            pk = self._pk_cache[key] = pack_module(conv, bn, self.device, cin_pad)
        return pk

    def _rebalance_outliers(self, bb):
        """COMPENSATED OUTLIER CHANNELS, rebalanced at pack time (round 6).  A BN-folded checkpoint can carry channels whose producers
        amplify them 2^k over the typical channel (a huge gamma / sigma) while every consumer's filters hold the inverse — exact in fp32,
        but the fp16x2 tiles give an activation tensor ONE power-of-two scale and a filter row ONE: the typical channels of such a
        tensor sit k binades below its bound.  Round 4 moved the consuming layers to bf16x3 tiles (Packed.tiny_columns: 18 layers, no
        Winograd, no fusions; bench.py secondary.outlier_plan: 6.85 ms instead of 3.94 per batch-8 step).  Here the re-parametrisation
        is UNDONE instead: channel c of a ResNet stage tensor is multiplied by 2^-k in every producer (each block's folded bn3 and the
        projection shortcut's BN: the identity shortcuts carry the same factor) and by 2^k in every consumer's filters (the conv1 of
        the following blocks, the next stage's conv1 / projection shortcut, the FPN lateral); likewise proto_net[0] -> proto_net[2].
        Powers of two commute with fp32 rounding and ReLU, so in fp32 arithmetic every product is unchanged — the network is the same
        function, with balanced tensors.  k = min(producer excess, consumer deficit) per channel, only where both exceed 2^6: a channel
        that is merely large (no tiny consumer column) is left alone — moving ITS range into the filter rows would cost them what it
        saves the tensor.  YOLACT_AMD_REBALANCE=0 keeps the checkpoint's own parametrisation (then the guard of round 4 acts)."""
        self.rebalanced = []
        if not (self.h2 and os.environ.get('YOLACT_AMD_REBALANCE', '1') == '1' and isinstance(bb, M.ResNetBackbone)):
            return

        def exps(gain, cols, thr=6):
            g = gain.double().clamp_min(0)
            pos = g[g > 0]
            if pos.numel() < 8:
                return None
            kg = torch.floor(torch.log2((g / pos.median()).clamp_min(2.0 ** -126)))
            c = cols.double()
            cpos = c[c > 0]
            if cpos.numel() < 8:
                return None
            kc = torch.floor(torch.log2((cpos.median() / c.clamp_min(2.0 ** -126))))
            k = torch.minimum(kg, kc).clamp(min=0, max=40)
            k = torch.where((kg >= thr) & (kc >= thr) & (c > 0), k, torch.zeros_like(k))
            return k if bool((k > 0).any()) else None
        layers = list(bb.layers)
        sel = list(self.net.backbone_selected)
        fpn = self.net.fpn
        for li, layer in enumerate(layers):
            blocks = list(layer)
            if not blocks or blocks[0].downsample is None:
                continue
            prod = [self._pack(b.conv3, b.bn3) for b in blocks] + [self._pack(blocks[0].downsample[0], blocks[0].downsample[1])]
            cons = [self._pack(b.conv1, b.bn1) for b in blocks[1:]]
            if li + 1 < len(layers):
                nb = list(layers[li + 1])[0]
                cons.append(self._pack(nb.conv1, nb.bn1))
                if nb.downsample is not None:
                    cons.append(self._pack(nb.downsample[0], nb.downsample[1]))
            if li in sel:
                cons.append(self._pack(fpn.lat_layers[len(sel) - 1 - sel.index(li)]))
            if not cons or any(pk.Cin != prod[0].Cout or pk.Kpad != pk.kh * pk.kw * pk.Cin for pk in cons):
                continue
            gain = torch.stack([pk.out_gain()[:prod[0].Cout] for pk in prod]).amax(0)
            cols = torch.stack([pk.in_column_max() for pk in cons]).amax(0)
            k = exps(gain, cols)
            if k is None:
                continue
            down, up = torch.pow(2.0, -k).float(), torch.pow(2.0, k).float()
            for pk in prod:
                pk.scale_out_channels(down)
            for pk in cons:
                pk.scale_in_channels(up)
            self.rebalanced.append(('C%d' % (li + 2), int((k > 0).sum()), int(k.max())))
        # proto_net[0] (3x3 + ReLU) -> proto_net[2]: the same signature one level down the P3 branch
        pm_ = list(self.net.proto_net)
        self._proto0_down = None
        if (len(pm_) > 2 and isinstance(pm_[0], nn.Conv2d) and isinstance(pm_[1], nn.ReLU) and isinstance(pm_[2], nn.Conv2d)
                and pm_[0].bias is not None):
            p0, p2 = self._pack(pm_[0]), self._pack(pm_[2])
            if p2.Cin == p0.Cout and p2.Kpad == p2.kh * p2.kw * p2.Cin:
                k = exps(p0.out_gain(), p2.in_column_max())
                if k is not None:
                    down, up = torch.pow(2.0, -k).float(), torch.pow(2.0, k).float()
                    p0.scale_out_channels(down)
                    p2.scale_in_channels(up)
                    self._proto0_down = down
                    self.rebalanced.append(('proto_net.0', int((k > 0).sum()), int(k.max())))

    # ---- graph construction --------------------------------------------------------------------
    def _build(self):
        net, B, H, W, dev = self.net, self.B, self.H, self.W, self.device
        cfg = net.cfg
        lib = self.lib
        ar = self.arena

        self.early_lat, self._pending_lat = {}, []
        self._early_lat_on = self.two_streams and os.environ.get('YOLACT_AMD_EARLY_LAT', '0') == '1'
        bb = net.backbone
        self._pk_cache = {}
        self._rebalance_outliers(bb)
        # ResNet stem (fp16x2 plans): layout change + 7x7/2 conv + BN + ReLU + 3x3/2 max-pool in ONE launch straight from the NCHW
        # input (csrc/stem.hip: 0.107 vs 0.168 ms for the three launches at batch 8, 0.020 vs 0.035 at batch 1, bit-identical (see the test for the exact statement)
        # output; profiles/r03_stem_probe.txt).  YOLACT_AMD_FUSED_STEM=0 keeps the separate launches.
        c1 = getattr(bb, 'conv1', None)
        self.fused_stem = (self.h2 and isinstance(bb, M.ResNetBackbone) and os.environ.get('YOLACT_AMD_FUSED_STEM', '1') == '1'
                           and c1 is not None and tuple(c1.kernel_size) == (7, 7) and tuple(c1.stride) == (2, 2)
                           and tuple(c1.padding) == (3, 3) and c1.in_channels == 3 and c1.out_channels == 64 and H >= 7 and W >= 7)
        x4 = None
        if not self.fused_stem:
            # input: NCHW fp32 -> NHWC with C padded to 4 (pointer patched per call)
            x4 = self._new(B, H, W, 4, slot=self._slot())
            self.in_args = [None, x4.ptr, B, 3, H, W]
            self.in_amax = (x4.ptr, B * H * W * 4, self._slot_ptr(x4.slot))    # the input's magnitude bound: ymi_amax_f32
            self.ops.append(('input', None, 'nchw_to_nhwc4', 'A'))
        if isinstance(bb, M.ResNetBackbone):
            outs = self._resnet(bb, x4)
        else:
            outs = self._darknet(bb, x4)
        self._flush_early_laterals()           # (anything still pending: a stage whose successor has no block to hide behind)
        sel = [outs[i] for i in net.backbone_selected]
        for i, t in enumerate(outs):
            if i not in net.backbone_selected and t is not None:
                ar.free(t)

        # FPN laterals + top-down sums (yolact.py:319-341) on stream A
        fpn = net.fpn
        n = len(sel)
        sums = [None] * n
        prev = None
        for i in range(n):
            j = n - 1 - i
            pk = self._pack(fpn.lat_layers[i])
            if j in self.early_lat and prev is not None:
                raw = self.early_lat[j]                 # lat(C_j), computed on B long ago; the sum happens here, in place
                self.wait('lat%d' % i)
                slot = self._slot()
                self.call(lib.ymi_bilinear_add_nhwc_f32, prev.ptr, raw.ptr, raw.B, prev.H, prev.W, raw.C, raw.H, raw.W,
                          self._slot_ptr(slot) if self.h2 else None, name='fpn.add%d' % i)
                raw.slot = slot
                if raw.gain is not None and prev.gain is not None and raw.gain.numel() == prev.gain.numel():
                    raw.gain = torch.maximum(raw.gain, prev.gain)
                sums[j] = raw
            elif prev is None:
                sums[j] = self.conv('fpn.lat%d' % i, sel[j], pk)
            else:
                sums[j] = self.conv('fpn.lat%d' % i, sel[j], pk, res=prev, res_mode=L.RES_BILINEAR)
            prev = sums[j]
        for t in sel:
            ar.free(t)

        # level geometry (pred convs keep the size, downsample convs are 3x3 / stride 2 / pad 1)
        shapes = [(t.H, t.W) for t in sums]
        for _ in fpn.downsample_layers:
            shapes.append((out_size(shapes[-1][0], 3, 2, 1), out_size(shapes[-1][1], 3, 2, 1)))
        self.feat_shapes = shapes
        nlev = len(shapes)

        # prediction heads (yolact.py:133-212), shared weights, one merged GEMM per level writing straight into
        # the level-concatenated [B,P,k] tensors
        pm = net.prediction_layers[0]
        A = pm.num_priors
        Ccls, D = cfg.num_classes, net.mask_dim
        cells = [h * w for h, w in shapes]
        P = sum(cells) * A
        self.P, self.A, self.D, self.Ccls = P, A, D, Ccls
        # class rows are padded to a multiple of 4 floats (81 -> 84): every head output row is then 16-byte aligned and the
        # head GEMM / Winograd output transform store float4s (the 243-float rows of the dense layout forced scalar
        # stores on 69 % of the head's output channels); Detect reads the rows with stride `conf_ld`
        Cp = _ceil(Ccls, 4) if os.environ.get('YOLACT_AMD_PAD_CONF', '1') == '1' else Ccls
        self.conf_ld = Cp
        self.loc = torch.empty(B, P, 4, device=dev)
        self.conf = torch.zeros(B, P, Cp, device=dev)
        self.coef = torch.empty(B, P, D, device=dev)
        up_pk = [pack_module(m, device=dev) for m in pm.upfeature if isinstance(m, nn.Conv2d)] \
            if hasattr(pm, 'upfeature') else []
        # row order bbox | coef | conf keeps the bbox and coef segments 16-byte aligned (vector stores)
        cw, cb = pm.conf_layer.weight, pm.conf_layer.bias
        if Cp != Ccls:      # zero filters for the padding columns of every anchor's class row
            cw = torch.nn.functional.pad(cw.view(A, Ccls, *cw.shape[1:]), (0, 0, 0, 0, 0, 0, 0, Cp - Ccls)).reshape(A * Cp, *cw.shape[1:])
            cb = torch.nn.functional.pad(cb.view(A, Ccls), (0, Cp - Ccls)).reshape(A * Cp)
        wcat = torch.cat([pm.bbox_layer.weight, pm.mask_layer.weight, cw], 0)
        bcat = torch.cat([pm.bbox_layer.bias, pm.mask_layer.bias, cb], 0)
        hp = pm.bbox_layer
        head_pk = Packed(wcat, bcat, None, hp.stride[0], hp.padding[0], None, dev)
        head_pk.cout_alg = A * (4 + D + Ccls)
        coef_act = {'tanh': L.ACT_TANH, 'sigmoid': L.ACT_SIGMOID, 'relu': L.ACT_RELU, 'none': L.ACT_NONE}[
            act_name(cfg.mask_proto_coeff_activation)]
        n_b, n_c, n_m = A * 4, A * Cp, A * D
        offs = [sum(cells[:l]) * A for l in range(nlev)]
        bbc = cfg.backbone
        pri = []
        for lvl, (fh, fw) in enumerate(shapes):
            pri += make_priors_host(fh, fw, bbc.pred_scales[lvl], bbc.pred_aspect_ratios[lvl], cfg.max_size, bbc)

        # head0.upfeature and proto_net[0] are both 3x3 / pad 1 / 256 -> 256 + ReLU convolutions of the SAME tensor (P3): one
        # launch with their filters concatenated along Cout shares the input tile (direct kernel) or the whole Winograd input
        # transform V (one transform instead of two, one 512-column GEMM), and scatters to two dense outputs
        pmods = list(net.proto_net)
        up_convs = [m for m in pm.upfeature if isinstance(m, nn.Conv2d)] if hasattr(pm, 'upfeature') else []
        self._merged_p3 = None
        merge_p3 = (os.environ.get('YOLACT_AMD_MERGE_P3', '1') == '1' and len(up_convs) == 1 and len(pmods) > 2
                    and isinstance(pmods[0], nn.Conv2d) and isinstance(pmods[1], nn.ReLU)
                    and all(c.kernel_size == (3, 3) and c.padding == (1, 1) and c.stride == (1, 1) and c.bias is not None
                            for c in (up_convs[0], pmods[0]))
                    and up_convs[0].in_channels == pmods[0].in_channels and up_convs[0].out_channels % 4 == 0
                    and pmods[0].out_channels % 4 == 0)

        def head(lvl, f):
            off = offs[lvl]
            u = f
            if lvl == 0 and merge_p3:
                cu, cp = up_convs[0], pmods[0]
                u = self._new(f.B, f.H, f.W, cu.out_channels)
                t0 = self._new(f.B, f.H, f.W, cp.out_channels)
                pkm = Packed(torch.cat([cu.weight, cp.weight], 0), torch.cat([cu.bias, cp.bias], 0), None, 1, 1, None, dev)
                if getattr(self, '_proto0_down', None) is not None:      # (the proto_net[0] half of the merged launch: _rebalance_outliers)
                    pkm.scale_out_channels(torch.cat([torch.ones(cu.out_channels), self._proto0_down]))
                hw = f.H * f.W
                self.conv('head0.up0+proto.0', f, pkm, segs=[
                    (0, cu.out_channels, L.ACT_RELU, cu.out_channels, hw * cu.out_channels, u.ptr),
                    (cu.out_channels, cu.out_channels + cp.out_channels, L.ACT_RELU, cp.out_channels, hw * cp.out_channels,
                     t0.ptr)])
                # one bound PER HALF (segment k raises slot k of consecutive slots): the two halves are different tensors — a large
                # proto_net[0] channel must not coarsen the fp16x2 scale of the head's input (round-4 outlier stress test)
                u.slot, t0.slot = self.last_yslot, self.last_yslot + 1
                u.gain, t0.gain = self.last_out_gain[:cu.out_channels], self.last_out_gain[cu.out_channels:]
                self._merged_p3 = t0
            else:
                for k, pk in enumerate(up_pk):
                    nu = self.conv('head%d.up%d' % (lvl, k), u, pk, act=L.ACT_RELU)
                    if u is not f:
                        self.free(u)
                    u = nu
                    lev_ops.setdefault(lvl, [f]).append(len(self.ops) - 1)
            segs = [
                (0, n_b, L.ACT_NONE, n_b, P * 4, self.loc.data_ptr() + off * 4 * 4),
                (n_b, n_b + n_m, coef_act, n_m, P * D, self.coef.data_ptr() + off * D * 4),
                (n_b + n_m, n_b + n_m + n_c, L.ACT_NONE, n_c, P * Cp, self.conf.data_ptr() + off * Cp * 4),
            ]
            self.conv('head%d.out' % lvl, u, head_pk, segs=segs)
            lev_ops.setdefault(lvl, [f]).append(len(self.ops) - 1)
            if u is not f:
                self.free(u)

        lev_ops = {}       # level -> [input, op index of every up-feature conv ..., op index of the .out conv] (_build_level_merge)

        def pred(j):   # pred_layers are stored top-down: index n-1-j belongs to level j (yolact.py:286-289)
            i = n - 1 - j
            return self.conv('fpn.pred%d' % i, sums[j], pack_module(fpn.pred_layers[i], device=dev), act=L.ACT_RELU)

        assert net.proto_src == 0, 'prototypes are taken from P3 in every shipped config'
        # ---- fork: the P3 branch (75 % of the remaining FLOPs) stays on A, P4..P7 + Detect go to the side stream B
        self.record('fork')
        self.on('B')
        self.wait('fork')
        self.on('A')
        p3 = pred(0)
        self.free(sums[0])
        self.on('B')
        feats_b = [pred(j) for j in range(1, n)]
        for j in range(1, n):
            self.free(sums[j])
        for i, m in enumerate(fpn.downsample_layers):
            feats_b.append(self.conv('fpn.down%d' % i, feats_b[-1], pack_module(m, device=dev)))
        # the P3 head stays on A (moving it to B as well measured 862 vs 877 images/s)
        self.on('A')
        head(0, p3)
        self.record('head0')
        self.on('B')
        for lvl in range(1, nlev):
            head(lvl, feats_b[lvl - 1])
        self._build_level_merge(lev_ops, up_pk, head_pk, offs, (4, D, Cp), (n_b, n_m, n_c), coef_act)
        self.wait('head0')
        for f in feats_b:
            self.free(f)
        self.ops.append(('detect', None, 'detect', self._cur))
        self.record('b_done')
        self.on('A')

        # protonet (utils/functions.py:163-213 + yolact.py:588-599) on A; the last conv writes the per-call proto tensor
        t = p3
        mods = list(net.proto_net)
        conv_idx = [i for i, m in enumerate(mods) if isinstance(m, nn.Conv2d)]
        self.proto_patch = None
        self.proto_patch_wino = None     # the F(4x4) descriptor that writes the proto tensor when the last 1x1 is fused into it (wino_proj)
        self.wino_proj = None            # (op index of the 3x3 before the last 1x1, op index of that 1x1): see _tune_winograd
        prev_conv_op = None
        held = None      # low-res source of a fusable 2x upsampling: the consuming conv's F(4x4) input transform may read IT instead
                         # of the upsampled tensor (ymi_wino_desc.x_up), so its buffer stays allocated until that conv's output
                         # has been allocated — freed earlier, the best-fit arena could hand it to the conv's own output
        for i, m in enumerate(mods):
            if i == 0 and self._merged_p3 is not None:      # proto.0 was computed together with head0.up0
                self.free(t)
                t = self._merged_p3
                continue
            if isinstance(m, nn.Conv2d):
                last = i == conv_idx[-1]
                has_relu = (i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU))
                if last:
                    a = {'relu': L.ACT_RELU, 'none': L.ACT_NONE, 'sigmoid': L.ACT_SIGMOID, 'tanh': L.ACT_TANH}[
                        act_name(cfg.mask_proto_prototype_activation)]
                    assert not has_relu
                else:
                    a = L.ACT_RELU if has_relu else L.ACT_NONE
                pk = self._pack(m)
                if last:
                    Ho, Wo = out_size(t.H, pk.kh, pk.stride, pk.pad), out_size(t.W, pk.kw, pk.stride, pk.pad)
                    self.proto_shape = (B, Ho, Wo, pk.Cout)
                    self.conv('proto.%d' % i, t, pk, segs=[(0, pk.Cout, a, pk.Cout, Ho * Wo * pk.Cout, None)])
                    self.proto_patch = self.ops[-1][1].contents  # seg[0].ptr set per call
                    nt = None
                    # conv3x3(256 -> 256) + ReLU -> conv1x1(256 -> <= 32): when the 3x3 runs as F(4x4,3x3) its output transform can
                    # multiply each tile by the 1x1's filters and write the prototypes directly (ymi_wino_desc.proj_*)
                    if (self.h2 and prev_conv_op is not None and prev_conv_op in self.wino_alt and (pk.kh, pk.kw, pk.stride, pk.pad) == (1, 1, 1, 0)
                            and pk.Cin == 256 and pk.Cout <= 32 and pk.Cout % 4 == 0 and a <= L.ACT_LEAKY01 and not getattr(pk, 'wide', False)
                            and os.environ.get('YOLACT_AMD_WINO_PROJ', '1') == '1'):
                        self.wino_proj = (prev_conv_op, len(self.ops) - 1)
                else:
                    nt = self.conv('proto.%d' % i, t, pk, act=a)
                    prev_conv_op = len(self.ops) - 1
                self.free(t)
                if held is not None:
                    self.free(held)
                    held = None
                t = nt
            elif isinstance(m, M.InterpolateModule):
                prev_conv_op = None
                s = int(m.scale_factor)
                has_relu = (i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU))
                y = self._new(t.B, t.H * s, t.W * s, t.C, slot=t.slot, gain=t.gain)   # convex interpolation: the input's bound (and gain) holds
                self.call(lib.ymi_bilinear_nhwc_f32, t.ptr, y.ptr, t.B, t.H, t.W, t.C, y.H, y.W,
                          C.c_float(1.0 / s), C.c_float(1.0 / s), 1 if has_relu else 0, name='proto.interp')
                if s == 2 and os.environ.get('YOLACT_AMD_FUSED_UPSAMPLE', '1') == '1':
                    # (the tuner drops this launch when the consuming conv runs as F(4x4,3x3): csrc/winograd.hip UPS)
                    self._upsrc[id(y)] = (len(self.ops) - 1, t.ptr, 1 if has_relu else 0)
                    held = t
                else:
                    self.free(t)
                t = y
        assert self.proto_patch is not None and held is None
        self.wait('b_done')
        self.priors = torch.tensor(pri, dtype=torch.float32).view(-1, 4).to(dev)
        assert self.priors.shape[0] == P

    def _resnet(self, bb: M.ResNetBackbone, x4: T):
        dev, ar, lib = self.device, self.arena, self.lib
        pk0 = pack_module(bb.conv1, bb.bn1, dev, cin_pad=4)
        if self.fused_stem:
            B, H, W = self.B, self.H, self.W
            Hs, Ws = out_size(H, 7, 2, 3), out_size(W, 7, 2, 3)
            Hp, Wp = out_size(Hs, 3, 2, 1), out_size(Ws, 3, 2, 1)
            x = self._new(B, Hp, Wp, 64, slot=self._slot(), gain=pk0.out_gain())
            planes, sc2, winv = pk0.h2()
            sd = L.StemDesc()
            sd.y, sd.B, sd.H, sd.W, sd.cout_pad, sd.kpad = x.ptr, B, H, W, pk0.CoutPad, pk0.Kpad
            sd.w_h2, sd.scale_h2, sd.bias, sd.y_amax = planes.data_ptr(), sc2.data_ptr(), pk0.bias.data_ptr(), self._slot_ptr(x.slot)
            self.keepalive.append(pk0)
            md = L.ConvDesc()          # accounting only (FLOPs of the 7x7 conv; bench.py takes the bytes of the fused launch)
            md.B, md.H, md.W, md.Cin, md.ldx, md.Ho, md.Wo, md.Cout = B, H, W, 4, 4, Hs, Ws, 64
            md.kh, md.kw, md.stride, md.pad, md.Kpad, md.cin_alg, md.cout_alg = 7, 7, 2, 3, pk0.Kpad, 3, 64
            self.conv_meta.append(('stem', md))
            self.ops.append(('stem', sd, 'stem+maxpool', 'A'))
            self._stem_desc = sd
        else:
            stem = self.conv('stem', x4, pk0, act=L.ACT_RELU)
            ar.free(x4)
            Hp, Wp = out_size(stem.H, 3, 2, 1), out_size(stem.W, 3, 2, 1)
            x = self._new(stem.B, Hp, Wp, stem.C, slot=stem.slot, gain=stem.gain)        # max-pooling cannot raise the magnitude bound
            self.call(lib.ymi_maxpool3x3s2_nhwc_f32, stem.ptr, x.ptr, stem.B, stem.H, stem.W, stem.C, Hp, Wp, name='maxpool')
            ar.free(stem)
        outs = []
        self._stage_out_ptr = {}
        held = []        # buffers of a stage's last block kept until the next block's conv1 output is allocated (see below)
        for li, layer in enumerate(bb.layers):
            for bi, blk in enumerate(layer):
                nm = 'layer%d.%d' % (li, bi)
                side_down = blk.downsample is not None and self.two_streams and self.down_on_side_stream
                if side_down:
                    # the projection shortcut only depends on the block input: run it on the side stream while A does
                    # conv1 / conv2 (fills their tails); A picks it up before conv3
                    self.record(nm + '.in')
                    self.on('B')
                    self.wait(nm + '.in')
                    res = self.conv(nm + '.down', x, self._pack(blk.downsample[0], blk.downsample[1]))
                    self.record(nm + '.down')
                    self.on('A')
                o1 = self.conv(nm + '.conv1', x, self._pack(blk.conv1, blk.bn1), act=L.ACT_RELU)
                for t in held:
                    ar.free(t)
                held = []
                if blk.use_dcn:
                    dcn = blk.conv2
                    om = self.conv(nm + '.offmask', o1, pack_offmask(dcn.conv_offset_mask, dev, self.om_interleave) if self.om_pad
                                   else pack_module(dcn.conv_offset_mask, None, dev))
                    pk = Packed(dcn.weight, dcn.bias, blk.bn2, dcn.stride[0], 1, None, dev)     # (stride is a pair, dcn_v2.py:62)
                    o2 = self.conv(nm + '.dcn', o1, pk, act=L.ACT_RELU, dcn_offmask=om)
                    ar.free(om)
                else:
                    o2 = self.conv(nm + '.conv2', o1, pack_module(blk.conv2, blk.bn2, dev), act=L.ACT_RELU)
                ar.free(o1)
                if side_down:
                    self.wait(nm + '.down')
                elif blk.downsample is not None:
                    res = self.conv(nm + '.down', x, self._pack(blk.downsample[0], blk.downsample[1]))
                else:
                    res = x
                y = self.conv(nm + '.conv3', o2, self._pack(blk.conv3, blk.bn3), act=L.ACT_RELU, res=res,
                              res_mode=L.RES_ADD)
                # the exit of a 64-plane stage may become ONE launch with the next stage's conv1 (_fuse_stage_exit), which then
                # writes that conv1's output while it still reads o2 and the residual: the best-fit arena must not hand conv1 a
                # buffer that contains either, so both stay allocated until conv1's output exists.  UNCONDITIONAL on purpose (also
                # with YOLACT_AMD_CHAIN_EXIT=0 or a table decision of 0, where it only keeps two buffers alive a little longer): the
                # buffer layout of a plan must not depend on a table lookup or a switch that is read after the plan is built
                hold = (self.h2 and bi == len(layer) - 1 and li + 1 < len(bb.layers) and blk.downsample is None
                        and o2.C == 64 and y.C == 256)
                if hold:
                    held = [o2, x]
                else:
                    ar.free(o2)
                if side_down:
                    self.on('B')          # back to the side stream's pool: its next op waits for a later event of A
                    self.free(res)
                    self.on('A')
                elif res is not x:
                    ar.free(res)
                if not hold:
                    ar.free(x)
                x = y
                if bi == 0:                     # behind this stage's projection shortcut on B: the previous stages' FPN laterals
                    self._flush_early_laterals()
            # stage output: still needed by the FPN, so the next stage only borrows it
            outs.append(x)
            self._stage_out_ptr[li] = x.ptr
            self._stage_done(li, x)
            x = _Borrowed(x)
        for t in held:
            ar.free(t)
        return outs

    def _darknet(self, bb: M.DarkNetBackbone, x4: T):
        dev, ar = self.device, self.arena

        def unit(name, t, seq, cin_pad=None, res=None):
            pk = pack_module(seq[0], seq[1], dev, cin_pad=cin_pad)
            if res is None:
                return self.conv(name, t, pk, act=L.ACT_LEAKY01)
            return self.conv(name, t, pk, act=L.ACT_LEAKY01, res=res, res_mode=L.RES_ADD, res_after_act=1)

        x = unit('preconv', x4, bb._preconv, cin_pad=4)
        ar.free(x4)
        outs = []
        for li, layer in enumerate(bb.layers):
            mods = list(layer)
            y = unit('dark%d.down' % li, x, mods[0])
            ar.free(x)
            x = y
            for bi, blk in enumerate(mods[1:]):
                a = unit('dark%d.%d.conv1' % (li, bi), x, blk.conv1)
                y = unit('dark%d.%d.conv2' % (li, bi), a, blk.conv2, res=x)
                ar.free(a)
                ar.free(x)
                x = y
                if bi == 0:
                    self._flush_early_laterals()
            outs.append(x)
            self._stage_done(li, x)
            x = _Borrowed(x)
        return outs

    # ---- execution -------------------------------------------------------------------------------
    @staticmethod
    def section_of(name):
        """The reference's timer section an op belongs to (yolact.py:570 'backbone', :574 'fpn', :581 'proto',
        :607 'pred_heads'); 'Detect' (detection.py:63) is timed by Detect.finish."""
        if name.startswith('fpn.'):
            return 'fpn'
        if name.startswith('proto.'):
            return 'proto'
        if name.startswith('head'):
            return 'pred_heads'
        return 'backbone'

    def mark_done(self):
        """Record, on the caller's current stream, that everything reading this plan's persistent buffers has been
        enqueued; the next run() — possibly on another stream — waits for it."""
        if self.device.type == 'cuda' and not torch.cuda.is_current_stream_capturing():
            if self._done_event is None:
                self._done_event = torch.cuda.Event()
            self._done_event.record(torch.cuda.current_stream(self.device))

    def run(self, x: torch.Tensor, detect=None, timer=None, skip_proto=False):
        """x [B,3,H,W] fp32 contiguous on the plan's device. Returns (proto, detect_result): the fresh proto tensor
        and whatever `detect(stream_ptr)` returned (None without a callback).  loc/conf/coef are the plan's persistent
        head buffers.  `detect` is invoked at the point of the op list where every head has been written; its
        kernels must be launched on the stream it is handed (the side stream in two-stream mode) while its output
        tensors are allocated by the caller's ambient stream — they are only consumed after the final join.
        `timer`: the reference's utils.timer module (or None): the op ranges are bracketed with its section names.
        The arena, the head buffers and the Winograd workspaces are shared by every run of this plan: callers serialise
        run() on the host (Yolact._run_lock_for(device)) and consecutive runs are ordered on the device by an event, so two user
        streams cannot overlap on the same buffers."""
        lib = self.lib
        cur = torch.cuda.current_stream(self.device)
        capturing = torch.cuda.is_current_stream_capturing()
        if self._done_event is not None and not capturing:
            cur.wait_event(self._done_event)
        sa = C.c_void_p(cur.cuda_stream)
        two = self.two_streams and self.overlap
        sb = C.c_void_p(self.stream_b.cuda_stream) if two else sa
        # skip_proto: cfg.eval_mask_branch is False at call time (eval.py --detect, eval.py:1067-1068): the reference computes no
        # prototypes (yolact.py:579-580) — the protonet's launches are left out of the op loop and None is returned for them
        proto = None
        if not skip_proto:
            proto = torch.empty(self.proto_shape, dtype=torch.float32, device=self.device)
            self.proto_patch.seg[0].ptr = proto.data_ptr()
            if self.proto_patch_wino is not None:
                self.proto_patch_wino.proj_y = proto.data_ptr()
        # only a module with the reference's timer API (utils/timer.py: start / stop / env) is driven
        if timer is not None and not all(hasattr(timer, a) for a in ('start', 'stop', 'env')):
            timer = None
        if timer is None and self.native_exec:
            nat = self._native_plan()
            if nat is not None:          # the whole op list in two native calls (csrc/plan_exec.cpp) around the Detect callback
                det = self._run_native(nat, x, sa, sb, two, detect, skip_proto)
                self.mark_done()
                return proto, det
        if self.h2:                  # magnitude bounds are re-derived by every run (on the caller's stream, ahead of every op)
            self.amax[:self._nslots * L.AMAX_SLOT_FLOATS].zero_()
        self._sec = None
        try:
            det = self._dispatch(x, cur, sa, sb, two, detect, timer, skip_proto)
        finally:
            if timer is not None and self._sec is not None:   # a failed launch must not leave a reference timer running
                timer.stop(self._sec)
        self.mark_done()
        return proto, det

    # ---- native executor (csrc/plan_exec.cpp, ABI 7) ------------------------------------------------------------------------------
    _SEC_ID = {'backbone': L.SEC_BACKBONE, 'fpn': L.SEC_FPN, 'proto': L.SEC_PROTO, 'pred_heads': L.SEC_HEADS}

    def _native_plan(self):
        """The op list as a ymi_plan_op array (rebuilt whenever an op was replaced: tuner, set_winograd), the index of the Detect
        marker, the event handles and the index of the input-layout op.  None when the list holds a call the executor does not know
        (the Python loop then runs it)."""
        key = (self.ops.version, len(self.ops)) if isinstance(self.ops, _OpList) else tuple(map(id, self.ops))
        if self._native is not None and self._native[0] == key:
            return self._native[1]
        lib = self.lib
        n = len(self.ops)
        arr = (L.PlanOp * (n + 1))()
        arr[0].kind, arr[0].stream = L.OP_MEMSET, 0
        arr[0].p[0], arr[0].i[0] = self.amax.data_ptr(), 4 * self._nslots * L.AMAX_SLOT_FLOATS
        ev_index, det_idx, in_idx, ok = {}, None, None, True
        by_fn = {id(lib.ymi_conv2d_nhwc_f32): L.OP_CONV, id(lib.ymi_conv3x3_winograd_f32): L.OP_WINO,
                 id(lib.ymi_dcn_v2_forward_f32): L.OP_DCN, id(lib.ymi_pointwise_chain_f32): L.OP_CHAIN,
                 id(lib.ymi_stage_exit_chain_f32): L.OP_STAGE_EXIT}
        for k, (fn, args, name, where) in enumerate(self.ops):
            o = arr[k + 1]
            o.stream = 1 if where == 'B' else 0
            o.section = self._SEC_ID.get(self.sections[k], 0) if self.sections[k] else 0
            if fn == 'input':
                a = self.in_args
                o.kind, in_idx = L.OP_INPUT, k + 1
                o.p[1] = a[1]
                o.p[2] = self.in_amax[2] if self.h2 else None
                o.i[0], o.i[1], o.i[2], o.i[3] = a[2], a[3], a[4], a[5]
            elif fn == 'stem':
                o.kind, o.desc = L.OP_STEM, C.addressof(args)
            elif fn == 'nop':
                o.kind = L.OP_NOP
            elif fn in ('record', 'wait'):
                o.kind = L.OP_RECORD if fn == 'record' else L.OP_WAIT
                o.i[0] = ev_index.setdefault(args, len(ev_index))
            elif fn == 'detect':
                o.kind, det_idx = L.OP_NOP, k + 1
            elif id(fn) in by_fn:
                o.kind, o.desc = by_fn[id(fn)], C.addressof(args.contents)
            elif fn is lib.ymi_bilinear_nhwc_f32:
                o.kind = L.OP_BILINEAR
                o.p[0], o.p[1] = args[0], args[1]
                for q in range(6):
                    o.i[q] = args[2 + q]
                o.f[0], o.f[1], o.i[6] = args[8].value, args[9].value, args[10]
            elif fn is lib.ymi_maxpool3x3s2_nhwc_f32:
                o.kind = L.OP_MAXPOOL
                o.p[0], o.p[1] = args[0], args[1]
                for q in range(6):
                    o.i[q] = args[2 + q]
            elif fn is lib.ymi_bilinear_add_nhwc_f32:
                o.kind = L.OP_BILINEAR_ADD
                o.p[0], o.p[1], o.p[2] = args[0], args[1], args[8]
                for q in range(6):
                    o.i[q] = args[2 + q]
            else:
                ok = False
                break
        if not ok or det_idx is None:
            self._native = (key, None)
            return None
        if self._native_events is None or len(self._native_events) < len(ev_index):
            for h in (self._native_events or ()):       # regrown: the old handles are destroyed, not leaked
                if h:
                    lib.ymi_event_destroy(C.c_void_p(h))
            evs = (C.c_void_p * max(len(ev_index), 1))()
            for q in range(len(ev_index)):
                h = C.c_void_p()
                L.check(lib.ymi_event_create(C.byref(h)), 'ymi_event_create')
                evs[q] = h.value
            self._native_events = evs
        nat = (arr, det_idx, self._native_events, in_idx, n + 1)
        self._native = (key, nat)
        return nat

    def _run_native(self, nat, x, sa, sb, two, detect, skip_proto):
        arr, det_idx, evs, in_idx, n = nat
        lib = self.lib
        if in_idx is not None:
            arr[in_idx].p[0] = x.data_ptr()
        if self._stem_desc is not None:
            self._stem_desc.x = x.data_ptr()
        skip = (1 << L.SEC_PROTO) if skip_proto else 0
        failed = C.c_int32(-1)
        ov = 1 if two else 0

        def go(first, last):
            rc = lib.ymi_plan_run(arr, first, last, sa, sb, evs, ov, skip, C.byref(failed))
            if rc != 0:
                L.check(rc, self.ops[failed.value - 1][2] if failed.value > 0 else 'plan op')
        go(0 if self.h2 else 1, det_idx)
        det = None
        if detect is not None:
            det = detect(sb if self.ops[det_idx - 1][3] == 'B' else sa)
        go(det_idx + 1, n)
        return det

    def __del__(self):
        try:
            if getattr(self, '_native_events', None) is not None:
                for h in self._native_events:
                    if h:
                        self.lib.ymi_event_destroy(h)
        except Exception:
            pass

    def _dispatch(self, x, cur, sa, sb, two, detect, timer, skip_proto=False):
        """The flat op loop of run(): C-ABI launches on the two streams, event records / waits, the Detect callback."""
        lib = self.lib
        det = None
        for (fn, args, name, where), nsec in zip(self.ops, self.sections):
            s = sb if where == 'B' else sa
            if timer is not None and nsec is not None and nsec != self._sec:
                if self._sec is not None:
                    timer.stop(self._sec)
                timer.start(nsec)
                self._sec = nsec
                if nsec == 'pred_heads' and not self._priors_timed:
                    with timer.env('makepriors'):       # yolact.py:219: priors are host constants of the plan, built once
                        self._priors_timed = True
            if fn == 'input':
                a = self.in_args
                if self.h2:          # layout change + magnitude bound of the input in one launch
                    rc = lib.ymi_nchw_to_nhwc4_amax_f32(x.data_ptr(), a[1], a[2], a[3], a[4], a[5], self.in_amax[2], s)
                else:
                    rc = lib.ymi_nchw_to_nhwc4_f32(x.data_ptr(), a[1], a[2], a[3], a[4], a[5], s)
            elif fn == 'nop' or (skip_proto and nsec == 'proto'):
                continue
            elif fn == 'stem':
                args.x = x.data_ptr()
                rc = lib.ymi_stem_pool_f32(C.byref(args), s)
            elif fn == 'record':
                if two:
                    self.events[args].record(self.stream_b if where == 'B' else cur)
                continue
            elif fn == 'wait':
                if two:
                    (self.stream_b if where == 'B' else cur).wait_event(self.events[args])
                continue
            elif fn == 'detect':
                if detect is not None:
                    det = detect(s)
                continue
            elif isinstance(args, tuple):
                rc = fn(*args, s)
            else:
                rc = fn(args, s)
            if rc != 0:
                L.check(rc, name)
        return det

    def conv_flops(self):
        return sum(self.lib.ymi_conv_flops(C.byref(d)) for _, d in self.conv_meta)


class _Borrowed(T):
    """A stage output that is still needed later (FPN input): the consuming block must not free it."""
    __slots__ = ()

    def __init__(self, t: T):
        super().__init__(t.buf, t.B, t.H, t.W, t.C, t.slot, t.gain)
