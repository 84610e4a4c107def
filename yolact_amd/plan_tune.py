"""Tile / algorithm selection of an execution plan: `PlanTuning`, the mixin engine.Plan inherits its tuner from.

Plan.tune() installs, per launch, what the shipped table (tune_table.py) says, and measures what the table does not know: the
candidates of every direct convolution, direct against Winograd per 3x3 layer, and the chain / stage-exit fusions of the first
ResNet stage.  Everything here works on the plan's op list and descriptors through `self`; engine.py is never imported.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _lib as L
from . import tune_table as TT


def _ceil(a, b):
    return (a + b - 1) // b * b


def _desc_pointers(d):
    """Every non-NULL pointer a ctypes descriptor holds, nested structures and arrays included (Plan.stage_exit_candidates: who else
    names a buffer).  Walks `_fields_`, so it does not depend on what a pointer field is called."""
    out = []
    if isinstance(d, C.Array):
        for e in d:
            out += _desc_pointers(e) if isinstance(e, (C.Structure, C.Array)) else ([int(e)] if isinstance(e, int) and e else [])
        return out
    for f in d._fields_:
        name, typ = f[0], f[1]
        v = getattr(d, name)
        if typ is C.c_void_p:
            if v:
                out.append(int(v))
        elif isinstance(v, (C.Structure, C.Array)) and (issubclass(typ, C.Structure) or issubclass(getattr(typ, '_type_', int), (C.Structure, C.c_void_p))):
            out += _desc_pointers(v)
    return out


def _split_k_ids(tid, blocks, nk, Cout):
    """Direct choices (tid, S) for the chunk-aligned K splits S worth measuring on a grid of `blocks` blocks that alone leaves CUs idle:
    ranges of at least 4 chunks, none empty, 128 .. 1100 blocks in all."""
    out = []
    if blocks < 400 and Cout % 4 == 0:
        for S in (2, 3, 4, 5, 6, 8, 9, 12, 16):
            per = -(-nk // S)                             # chunks per range (the last range may be shorter, never empty)
            if per >= 4 and per * (S - 1) < nk and 128 <= blocks * S <= 1100:
                out.append(TT.direct_choice(tid, S))
    return out


def _timed(run, e0, e1, reps):
    """ms per call of run(): warmed once, then the better of two rounds of `reps` calls between the HIP events e0 / e1."""
    run()
    best = 1e30
    for _ in range(2):
        e0.record()
        for _ in range(reps):
            run()
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1) / reps)
    return best


def _rows_overlap(M, a, lda, b, ldb):
    """Do M rows of fp32 at `a` (row stride lda) and M rows at `b` (row stride ldb) share an address?"""
    a, b = int(a or 0), int(b or 0)
    return a < b + 4 * M * int(ldb) and b < a + 4 * M * int(lda)


def _fill_chain(cd, d3, d1=None):
    """The ymi_chain_desc fields of conv3 (d3: 1x1, + shortcut, activation) and, if given, of the 1x1 conv1 that reads its output (d1)."""
    cd.x, cd.res, cd.y = d3.x, d3.res, d3.seg[0].ptr
    cd.w_a_h2, cd.scale_a_h2, cd.bias_a = d3.w_h2, d3.scale_h2, d3.bias
    cd.x_amax, cd.y_amax = d3.x_amax, d3.y_amax
    cd.M, cd.ldx, cd.res_ld, cd.ldy = d3.B * d3.Ho * d3.Wo, d3.ldx, d3.res_ld, d3.seg[0].row_stride
    cd.k_a, cd.n_a, cd.n_b = d3.Cin, d3.Cout, d1.Cout if d1 is not None else d3.Cin
    cd.cout_pad_a, cd.cout_pad_b = _ceil(cd.n_a, 128), _ceil(cd.n_b, 128)
    cd.act_a = d3.seg[0].act
    if d1 is not None:
        cd.z, cd.ldz, cd.z_amax, cd.act_b = d1.seg[0].ptr, d1.seg[0].row_stride, d1.y_amax, d1.seg[0].act
        cd.w_b_h2, cd.scale_b_h2, cd.bias_b = d1.w_h2, d1.scale_h2, d1.bias
    return cd


def _set_wino_choice(wd, v):
    """Install a Winograd choice of the table (GEMM tile, V planes) in a ymi_wino_desc."""
    wd.tile, wd.v_planes = TT.wino_parts(v)


class PlanTuning:
    # ---- tile / algorithm selection ------------------------------------------------------------------
    def tune(self, x: torch.Tensor, reps: int = 3):
        """Pick the tile of every conv launch and direct-vs-Winograd per 3x3 layer.

        Deterministic by default: the choices come from the SHIPPED table `yolact_amd/tune/gfx950.json` (measured on
        MI355X by tools/make_tune_table.py, keyed by layer shape), so two processes on two boxes run the same kernels
        in the same summation order and produce the same bits.  A shape the table does not know is measured on the
        device (HIP events on the launch stream, `self.tune_misses` counts them); such a plan is only reproducible
        within its process unless YOLACT_AMD_TUNE_CACHE names a file to persist the new entries in.

        YOLACT_AMD_AUTOTUNE: '1' (default) table + measure on miss | '0' no tuning at all (library heuristic tiles,
        direct kernels only) | 'table' table only, a miss falls back to the heuristic | 'force' ignore the tables and
        measure everything (what tools/make_tune_table.py uses)."""
        mode = os.environ.get('YOLACT_AMD_AUTOTUNE', '1')
        self.tune_table, self.wino_table, self.tune_misses = [], [], 0
        if mode == '0':
            return []
        cache_path = os.environ.get('YOLACT_AMD_TUNE_CACHE')
        disk = {}
        if mode != 'force':
            disk.update(TT.load_tune_table(self.device))
            if cache_path and os.path.exists(cache_path):
                disk.update(TT.read_table_file(cache_path))
        n0 = len(disk)
        self.run(x)                      # realistic values in every buffer
        s = L.stream_ptr()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        measure = mode != 'table'
        self._tune_direct(e0, e1, s, reps, disk, measure)
        self._tune_winograd(e0, e1, s, reps, disk, measure)
        self._merge_levels(e0, e1, s, reps, disk, measure)
        self._fuse_pointwise_chains(e0, e1, s, reps, disk, measure)
        torch.cuda.synchronize(self.device)
        if cache_path and (len(disk) != n0 or mode == 'force'):
            TT.write_table_file(cache_path, disk, self.device)
        self.tune_entries = disk
        return self.tune_table

    def _splitk_ws(self, where, numel):
        """Per-stream workspace of the split-K partial sums (grown on demand; every layer of a stream shares it)."""
        ws = self._sk_ws.get(where)
        if ws is None or ws.numel() < numel:
            ws = self._sk_ws[where] = torch.empty(numel, dtype=torch.float32, device=self.device)
            for fn, dptr, _n, w in self.ops:          # re-point descriptors that already use the old buffer
                if fn is self.lib.ymi_conv2d_nhwc_f32 and w == where and dptr.contents.split_k > 1:
                    dptr.contents.split_ws = ws.data_ptr()
                elif fn is self.lib.ymi_dcn_v2_forward_f32 and w == where and dptr.contents.conv.split_k > 1:
                    dptr.contents.conv.split_ws = ws.data_ptr()
        return ws

    @staticmethod
    def _splitk_ok(d):
        """Shapes the split-K path takes (csrc/conv_igemm.hip run_splitk): small-map 1x1 convolutions with a long K."""
        return (d.kh == 1 and d.kw == 1 and d.pad == 0 and d.Cin == d.Kpad and d.Cin % 32 == 0 and d.nseg == 1
                and d.Cout % 4 == 0 and d.seg[0].act <= L.ACT_LEAKY01 and d.res_mode in (L.RES_NONE, L.RES_ADD)
                and d.B * d.Ho * d.Wo <= 16384 and d.Kpad >= 256)

    def _fuse_pointwise_chains(self, e0, e1, s, reps, disk, measure):
        """conv3 (1x1, 64 -> 256, + shortcut, ReLU) of a first-stage bottleneck directly followed by conv1 (1x1, 256 -> 64, ReLU) of
        the next one -> ONE ymi_pointwise_chain_f32 launch (csrc/chain.hip: the 256-channel tensor is written once and never read
        back); a conv3 of that shape WITHOUT such a successor (the last block of the stage) -> the same streaming kernel with its
        second layer switched off.  Either only where measured faster than the launches it replaces: the decision is a table entry
        like every other choice ('chain(B, H, W)' / 'chain1(B, H, W)': [1 | 0, ms of the plan's launches, ms of the chain launch]);
        YOLACT_AMD_CHAIN=0 keeps the plan's launches (and those of the stage exit, _fuse_stage_exit, which is tried first).
        A pair that is installed and whose residual is a projection shortcut nothing else reads (entry_chain_candidates: layer0.0)
        may also COMPUTE that shortcut in the launch (the ENTRY form: the 256-channel shortcut tensor is neither written nor read
        back); decided the same way, table entry 'chain(B, H, W, 64)': [1 | 0, ms of the shortcut on its table tile + the pair
        launch, ms of the entry launch].  YOLACT_AMD_CHAIN_ENTRY = 1 (default) | 0 | force (install it whatever the table says)."""
        self.chain_table, self.chainx_table, self.chaine_table = [], [], []
        if not self.h2 or os.environ.get('YOLACT_AMD_CHAIN', '1') != '1':
            return
        lib = self.lib

        def timed(run):
            return _timed(run, e0, e1, reps)
        entry_mode = os.environ.get('YOLACT_AMD_CHAIN_ENTRY', '1')
        # (on the op list as built: the stage exit below replaces launches, never moves them, so the indices hold)
        entry = {i3: idn for idn, i3, _ in self.entry_chain_candidates()} if entry_mode in ('1', 'force') else {}
        self._fuse_stage_exit(s, disk, measure, timed)       # (first: a 'chainx' decision of 1 takes the op before 'chain1' sees it)
        i = 0
        while i < len(self.ops):
            f3, p3, n3, w3 = self.ops[i]
            i += 1
            if f3 is not lib.ymi_conv2d_nhwc_f32 or (i - 1) in self.wide_ops:
                continue
            d3 = p3.contents
            M = d3.B * d3.Ho * d3.Wo
            P_ = d3.Cin
            if not ((d3.kh, d3.kw, d3.stride, d3.pad, d3.nseg) == (1, 1, 1, 0, 1) and P_ in (64, 128, 256) and d3.Cout == 4 * P_
                    and d3.res_mode == L.RES_ADD and not d3.res_after_act and d3.seg[0].n0 == 0 and d3.seg[0].act <= L.ACT_LEAKY01
                    and d3.w_h2 and d3.x_amax and M * max(d3.seg[0].row_stride, d3.res_ld) < (1 << 29)):
                continue
            if P_ > 64 and os.environ.get('YOLACT_AMD_CHAIN2', '0') not in ('1', 'force'):       # csrc/chain2.hip is OPT-IN: measured 0.80x of the two launches it replaces (profiles/r06_chain2_probe.txt)
                continue
            pair = False
            if i < len(self.ops) and self.ops[i][0] is lib.ymi_conv2d_nhwc_f32 and self.ops[i][3] == w3 and i not in self.wide_ops:
                d1 = self.ops[i][1].contents
                pair = ((d1.kh, d1.kw, d1.stride, d1.pad, d1.Cin, d1.Cout, d1.nseg) == (1, 1, 1, 0, 4 * P_, P_, 1)
                        and d1.res_mode == L.RES_NONE and d1.x == d3.seg[0].ptr and d1.ldx == d3.seg[0].row_stride
                        and d1.seg[0].n0 == 0 and d1.seg[0].act <= L.ACT_LEAKY01 and bool(d1.w_h2))
            if P_ > 64 and not pair:          # csrc/chain2.hip without its second layer has nothing over the pipelined tiles
                continue
            cd = _fill_chain(L.ChainDesc(), d3, d1 if pair else None)
            if P_ > 64:                       # the rigorous bound of y (include/yolact_amd.h, ABI 8)
                info = getattr(self, '_desc_info', {}).get(C.addressof(d3))
                if info is None or info[1] is None:
                    continue
                cd.gain_a, cd.bias_max_a = info[0].l1_gain()
                cd.res_amax = self._slot_ptr(info[1])
            name = n3
            if pair:
                f1, p1, n1, w1 = self.ops[i]
                name = n3 + '+' + n1
                # aliasing contract of ymi_pointwise_chain_f32 (include/yolact_amd.h): z must not overlap y or the residual, and may
                # alias the INPUT x only exactly in place (same base, same row stride): every block reads x tile T before it writes
                # z tile T and nobody else touches those rows.  The arena normally hands conv1's output the buffer conv3's input
                # just freed, which is that case; any other overlap (a z that landed in a buffer of another layout) is not fused.
                in_place = int(cd.z) == int(cd.x) and cd.ldz == cd.ldx
                if (_rows_overlap(M, cd.z, cd.ldz, cd.y, cd.ldy) or _rows_overlap(M, cd.z, cd.ldz, cd.res, cd.res_ld)
                        or (_rows_overlap(M, cd.z, cd.ldz, cd.x, cd.ldx) and not in_place)):
                    continue
            cptr = C.pointer(cd)
            key = TT.chain_key('chain' if pair else 'chain1', d3.B, d3.Ho, d3.Wo, P_ if P_ > 64 else None, self.mode)
            ent = disk.get(key)
            if P_ > 64 and os.environ.get('YOLACT_AMD_CHAIN2') == 'force':     # (A/B switch: install it whatever its isolated time says)
                ent = [1, 0.0, 0.0]
            if ent is None:
                self.tune_misses += 1
                if not measure or lib.ymi_pointwise_chain_f32(cptr, s) != 0:
                    continue
                t_plan = timed((lambda: (f3(p3, s), f1(p1, s))) if pair else (lambda: f3(p3, s)))
                t_one = timed(lambda: lib.ymi_pointwise_chain_f32(cptr, s))
                ent = disk[key] = [1 if t_one < 0.97 * t_plan else 0, round(t_plan, 4), round(t_one, 4)]
            self.chain_table.append((name, ent[0], ent[1], ent[2]))
            if ent[0] and lib.ymi_pointwise_chain_f32(cptr, s) == 0:
                self.keepalive.append(cd)
                self.ops[i - 1] = (lib.ymi_pointwise_chain_f32, cptr, name, w3)
                if pair:
                    self.ops[i] = ('nop', None, n1 + '[fused into ' + n3 + ']', w1)
                    i += 1
                    if P_ == 64 and (i - 2) in entry:
                        self._fuse_entry_shortcut(i - 2, entry[i - 2], cd, s, disk, measure, timed, entry_mode)

    def _fuse_entry_shortcut(self, ic, idn, cd, s, disk, measure, timed, mode):
        """The pair launch just installed at op `ic` (descriptor `cd`) -> its ENTRY form, with the projection shortcut of op `idn`
        computed inside (_fuse_pointwise_chains).  The chain op keeps its function and its name; the shortcut's op becomes a nop
        (its record / wait markers stay where they are)."""
        lib = self.lib
        fd, pd, nd, wd = self.ops[idn]
        ce = self._entry_chain_desc(cd, idn)
        if ce is None:
            return
        dd = pd.contents
        eptr, cptr = C.pointer(ce), C.pointer(cd)
        key = TT.chain_key('chain', dd.B, dd.Ho, dd.Wo, 64, self.mode)
        ent = disk.get(key)
        if mode == 'force':
            ent = [1, 0.0, 0.0]
        if ent is None:
            self.tune_misses += 1
            if not measure or lib.ymi_pointwise_chain_f32(eptr, s) != 0:
                return
            t_plan = timed(lambda: (fd(pd, s), lib.ymi_pointwise_chain_f32(cptr, s)))
            t_one = timed(lambda: lib.ymi_pointwise_chain_f32(eptr, s))
            ent = disk[key] = [1 if t_one < 0.97 * t_plan else 0, round(t_plan, 4), round(t_one, 4)]
        fc, _, nc, wc = self.ops[ic]
        self.chaine_table.append((nc, ent[0], ent[1], ent[2]))
        if ent[0] and lib.ymi_pointwise_chain_f32(eptr, s) == 0:
            self.keepalive.append(ce)
            self.ops[ic] = (fc, eptr, nc, wc)
            self.ops[idn] = ('nop', None, nd + '[fused into ' + nc.split('+')[0] + ']', wd)
            # profile records map onto conv_meta by position (kind 13 = conv3, kind 12 = the shortcut, kind 12 = conv1)
            names = [n for n, _ in self.conv_meta]
            n3 = nc.split('+')[0]
            if nd in names and n3 in names:
                m = self.conv_meta.pop(names.index(nd))
                self.conv_meta.insert([n for n, _ in self.conv_meta].index(n3) + 1, m)

    def stage_exit_candidates(self):
        """Op indices (conv3, conv1, [stride-2 readers]) of every stage exit ymi_stage_exit_chain_f32 can take (csrc/chain.hip,
        chain_h2_k<128>): a 1x1 64 -> 256 + RES_ADD conv3 whose next launch on the same stream tag is a 1x1 / stride-1 256 -> 128
        conv reading its output (so it has no 64-wide successor), whose every OTHER reader is a 1x1 stride-2 convolution — a
        quarter of the pixels: the launch stores only those rows — and whose output is not a backbone output the FPN selects.
        Pure shape logic on the op list (works on a dry CPU plan); DarkNet plans have no such conv3."""
        conv = self.lib.ymi_conv2d_nhwc_f32
        selected = {int(p) for li, p in getattr(self, '_stage_out_ptr', {}).items() if li in self.net.backbone_selected}
        out = []
        for i3, (f3, p3, n3, w3) in enumerate(self.ops):
            if f3 is not conv or i3 in self.wide_ops:
                continue
            d3 = p3.contents
            if not ((d3.kh, d3.kw, d3.stride, d3.pad, d3.nseg, d3.Cin, d3.Cout) == (1, 1, 1, 0, 1, 64, 256)
                    and d3.res_mode == L.RES_ADD and not d3.res_after_act and d3.seg[0].n0 == 0 and d3.seg[0].act <= L.ACT_LEAKY01):
                continue
            yptr, ldy = int(d3.seg[0].ptr or 0), d3.seg[0].row_stride
            if not yptr or yptr in selected:
                continue
            # the next launch on this stream tag (an event record in between only covers more; a wait does not commute)
            i1 = None
            for j in range(i3 + 1, len(self.ops)):
                fj, pj, _, wj = self.ops[j]
                if wj != w3 or fj in ('record', 'nop'):
                    continue
                if fj is conv and j not in self.wide_ops:
                    d1 = pj.contents
                    if ((d1.kh, d1.kw, d1.stride, d1.pad, d1.Cin, d1.Cout, d1.nseg) == (1, 1, 1, 0, 256, 128, 1)
                            and d1.res_mode == L.RES_NONE and int(d1.x or 0) == yptr and d1.ldx == ldy
                            and (d1.B, d1.H, d1.W) == (d3.B, d3.Ho, d3.Wo) and d1.seg[0].n0 == 0 and d1.seg[0].act <= L.ACT_LEAKY01):
                        i1 = j
                break
            if i1 is None:
                continue
            # every other reader of y.  y is no selected output, so only backbone launches can read it, and its buffer is held until
            # the backbone ends (_build frees it there): a launch of another section that names the address means the tensor the
            # arena put there afterwards
            downs, ok = [], True
            for j in range(i3 + 1, len(self.ops)):
                fj, pj, _, _ = self.ops[j]
                if j == i1 or isinstance(fj, str) or self.sections[j] != 'backbone':
                    continue
                if fj is conv:
                    dj = pj.contents
                    if (int(dj.x or 0) == yptr and (dj.kh, dj.kw, dj.stride, dj.pad) == (1, 1, 2, 0) and dj.nseg == 1
                            and (dj.B, dj.H, dj.W, dj.ldx) == (d3.B, d3.Ho, d3.Wo, ldy) and int(dj.res or 0) != yptr
                            and int(dj.seg[0].ptr or 0) != yptr):
                        downs.append(j)
                        continue
                    ptrs = _desc_pointers(dj)
                elif isinstance(pj, tuple):                  # pooling / resize passes
                    ptrs = [a for a in pj if isinstance(a, int)]
                else:                                        # DCN / Winograd / chain descriptors: EVERY pointer field they hold, whatever
                    ptrs = _desc_pointers(pj.contents)       # its name (a descriptor that gains an input is still seen here)
                if yptr in ptrs:
                    ok = False
                    break
            if ok:
                out.append((i3, i1, downs))
        return out

    def entry_chain_candidates(self):
        """Op indices (shortcut, conv3, conv1) of every 64-plane pair whose residual ymi_pointwise_chain_f32 can COMPUTE instead of
        reading it (csrc/chain.hip, chain_h2_k<64, true>): a 1x1 64 -> 256 + RES_ADD conv3 directly followed by the 1x1 256 -> 64
        conv1 that reads its output, whose residual is the output of a 1x1 / stride-1 / pad-0 64 -> 256 convolution of one segment
        with no activation and no residual (the block's projection shortcut), at conv3's pixels, and which nothing but conv3 reads.
        Pure shape logic on the op list (works on a dry CPU plan): fp16x2 planes, magnitude slots and aliasing are checked where the
        launch is installed (_fuse_pointwise_chains).  ResNet plans have one such block, layer0.0; DarkNet plans have none."""
        conv = self.lib.ymi_conv2d_nhwc_f32
        out = []
        for i3, (f3, p3, _, w3) in enumerate(self.ops):
            if f3 is not conv or i3 in self.wide_ops or i3 + 1 >= len(self.ops):
                continue
            d3 = p3.contents
            if not ((d3.kh, d3.kw, d3.stride, d3.pad, d3.nseg, d3.Cin, d3.Cout) == (1, 1, 1, 0, 1, 64, 256)
                    and d3.res_mode == L.RES_ADD and not d3.res_after_act and d3.seg[0].n0 == 0 and d3.seg[0].act <= L.ACT_LEAKY01
                    and d3.res):
                continue
            f1, p1, _, w1 = self.ops[i3 + 1]
            if f1 is not conv or w1 != w3 or (i3 + 1) in self.wide_ops:
                continue
            d1 = p1.contents
            if not ((d1.kh, d1.kw, d1.stride, d1.pad, d1.Cin, d1.Cout, d1.nseg) == (1, 1, 1, 0, 256, 64, 1)
                    and d1.res_mode == L.RES_NONE and d1.x == d3.seg[0].ptr and d1.ldx == d3.seg[0].row_stride
                    and d1.seg[0].n0 == 0 and d1.seg[0].act <= L.ACT_LEAKY01):
                continue
            rptr = int(d3.res)
            idn = None
            for j in range(i3 - 1, -1, -1):                  # the launch that wrote the residual: the last one before conv3 that names it
                fj, pj, _, _ = self.ops[j]
                if fj is conv and any(int(pj.contents.seg[k].ptr or 0) == rptr for k in range(pj.contents.nseg)):
                    idn = j
                    break
            if idn is None or idn in self.wide_ops:
                continue
            dd = self.ops[idn][1].contents
            if not ((dd.kh, dd.kw, dd.stride, dd.pad, dd.nseg, dd.Cin, dd.Cout) == (1, 1, 1, 0, 1, 64, 256)
                    and dd.res_mode == L.RES_NONE and dd.seg[0].act == L.ACT_NONE and dd.seg[0].n0 == 0
                    and (dd.B, dd.Ho, dd.Wo) == (d3.B, d3.Ho, d3.Wo) and dd.seg[0].row_stride == d3.res_ld
                    and int(dd.x or 0) != rptr):
                continue
            # every other launch that names the shortcut tensor, in program order from the shortcut on: the arena frees its buffer
            # after conv3, so the first one may be the launch that WRITES the next tensor put there (a convolution that names the
            # address as an output only) — behind that one the address means another tensor.  Anything else that names it first is
            # a reader, or a launch this scan cannot tell from one
            ok = True
            for j in range(idn + 1, len(self.ops)):
                fj, pj, _, _ = self.ops[j]
                if j == i3 or isinstance(fj, str):
                    continue
                if isinstance(pj, tuple):                    # pooling / resize passes
                    ptrs = [a for a in pj if isinstance(a, int)]
                else:
                    ptrs = _desc_pointers(pj.contents)
                if rptr not in ptrs:
                    continue
                if fj is conv:
                    dj = pj.contents
                    n_out = sum(1 for k in range(dj.nseg) if int(dj.seg[k].ptr or 0) == rptr)
                    ok = ptrs.count(rptr) == n_out
                else:
                    ok = False
                break
            if ok:
                out.append((idn, i3, i3 + 1))
        return out

    def _entry_chain_desc(self, cd, idn):
        """The ENTRY form of a pair's ymi_chain_desc `cd` (a copy: the residual is computed from the shortcut's input by the
        launch), or None where the shortcut of op `idn` has no fp16x2 planes / magnitude slot or the buffers break the aliasing
        contract of include/yolact_amd.h: y must not overlap x0, z may overlap x0 only exactly in place (the arena hands
        conv1's output a buffer the block has just freed: conv3's input or the block input, both M x 64)."""
        dd = self.ops[idn][1].contents
        if not (dd.w_h2 and dd.scale_h2 and dd.x_amax and dd.x):
            return None
        ce = L.ChainDesc.from_buffer_copy(cd)
        ce.res, ce.res_ld = None, 0
        ce.x0, ce.ldx0, ce.x0_amax = dd.x, dd.ldx, dd.x_amax
        ce.w_d_h2, ce.scale_d_h2, ce.bias_d, ce.cout_pad_d = dd.w_h2, dd.scale_h2, dd.bias, _ceil(dd.Cout, 128)
        M = int(ce.M)
        if M * ce.ldx0 >= (1 << 29) or _rows_overlap(M, ce.y, ce.ldy, ce.x0, ce.ldx0):
            return None
        if _rows_overlap(M, ce.z, ce.ldz, ce.x0, ce.ldx0) and not (int(ce.z) == int(ce.x0) and ce.ldz == ce.ldx0):
            return None
        return ce

    def _fuse_stage_exit(self, s, disk, measure, timed):
        """layer0.2.conv3 (+ shortcut, ReLU) and layer1.0.conv1 (256 -> 128) -> ONE ymi_stage_exit_chain_f32 launch that takes y from LDS
        for the second GEMM and, where the only other readers are stride-2 shortcuts, stores y at even rows and columns only (C2 is no
        FPN input: 117 MB per batch-8 step that nothing reads).  Table entry 'chainx(B, H, W)': [1 | 0, ms of the two launches, ms of
        this one], installed where t_one < 0.97 * t_plan.  YOLACT_AMD_CHAIN_EXIT = 1 (default) | 0 | force (install it whatever the
        table says)."""
        mode = os.environ.get('YOLACT_AMD_CHAIN_EXIT', '1')
        self.chainx_table = []
        if mode not in ('1', 'force'):
            return
        lib = self.lib
        for i3, i1, downs in self.stage_exit_candidates():
            f3, p3, n3, w3 = self.ops[i3]
            f1, p1, n1, w1 = self.ops[i1]
            d3, d1 = p3.contents, p1.contents
            if not (d3.w_h2 and d3.x_amax and d1.w_h2):
                continue
            M = d3.B * d3.Ho * d3.Wo
            if M * max(d3.seg[0].row_stride, d3.res_ld, d1.seg[0].row_stride) >= (1 << 29):
                continue
            xd = L.StageExitDesc()
            cd = _fill_chain(xd.chain, d3, d1)
            xd.B, xd.H, xd.W = d3.B, d3.Ho, d3.Wo
            xd.y_stride = 2 if downs else 1         # (no other reader at all: y is written in full, nothing says who reads it)
            # aliasing contract of ymi_stage_exit_chain_f32 (include/yolact_amd.h): z must not overlap x, the residual or y
            if (_rows_overlap(M, cd.z, cd.ldz, cd.y, cd.ldy) or _rows_overlap(M, cd.z, cd.ldz, cd.x, cd.ldx)
                    or (cd.res and _rows_overlap(M, cd.z, cd.ldz, cd.res, cd.res_ld))):
                continue
            xptr = C.pointer(xd)
            name = n3 + '+' + n1
            key = TT.chainx_key(d3.B, d3.Ho, d3.Wo, self.mode)
            ent = disk.get(key)
            if mode == 'force':
                ent = [1, 0.0, 0.0]
            if ent is None:
                self.tune_misses += 1
                if not measure or lib.ymi_stage_exit_chain_f32(xptr, s) != 0:
                    continue
                # the launches it replaces: conv3 — on the streaming kernel where the table prefers that ('chain1') — and conv1
                run3 = lambda: f3(p3, s)
                c1 = disk.get(TT.chain_key('chain1', d3.B, d3.Ho, d3.Wo, mode=self.mode))
                if c1 is not None and c1[0]:
                    ccp = C.pointer(_fill_chain(L.ChainDesc(), d3))
                    if lib.ymi_pointwise_chain_f32(ccp, s) == 0:
                        run3 = lambda: lib.ymi_pointwise_chain_f32(ccp, s)
                t_plan = timed(lambda: (run3(), f1(p1, s)))
                t_one = timed(lambda: lib.ymi_stage_exit_chain_f32(xptr, s))
                ent = disk[key] = [1 if t_one < 0.97 * t_plan else 0, round(t_plan, 4), round(t_one, 4)]
            self.chainx_table.append((name, ent[0], ent[1], ent[2]))
            if ent[0] and lib.ymi_stage_exit_chain_f32(xptr, s) == 0:
                self.keepalive.append(xd)
                self.ops[i3] = (lib.ymi_stage_exit_chain_f32, xptr, name, w3)
                self.ops[i1] = ('nop', None, n1 + '[fused into ' + n3 + ']', w1)
                # profile records map onto conv_meta by position (kind 13, then kind 12 = conv1): in two-stream plans the
                # projection shortcut was appended between the two layers
                names = [n for n, _ in self.conv_meta]
                if n3 in names and n1 in names:
                    a, b = names.index(n3), names.index(n1)
                    if b > a + 1:
                        self.conv_meta.insert(a + 1, self.conv_meta.pop(b))

    def _apply_choice(self, fn, dptr, where, val, s):
        """Install a direct choice of the table (tile id, split_k) in a descriptor; returns the launch status of one run."""
        d = dptr.contents.conv if fn is self.lib.ymi_dcn_v2_forward_f32 else dptr.contents
        tile, S = TT.direct_parts(val)
        d.tile = tile
        if S > 1:
            is_dcn = fn is self.lib.ymi_dcn_v2_forward_f32
            if tile & L.TILE_DCNP:
                nk_ = d.Kpad // 32
                if -(-nk_ // S) * (S - 1) >= nk_:
                    return -1
            elif is_dcn or not self._splitk_ok(d) or (d.Kpad // 32) % S:
                return -1
            d.split_k = S
            d.split_ws = self._splitk_ws(where, S * d.B * d.Ho * d.Wo * d.Cout).data_ptr()
        else:
            d.split_k = 0
        return fn(dptr, s)

    @staticmethod
    def _pipe_ok(d):
        """Ordinary convolutions the pipelined kernel of csrc/dcn.hip takes (run_pipe): 3x3 / pad 1 or 1x1 / pad 0, Cin % 32 == 0, one
        dense output, activation none / ReLU / LeakyReLU, residual none / add."""
        return ((d.kh, d.kw, d.pad) in ((3, 3, 1), (1, 1, 0)) and d.Cin % 32 == 0 and d.Kpad == d.kh * d.kw * d.Cin and d.Kpad >= 64
                and d.nseg == 1 and d.Cout % 4 == 0 and d.seg[0].n0 == 0 and d.seg[0].act <= L.ACT_LEAKY01
                and d.seg[0].row_stride % 4 == 0 and d.seg[0].batch_stride == d.Ho * d.Wo * d.seg[0].row_stride
                and d.res_mode in (L.RES_NONE, L.RES_ADD))

    @staticmethod
    def dcnp_candidates(d, dcn=False):
        """Direct choices of the pipelined DCN kernel for a descriptor: every block tile unsplit, and — where a tile's grid alone
        leaves CUs idle (the 35x35 / 18x18 maps) — chunk-aligned K splits that bring the block count to 0.5 .. 2 blocks per CU."""
        M, nk = d.B * d.Ho * d.Wo, d.Kpad // 32
        out = []
        for t, name in sorted(L.DCNP_TILES.items()):
            bm, bn = (int(v) for v in name[4:].split('w')[0].split('x'))
            if (bn > 128 and d.Cout < 256) or (dcn and t in L.DCNP_PLAIN_ONLY) or (bn == 32) != (d.Cout <= 32):
                continue                                  # (32-column tiles: the Cout <= 32 layers, and nothing else for those)
            tid = t | L.TILE_H2 | L.TILE_DCNP
            out.append(tid)
            out += _split_k_ids(tid, -(-M // bm) * -(-d.Cout // bn), nk, d.Cout)
        return out

    @staticmethod
    def patch2_candidates(d):
        """Tile ids of csrc/patch2.hip (3x3 / stride 1 / pad 1 with the input patch of a pixel tile in LDS, filters streamed) for a
        descriptor it takes: Cin % 32 == 0, Cout >= 64 and % 4 == 0, no residual, 1 .. 3 dense segments with boundaries at multiples of 128
        channels, activation none / ReLU / LeakyReLU.  YOLACT_AMD_PATCH2=0 removes them (A/B switch)."""
        if os.environ.get('YOLACT_AMD_PATCH2', '1') != '1':
            return []
        if not ((d.kh, d.kw, d.stride, d.pad) == (3, 3, 1, 1) and d.Cin % 32 == 0 and d.Kpad == 9 * d.Cin and d.Cout >= 64 and d.Cout % 4 == 0
                and d.res_mode == L.RES_NONE and 1 <= d.nseg <= 3 and d.w_h2):
            return []
        cov = 0
        for i in range(d.nseg):
            g = d.seg[i]
            if (g.n0 != cov or g.n0 % 128 or g.act > L.ACT_LEAKY01 or g.act < 0 or g.row_stride % 4 or g.row_stride < g.n1 - g.n0
                    or g.batch_stride != d.Ho * d.Wo * g.row_stride):
                return []
            cov = g.n1
        if cov < d.Cout:
            return []
        return [t | L.TILE_H2 | L.TILE_DCNP for t in sorted(L.PATCH2_TILES)]

    @staticmethod
    def pc_candidates(d):
        """Direct choices of the producer / consumer kernel (csrc/pcconv.hip) for a descriptor the pipelined kernel takes (_pipe_ok)
        with more than 32 output channels: the block tile unsplit, and the chunk-aligned K splits that bring a
        short grid to 0.5 .. 4 blocks per CU.  OPT-IN (YOLACT_AMD_PC=1): measured in sessions r6b / r6c, never in front of the pipelined
        tiles (profiles/r06_pc_probe.txt) — both are bound by the same global -> LDS rates, not by how the waves share the work."""
        if os.environ.get('YOLACT_AMD_PC', '0') != '1' or d.Cout <= 32:
            return []
        M, nk = d.B * d.Ho * d.Wo, d.Kpad // 32
        out = []
        for t, name in sorted(L.PC_TILES.items()):
            bm, bn = (int(v) for v in os.environ.get('YOLACT_AMD_PC_SHAPE', name[2:]).split('x'))     # (YMI_PC_FLAGS 32 / 64 experiments: the
            if bn > 128 and d.Cout < 256:                                                              #  block behind the id is 32 / 64 x 128)
                continue
            tid = t | L.TILE_H2 | L.TILE_DCNP
            out.append(tid)
            out += _split_k_ids(tid, -(-M // bm) * -(-d.Cout // bn), nk, d.Cout)
        return out

    @staticmethod
    def ws_candidates(d):
        """Direct choices of the weight-stationary streaming kernel (csrc/wstat.hip) for a descriptor it takes
        (_pipe_ok, no residual, Cout <= 64): every block shape of the column width that covers Cout, with the K ranges that make a
        block's filters fit its 64 KB of LDS — the fewest ranges, and a few more where that leaves the grid short of the chip."""
        if d.res_mode != L.RES_NONE or d.Cout > 64:
            return []
        M, nk = d.B * d.Ho * d.Wo, d.Kpad // 32
        out = []
        for t, name in sorted(L.WS_TILES.items()):
            bm, bn = (int(v) for v in name[2:].split('w')[0].split('x'))
            if (bn == 32) != (d.Cout <= 32):
                continue
            cap = (64 * 1024) // (bn * 128)                # chunks of filters (bn columns x 32 k x 2 planes x 2 bytes) in 64 KB
            blocks, n = -(-M // bm), 0
            for S in (1, 2, 3, 4, 5, 6, 8, 9, 12, 16):
                per = -(-nk // S)
                if per > cap or (S > 1 and per * (S - 1) >= nk):
                    continue
                if n and blocks * S > 1200:                # beyond the fewest ranges: only while the grid is short of ~4 blocks per CU
                    break
                out.append(TT.direct_choice(t | L.TILE_H2 | L.TILE_DCNP, S))
                n += 1
                if n == 3:
                    break
        return out

    def direct_key(self, fn, d, wide=False):
        """Table key of one convolution / DCN descriptor; `wide`: the layer is under the outlier-channel guard (bf16x3 tiles, DCN:
        exact-fp32 tiles, for this layer only)."""
        is_dcn = fn is self.lib.ymi_dcn_v2_forward_f32
        h2_, split_ = self.h2 and not wide, self.split or (wide and not is_dcn)
        return TT.desc_key(d, 'x3' if split_ else 'h2' if h2_ else '', dcn=is_dcn)

    def direct_candidates(self, fn, d, wide=False):
        """Direct choices _tune_direct measures for one convolution descriptor (also tools/overlap_tune.py)."""
        is_dcn = fn is self.lib.ymi_dcn_v2_forward_f32
        h2_, split_ = self.h2 and not wide, self.split or (wide and not is_dcn)
        if is_dcn:                   # DCN gather loader: basic tiles; the bf16x3 arithmetic does not exist for it
            cands = [t for t in L.BASIC_TILES if t != L.TILE_128x32]
        elif d.Cin % 32 != 0:        # stem loader: basic tiles only
            cands = [L.TILE_128x64, L.TILE_64x64] if d.Cout <= 64 else list(L.BASIC_TILES)
        elif d.Cout <= 32:
            cands = [L.TILE_128x32, L.TILE_64x64, L.TILE_64x64_S3, L.TILE_32x32_K4, L.TILE_32x32_K4_S4,
                     L.TILE_64x32_K2, L.TILE_64x32_K2_S3]
        elif d.Cout <= 64:
            cands = [L.TILE_128x64, L.TILE_128x64_S3, L.TILE_64x64, L.TILE_64x64_S3, L.TILE_64x64_S4,
                     L.TILE_32x32_K4, L.TILE_32x32_K4_S4, L.TILE_64x32_K2, L.TILE_64x32_K2_S3,
                     L.TILE_32x64_K2, L.TILE_32x64_K2_S3]
        else:
            cands = [t for t in sorted(L.TILE_NAMES) if t != L.TILE_128x32 and not (t & (L.TILE_X3 | L.TILE_H2))]
            if d.Cout < 256:
                cands = [t for t in cands if t != L.TILE_128x256_W8]
        spflag = (L.TILE_X3 if split_ else L.TILE_H2 if h2_ else 0) if not (is_dcn and split_) else 0
        if spflag:      # (the Cin = 4 stem loader has the basic tiles only)
            base_ok = L.H2_BASE_TILES if spflag == L.TILE_H2 else L.X3_BASE_TILES
            cands = cands + [t | spflag for t in cands if t in base_ok
                             and (d.Cin % 32 == 0 or t in L.BASIC_TILES)]
        if is_dcn and h2_:           # the pipelined gather-GEMM of csrc/dcn.hip (fp16x2 plans)
            cands = cands + self.dcnp_candidates(d, dcn=True)
        if not is_dcn and h2_ and self.pipe and self._pipe_ok(d):   # the same pipelined kernel as an ordinary convolution
            cands = cands + self.dcnp_candidates(d) + self.ws_candidates(d)     # (+ the streaming kernel for narrow outputs)
            cands = cands + self.pc_candidates(d)                               # (+ round 6: producer / consumer blocks, opt-in)
        if not is_dcn and h2_ and self.pipe:
            cands = cands + self.patch2_candidates(d)                           # (+ round 6: 3x3 with the input patch in LDS)
            if ((d.kh, d.kw, d.stride, d.pad, d.Cin, d.Cout) == (3, 3, 1, 1, 64, 64) and d.res_mode == L.RES_NONE
                    and TT.patch_tile_allowed()):
                cands = cands + [L.DCNP_PATCH_C64 | L.TILE_H2 | L.TILE_DCNP]    # csrc/patch.hip: the input patch in LDS, filters in registers
        if not is_dcn and self._splitk_ok(d) and self.splitk:
            # split-K candidates: big tiles whose grid alone cannot fill the chip, K cut 2 / 4 ways
            x3 = spflag
            for S in (2, 4):
                if (d.Kpad // 32) % S == 0 and d.Kpad // S >= 128:
                    cands += [TT.direct_choice(t | x3, S) for t in (L.TILE_128x128, L.TILE_64x128, L.TILE_128x64, L.TILE_64x64,
                                                                    L.TILE_256x128_W8)]

        return cands

    def _tune_direct(self, e0, e1, s, reps, disk, measure):
        cache = {}
        cname = TT.choice_name
        for opi, (fn, dptr, name, where) in enumerate(self.ops):
            is_dcn = fn is self.lib.ymi_dcn_v2_forward_f32
            if fn is not self.lib.ymi_conv2d_nhwc_f32 and not is_dcn:
                continue
            d = dptr.contents.conv if is_dcn else dptr.contents
            wide = opi in self.wide_ops            # outlier-channel guard: bf16x3 tiles (DCN: exact-fp32 tiles) for this layer only
            skey = self.direct_key(fn, d, wide)
            key = (skey, wide)
            if key not in cache and skey in disk:
                v_ = int(disk[skey])
                patch_off = (TT.direct_parts(v_)[0] == (L.DCNP_PATCH_C64 | L.TILE_H2 | L.TILE_DCNP) and not TT.patch_tile_allowed())
                # (YOLACT_AMD_PATCH=0: the A/B switch of csrc/patch.hip — a table entry that names it counts as a miss)
                if not patch_off and self._apply_choice(fn, dptr, where, disk[skey], s) == 0:   # a stale / foreign entry must not make every forward raise
                    cache[key] = v_
            if key not in cache:
                self.tune_misses += 1
                if not measure:
                    cache[key] = L.TILE_AUTO
                    d.tile, d.split_k = L.TILE_AUTO, 0
                    continue
                cands = self.direct_candidates(fn, d, wide)
                best, best_ms, times = None, 1e30, {}
                ok_cands = []
                for t in cands:                       # warm every candidate once (code fetch, clocks); skip the
                    if self._apply_choice(fn, dptr, where, t, s) == 0:        # ones this layer cannot use
                        ok_cands.append(t)
                # the launch's own magnitude-bound slot is zeroed before every timed launch, as at the start of a real run:
                # a slot that already holds the maximum hides the atomics of the first residency round
                yslot = self.amax[(d.y_amax - self.amax.data_ptr()) // 4:][:L.AMAX_SLOT_FLOATS] if d.y_amax else None
                for rnd in range(2):                  # two interleaved rounds, keep each tile's best time: a single
                    for t in ok_cands:                # noisy sample used to flip near-ties and move bench by +-3 %
                        self._apply_choice(fn, dptr, where, t, s)
                        e0.record()
                        for _ in range(reps):
                            if yslot is not None:
                                yslot.zero_()
                            fn(dptr, s)
                        e1.record()
                        e1.synchronize()
                        ms = e0.elapsed_time(e1) / reps
                        times[cname(t)] = round(min(ms, times.get(cname(t), 1e30)), 4)
                for t in ok_cands:
                    if times[cname(t)] < best_ms:
                        best, best_ms = t, times[cname(t)]
                assert best is not None, name
                cache[key] = best
                disk[skey] = best
                self.tune_table.append((name, cname(best), times))
            self._apply_choice(fn, dptr, where, cache[key], s)

    def _wino_gemm_tiles(self):
        """Winograd choices (GEMM tile, V planes) the tuner measures for a layer of this plan's arithmetic."""
        wtiles = [L.TILE_64x64, L.TILE_64x128, L.TILE_128x64, L.TILE_128x128_W8, L.TILE_64x128_S3, L.TILE_32x64_K2,
                  L.TILE_128x128, L.TILE_128x128_S3, L.TILE_128x128_W8_S3, L.TILE_256x128_W8, L.TILE_256x128_W8_S3]
        if self.split:
            wtiles = wtiles + [t | L.TILE_X3 for t in wtiles]
        if self.h2:     # fp16x2 GEMM tiles, V either fp32 (split on the fly) or written as fp16 planes by the input transform
            hb = wtiles + [L.TILE_128x256_W8]
            wtiles = wtiles + [t | L.TILE_H2 for t in hb] + [TT.wino_choice(t | L.TILE_H2, planes=1) for t in hb]
            if os.environ.get('YOLACT_AMD_WGEMM', '1') == '1':       # round 6: the persistent producer / consumer grouped GEMM (planes only)
                wtiles = wtiles + [TT.wino_choice(L.TILE_WG_128x256 | L.TILE_H2, planes=1)]
        return wtiles

    def level_merge_keys(self):
        """Table keys of the merged P4..P7 head launches (engine.Plan._build_level_merge): the VIRTUAL Winograd shapes of
        tune_table.level_key, (merged up-feature, merged .out); None where the plan has no such alternative."""
        lm = self.level_merge
        if lm is None:
            return None
        B, Cin, Cup, Chead = lm['shape']
        return (TT.level_key(B, lm['tiles'], Cin, Cup, L.ACT_RELU, 0, self.mode),
                TT.level_key(B, lm['tiles'], Cup, Chead, L.ACT_NONE, lm['descs'][1].nseg, self.mode))

    def install_level_merge(self, choices=None):
        """Replace head1.up0 / head1.out by the merged launches (Winograd choices `choices`, default the descriptors' own) and turn
        the per-level launches of the other levels into nops.  Pure op-list surgery: works on a dry CPU plan.  conv_meta keeps every
        entry: the merged launches are recorded as head1's layers, the absorbed ones as kind 12 behind them (ymi_wino_desc.nabs)."""
        lm = self.level_merge
        if lm is None or self.merged_levels:
            return self.merged_levels
        conv = self.lib.ymi_conv2d_nhwc_f32
        wino = self.lib.ymi_conv3x3_winograd_f32
        if not all(self.ops[i][0] in (conv, wino) for i in lm['up'] + lm['out']):
            return False
        for d, v in zip(lm['descs'], choices or ()):
            _set_wino_choice(d, v)
        for d, idxs in zip(lm['descs'], (lm['up'], lm['out'])):
            _, _, name, where = self.ops[idxs[0]]
            name = name.replace('[wino]', '')
            self.ops[idxs[0]] = (wino, C.pointer(d), name + '[levels %d-%d][wino]' % (lm['levels'][0], lm['levels'][-1]), where)
            for i in idxs[1:]:
                _, _, n_i, w_i = self.ops[i]
                self.ops[i] = ('nop', None, n_i.replace('[wino]', '') + '[merged into ' + name + ']', w_i)
        self.merged_levels = True
        return True

    def _merge_levels(self, e0, e1, s, reps, disk, measure):
        """The P4..P7 prediction heads as ONE Winograd layer per shared conv (engine.Plan._build_level_merge, ymi_wino_desc.nlev),
        installed where the two merged launches measured faster than the per-level launches they replace (each level's tuned best:
        called after _tune_direct / _tune_winograd).  Two entries under the virtual shapes of tune_table.level_key:
        [4, Winograd choice of the merged GEMM, summed ms of the per-level launches, ms of the merged launch, 0, the same].
        YOLACT_AMD_MERGE_LEVELS = 1 (default) | 0 (keep the per-level launches) | force (install it whatever the table says).
        The descriptors' own (H, W) hold the virtual shape of their key (the library ignores them with a table): same B, C, Cout,
        tile and the same T, i.e. the GEMM shape the fp64 pin of that table key launches (tests/test_gpu_winograd_kat.py)."""
        self.level_table = []
        mode = os.environ.get('YOLACT_AMD_MERGE_LEVELS', '1')
        lm = self.level_merge
        if lm is None or mode not in ('1', 'force') or not self.use_winograd or 4 not in self.wino_variants:
            return
        if self.wino_force and mode != 'force':     # YOLACT_AMD_WINOGRAD_FORCE: every eligible layer on its OWN Winograd launches
            return
        lib = self.lib
        keys = self.level_merge_keys()
        ents = []
        for key, d, idxs in zip(keys, lm['descs'], (lm['up'], lm['out'])):
            ent = disk.get(key)
            if ent is not None and ent[1]:          # validate the stored tile with one launch
                _set_wino_choice(d, ent[1])
                if lib.ymi_conv3x3_winograd_f32(C.byref(d), s) != 0:
                    ent = None
            if ent is None:
                self.tune_misses += 1
                if not measure:
                    ents.append(None)
                    continue
                t_plan = sum(_timed((lambda f=self.ops[i][0], a=self.ops[i][1]: f(a, s)), e0, e1, reps) for i in idxs)
                best_t, best_ms = 0, 1e30
                dptr = C.pointer(d)
                for t in self._wino_gemm_tiles():
                    if not (TT.wino_parts(t)[0] & L.TILE_H2):
                        continue
                    _set_wino_choice(d, t)
                    if lib.ymi_conv3x3_winograd_f32(dptr, s) != 0:
                        continue
                    ms = _timed(lambda: lib.ymi_conv3x3_winograd_f32(dptr, s), e0, e1, reps)
                    if ms < best_ms:
                        best_t, best_ms = t, ms
                ent = disk[key] = [4 if best_t else 0, best_t, round(t_plan, 4), round(best_ms if best_t else 0.0, 4), 0.0,
                                   round(best_ms if best_t else 0.0, 4)]
            ents.append(ent)
        torch.cuda.synchronize(self.device)
        ok = all(e is not None and e[1] for e in ents)
        if ok:
            t_plan, t_one = sum(e[2] for e in ents), sum(e[3] for e in ents)
            self.level_table = [(k, e[1], e[2], e[3]) for k, e in zip(keys, ents)]
            if mode == 'force' or t_one < 0.97 * t_plan:
                self.install_level_merge([e[1] for e in ents])
        elif mode == 'force':
            for d in lm['descs']:
                d.tile, d.v_planes = L.TILE_128x128 | L.TILE_H2, 1
            if all(lib.ymi_conv3x3_winograd_f32(C.byref(d), s) == 0 for d in lm['descs']):
                self.install_level_merge()

    def _tune_winograd(self, e0, e1, s, reps, disk, measure):
        """Per eligible layer: best GEMM tile of the Winograd path, then Winograd vs the (already tuned) direct kernel.
        The winner replaces the op in the list."""
        lib = self.lib
        self.wino_toggle = {}       # table key -> [(op index, direct op, Winograd op, isolated timing favours Winograd)]: tools/instep_tune.py
        wtiles = self._wino_gemm_tiles()
        memo = {}
        for idx, alts in sorted(self.wino_alt.items()):
            fn, dptr, name, where = self.ops[idx]
            if fn is not lib.ymi_conv2d_nhwc_f32:
                continue
            w0 = alts[0]
            key = TT.wino_key(w0.B, w0.H, w0.W, w0.C, w0.Cout, w0.act, w0.nseg, tuple(a.m for a in alts), self.mode)
            if key not in memo and key in disk:
                ent = tuple(disk[key])
                ok = True
                if ent[1]:                                 # validate the stored (m, tile) with one launch
                    wd = [a for a in alts if a.m == ent[0]]
                    if wd:
                        _set_wino_choice(wd[0], ent[1])
                        ok = lib.ymi_conv3x3_winograd_f32(C.byref(wd[0]), s) == 0
                    else:
                        ok = False
                if ok:
                    memo[key] = ent
            if key not in memo:
                self.tune_misses += 1
                if not measure:
                    memo[key] = (0, 0, 0.0, 0.0, 0.0, 0.0)
                else:
                    t_direct = _timed(lambda: fn(dptr, s), e0, e1, reps)
                    best_m, best_t, best_ms, per_m = 0, 0, 1e30, {}
                    for wd in alts:
                        for t in wtiles:
                            _set_wino_choice(wd, t)
                            if lib.ymi_conv3x3_winograd_f32(C.byref(wd), s) != 0:
                                continue
                            wptr = C.pointer(wd)
                            ms = _timed(lambda: lib.ymi_conv3x3_winograd_f32(wptr, s), e0, e1, reps)
                            per_m[wd.m] = min(ms, per_m.get(wd.m, 1e30))
                            if ms < best_ms:
                                best_m, best_t, best_ms = wd.m, t, ms
                    memo[key] = (best_m, best_t, round(t_direct, 4), round(best_ms, 4),
                                 round(per_m.get(2, 0.0), 4), round(per_m.get(4, 0.0), 4))
                    disk[key] = list(memo[key])
            best_m, best_t, t_direct, t_wino, t_f2, t_f4 = memo[key]
            best_tile, best_planes = TT.wino_parts(best_t)
            self.wino_table.append((name, 'F%d/%s%s' % (best_m, L.TILE_NAMES.get(best_tile, '-'), 'p' if best_planes else ''),
                                    t_direct, t_wino, t_f2, t_f4))
            # 'instep|<key>' = 0 (tools/instep_tune.py, round 5): the isolated timings above favour Winograd, but measured INSIDE the step
            # — three launches and their V / M tensors crossing the memory side between them, against one launch — the direct kernel
            # is the faster choice for this shape: keep it.  (Decided on whole-step time with every layer of the shape toggled.)
            instep_direct = disk.get(TT.instep_key(key)) == 0 and not self.wino_force
            if best_t and not (self.wino_up.get(idx) is not None or (self.wino_proj is not None and self.wino_proj[0] == idx)):
                wd_ = [a for a in alts if a.m == best_m][0]
                _set_wino_choice(wd_, best_t)
                self.wino_toggle.setdefault(key, []).append(
                    (idx, (fn, dptr, name, where), (lib.ymi_conv3x3_winograd_f32, C.pointer(wd_), name + '[wino]', where),
                     bool(t_wino < 0.97 * t_direct)))
            if best_t and (self.wino_force or (t_wino < 0.97 * t_direct and not instep_direct)):
                wd = [a for a in alts if a.m == best_m][0]
                _set_wino_choice(wd, best_t)
                self.ops[idx] = (lib.ymi_conv3x3_winograd_f32, C.pointer(wd), name + '[wino]', where)
                up = self.wino_up.get(idx)
                if up is not None and best_m == 4 and wd.H % 2 == 0 and wd.W % 2 == 0:
                    bidx, lo_ptr, relu = up        # the upsampled tensor is never materialised: the input transform interpolates
                    wd.x_up, wd.up_relu = lo_ptr, relu
                    bfn, bargs, bname, bwhere = self.ops[bidx]
                    self.ops[bidx] = ('nop', None, bname + '[fused into ' + name + ']', bwhere)
                if self.wino_proj is not None and self.wino_proj[0] == idx and best_m == 4 and wd.Cout == 256 and wd.nseg == 0:
                    pidx = self.wino_proj[1]
                    pfn, pdptr, pname, pwhere = self.ops[pidx]
                    if pfn is lib.ymi_conv2d_nhwc_f32 and pwhere == where:
                        pd = pdptr.contents          # the 1x1's own descriptor: filters, epilogue, output, bound slot
                        wd.proj_w_h2, wd.proj_scale_h2, wd.proj_bias = pd.w_h2, pd.scale_h2, pd.bias
                        wd.proj_y, wd.proj_y_amax = pd.seg[0].ptr, pd.y_amax
                        wd.proj_cout, wd.proj_ldy, wd.proj_act = pd.Cout, pd.seg[0].row_stride, pd.seg[0].act
                        # proj_y is patched per call (NULL here): validate the fused descriptor with ONE launch into a scratch
                        # prototype tensor; if the library rejects it the two separate launches stay (round-4 advisor: every other
                        # fusion is validated before it is installed — an unvalidated one would make every forward raise)
                        scratch = torch.empty(self.proto_shape, dtype=torch.float32, device=self.device)
                        wd.proj_y = scratch.data_ptr()
                        rc = lib.ymi_conv3x3_winograd_f32(C.byref(wd), s)
                        torch.cuda.synchronize(self.device)
                        wd.proj_y = None
                        if rc != 0:
                            wd.proj_w_h2 = None
                            self.wino_proj_rejected = rc
                        else:
                            self.ops[pidx] = ('nop', None, pname + '[fused into ' + name + ']', pwhere)
                            self.proto_patch_wino = wd

    def set_winograd(self, key, on: bool):
        """Switch every layer of one Winograd table key between its direct launch and its three Winograd launches (tools/instep_tune.py:
        whole-step A/B of the choice the isolated timings made).  Only layers without a fused upsampling / projection are listed."""
        for idx, direct_op, wino_op, _ in self.wino_toggle.get(key, []):
            self.ops[idx] = wino_op if on else direct_op
