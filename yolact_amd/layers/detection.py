"""`Detect` — layers/functions/detection.py:11-78 on device.

Same constructor, same flags (`use_fast_nms`, `use_cross_class_nms`, set by eval.py:871-872), same return
structure.  The per-image Python loop, boolean-mask gathers and 80 sorts of the reference become three kernel
launches for the whole batch (csrc/detect.hip) plus ONE device->host read of the per-image counts, which the
reference's dynamic output shapes make unavoidable.

Traditional NMS (use_fast_nms False, the reference's per-class greedy Cython NMS, detection.py:182-228) runs on the device
(csrc/detect_greedy.hip) when `traditional_nms_on_device` is set — its default is the environment's YOLACT_AMD_TRADITIONAL_NMS=1
at construction.  Without it, use_fast_nms False still runs Fast NMS with a warning (YOLACT_AMD_STRICT_NMS=1: an error).
"""
from __future__ import annotations

import ctypes
import ctypes as C
import sys
import contextlib
import os
import threading
import warnings

import torch

from .. import _lib as L
from ..config import active_cfg


def _timer_env(name):
    t = sys.modules.get('utils.timer')
    return t.env(name) if (t is not None and hasattr(t, 'env')) else contextlib.nullcontext()


class Detect(object):
    _warned_traditional = False

    def __init__(self, num_classes, bkg_label, top_k, conf_thresh, nms_thresh):
        self.num_classes = num_classes
        self.background_label = bkg_label
        self.top_k = top_k
        self.nms_thresh = nms_thresh
        if nms_thresh <= 0:
            raise ValueError('nms_threshold must be non negative.')   # detection.py:25-26
        self.conf_thresh = conf_thresh
        self.use_cross_class_nms = False
        self.use_fast_nms = False  # detection.py:30: the reference's default; eval.py:871 sets it from --fast_nms (True)
        # opt-in: use_fast_nms False runs the device's greedy NMS instead of Fast NMS (the environment variable exists for callers
        # that build the model themselves, like the reference's eval.py)
        self.traditional_nms_on_device = os.environ.get('YOLACT_AMD_TRADITIONAL_NMS', '0') == '1'
        self._ws = {}
        self._ws_lock = threading.Lock()
        self.last_prior_idx = None   # per image: prior index of every returned detection (diagnostics / parity tests;
                                     # NOT part of the reference's return structure, so it is kept off the dicts)

    def nms_mode(self):
        """'greedy' (traditional NMS on the device), 'cross_class' (cross-class Fast NMS) or 'fast'."""
        if not self.use_fast_nms and self.traditional_nms_on_device:
            return 'greedy'
        return 'cross_class' if self.use_cross_class_nms else 'fast'

    def capacity(self):
        """Detections per image the device outputs can hold: top_k for cross-class Fast NMS, else cfg.max_num_detections
        (greedy NMS cuts to max_num_detections whatever use_cross_class_nms says, detection.py:220-222)."""
        if self.nms_mode() == 'cross_class':
            return int(self.top_k)
        return int(active_cfg().max_num_detections)

    def _workspace(self, B, P, C, D, cap, dev, slot=0, mode='fast'):
        """Scratch tensors of the three Detect kernels, one set per (shape, device, slot, NMS mode).  They live as long as this
        Detect object: raw addresses of a set may be baked into a captured hipGraph (YOLACT_AMD_GRAPH=1), so nothing
        is ever evicted behind a graph's back (a set is ~B*P*85*4 bytes, 52 MB at batch 8; greedy mode: class-major scores
        plus one byte buffer of ~B*P*(C-1)*8 bytes, its large-K candidate keys)."""
        key = (B, P, C, D, cap, dev, slot, mode)
        ws = self._ws.get(key)
        if ws is None:
            with self._ws_lock:
                ws = self._ws.get(key)
                if ws is None and mode == 'greedy':
                    d = L.DetectDesc()
                    d.B, d.P, d.C, d.D, d.max_det = B, P, C, D, cap
                    nbytes = L.lib().ymi_workspace_bytes(L.WS_DETECT_GREEDY, ctypes.byref(d))   # (C: the class count here)
                    if nbytes < 0:
                        raise RuntimeError('yolact_amd: greedy Detect workspace size failed (code %d)' % nbytes)
                    ws = dict(scores_t=torch.empty(B, C - 1, P, device=dev),
                              greedy=torch.empty(nbytes, dtype=torch.uint8, device=dev))
                    self._ws[key] = ws
                elif ws is None:
                    nfg = C - 1
                    ws = dict(
                        scores_t=torch.empty(B, nfg, P, device=dev), keep=torch.empty(B, P, dtype=torch.int32, device=dev),
                        num_keep=torch.zeros(B, dtype=torch.int32, device=dev), maxsc=torch.empty(B, P, device=dev),
                        argmax=torch.empty(B, P, dtype=torch.int32, device=dev),
                        cand_score=torch.empty(B, nfg * self.top_k, device=dev),
                        cand_prior=torch.empty(B, nfg * self.top_k, dtype=torch.int32, device=dev))
                    self._ws[key] = ws
        return ws

    def run_device(self, loc, conf, mask, priors, conf_is_logits, stream=None, slot=0, conf_ld=0):
        """Launch the Detect kernels; returns fixed-capacity device tensors (no host sync).  `stream`: raw
        hipStream_t (ctypes void*) to launch on — the execution plan passes its side stream — default: torch's
        current stream.  Output tensors are always allocated under the ambient stream."""
        self._require_fast_nms()
        mode = self.nms_mode()
        for name, t in (('loc', loc), ('conf', conf), ('mask', mask), ('priors', priors)):
            L.require_cuda(t, name)
        cfg = active_cfg()
        B, P, Ccls = conf.shape
        if conf_ld:                      # the engine's padded class rows [B, P, conf_ld]: num_classes of them are real
            Ccls = self.num_classes
            assert conf.shape[2] == conf_ld >= Ccls
        D = mask.shape[2]
        dev = conf.device
        max_det = int(cfg.max_num_detections)
        cap = self.capacity()
        ws = self._workspace(B, P, Ccls, D, cap, dev, slot, mode)
        return self._launch(loc, conf, mask, priors, conf_is_logits, stream, ws, B, P, Ccls, D, dev, max_det, cap, conf_ld,
                            greedy=(mode == 'greedy'))

    def _require_fast_nms(self):
        """detection.py:101-106: with use_fast_nms False (the reference's constructor default) the reference runs
        traditional_nms — per-class greedy NMS in Cython on the CPU (utils/cython_nms.pyx), outside the hot path (SURVEY 2:
        non-default in eval.py, a CPU round trip per class).  A plain `Yolact()(x)` must still work, so the engine runs
        Fast NMS — what eval.py:871 selects through its default --fast_nms=True — and says so once per Detect object, loudly;
        YOLACT_AMD_STRICT_NMS=1 turns the warning into NotImplementedError for callers that must not differ."""
        if self.use_fast_nms:
            return
        if self.traditional_nms_on_device:
            if self.use_cross_class_nms and not getattr(self, '_warned_cc_traditional', False):
                self._warned_cc_traditional = True               # detection.py:107-108 prints this and runs per-class NMS
                warnings.warn('Warning: Cross Class Traditional NMS is not implemented.', UserWarning, stacklevel=3)
            return
        msg = ('Detect.use_fast_nms is False (the reference default): traditional Cython/CPU NMS is not part of the MI355X '
               'hot path; running Fast NMS instead (eval.py:871 sets use_fast_nms = True for its default --fast_nms).')
        if os.environ.get('YOLACT_AMD_STRICT_NMS', '0') == '1':
            raise NotImplementedError(msg)
        if not getattr(self, '_warned_traditional_nms', False):    # once per Detect INSTANCE (round-3 advisor: a process-wide
            self._warned_traditional_nms = True                    # flag hid the deviation for every model after the first)
            Detect._warned_traditional = True
            warnings.warn(msg, UserWarning, stacklevel=3)

    def _launch(self, loc, conf, mask, priors, conf_is_logits, stream, ws, B, P, Ccls, D, dev, max_det, cap, conf_ld=0,
                greedy=False):
        out = dict(count=torch.empty(B, dtype=torch.int32, device=dev), box=torch.empty(B, cap, 4, device=dev),
                   score=torch.empty(B, cap, device=dev), cls=torch.empty(B, cap, dtype=torch.int64, device=dev),
                   coef=torch.empty(B, cap, D, device=dev), prior=torch.empty(B, cap, dtype=torch.int32, device=dev),
                   # the same detections as one fixed-size record per image (count | cap x (box, score, class, coef)): the
                   # payload of the data-parallel gather, written by the selection kernel itself (parallel.pack_records)
                   rec=torch.empty(B, 1 + cap * (6 + D), device=dev))
        d = L.DetectDesc()
        loc, conf, mask, priors = (t.contiguous() for t in (loc.float(), conf.float(), mask.float(), priors.float()))
        d.conf, d.loc, d.coef, d.priors = conf.data_ptr(), loc.data_ptr(), mask.data_ptr(), priors.data_ptr()
        d.B, d.P, d.C, d.D = B, P, Ccls, D
        d.conf_ld = int(conf_ld)
        d.conf_is_logits = 1 if conf_is_logits else 0
        d.top_k, d.max_det = int(self.top_k), max_det
        d.conf_thresh, d.nms_thresh = float(self.conf_thresh), float(self.nms_thresh)
        d.cross_class = 1 if self.use_cross_class_nms else 0
        d.scores_t = ws['scores_t'].data_ptr()
        if not greedy:
            d.keep, d.num_keep = ws['keep'].data_ptr(), ws['num_keep'].data_ptr()
            d.maxsc, d.argmax = ws['maxsc'].data_ptr(), ws['argmax'].data_ptr()
            d.cand_score, d.cand_prior = ws['cand_score'].data_ptr(), ws['cand_prior'].data_ptr()
        d.out_count, d.out_box, d.out_score = out['count'].data_ptr(), out['box'].data_ptr(), out['score'].data_ptr()
        d.out_class, d.out_coef, d.out_prior = out['cls'].data_ptr(), out['coef'].data_ptr(), out['prior'].data_ptr()
        d.out_rec = out['rec'].data_ptr()
        with torch.cuda.device(dev):
            s = stream if stream is not None else L.stream_ptr()
            if greedy:
                g = L.DetectGreedyWs()
                g.box_scale = float(active_cfg().max_size)        # detection.py:200: boxes * cfg.max_size
                g.ws = ws['greedy'].data_ptr()
                L.check(L.lib().ymi_detect_traditional_f32(C.byref(d), C.byref(g), s), 'ymi_detect_traditional_f32')
            else:
                L.check(L.lib().ymi_detect_f32(C.byref(d), s), 'ymi_detect_f32')
        out['_keepalive'] = (loc, conf, mask, priors)
        return out

    def __call__(self, predictions, net):
        """predictions: 'loc' [B,P,4], 'conf' [B,P,C] post-softmax (reference contract) or 'conf_logits' (fused
        softmax), 'mask' [B,P,D], 'priors' [P,4], optional 'proto' [B,ph,pw,D]."""
        if 'conf_logits' in predictions and 'conf' not in predictions:
            conf, is_logits = predictions['conf_logits'], True
        else:
            conf, is_logits = predictions['conf'], False
        proto = predictions.get('proto')
        o = self.run_device(predictions['loc'], conf, predictions['mask'], predictions['priors'], is_logits)
        return self.finish(o, proto, net)

    def finish(self, o, proto, net):
        """Fixed-capacity device outputs -> the reference's list of per-image dicts (one host read of the counts)."""
        with _timer_env('Detect'):
            counts = o['count'].tolist()          # the one host sync per batch
            out, pri = [], []
            for b, n in enumerate(counts):
                if n == 0:
                    out.append({'detection': None, 'net': net})
                    pri.append(None)
                    continue
                det = {'box': o['box'][b, :n], 'mask': o['coef'][b, :n], 'class': o['cls'][b, :n],
                       'score': o['score'][b, :n]}
                if proto is not None:
                    det['proto'] = proto[b]
                pri.append(o['prior'][b, :n])
                out.append({'detection': det, 'net': net})
            self.last_prior_idx = pri
        return out
