"""Traditional (greedy per-class) NMS on the MI355X (csrc/detect_greedy.hip): known answers, stage-isolated parity with the
reference-executed fixture, and the end-to-end paths (forward, forward_device, BatchPipeline, YOLACT_AMD_GRAPH)."""
import os

import numpy as np
import pytest
import torch

import traditional_nms_ref as T

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MIN_DECIDABLE = 3        # decidable images of the fixture (r50_sparse: 1, r50_few: 2), all index-exact


def _detect(conf_thresh=0.05, nms_thresh=0.5):
    from yolact_amd.layers.detection import Detect
    d = Detect(2, 0, 200, conf_thresh, nms_thresh)
    d.traditional_nms_on_device = True
    return d


class _max_size:
    """Pixel scale 64 for the known-answer inputs: boxes on a 1/64 grid decode and scale exactly (integer pixels)."""
    def __enter__(self):
        import yolact_amd
        yolact_amd.set_cfg('yolact_resnet50_config')
        from yolact_amd.config import active_cfg
        self.cfg = active_cfg()
        self.old = self.cfg.max_size
        self.cfg.max_size = 64
        return self

    def __exit__(self, *a):
        self.cfg.max_size = self.old


def _run_pixel_boxes(boxes, scores, det=None):
    """One image, one foreground class: integer pixel boxes [n,4] (max_size 64), scores [n] -> (device output, host reference)."""
    boxes = torch.as_tensor(boxes, dtype=torch.float32)
    scores = torch.as_tensor(scores, dtype=torch.float32)
    n = boxes.shape[0]
    rel = boxes / 64
    priors = torch.stack([(rel[:, 0] + rel[:, 2]) / 2, (rel[:, 1] + rel[:, 3]) / 2, rel[:, 2] - rel[:, 0], rel[:, 3] - rel[:, 1]], 1)
    conf = torch.stack([1 - scores, scores], 1)[None]
    loc = torch.zeros(1, n, 4)
    mask = torch.arange(n, dtype=torch.float32)[None, :, None].repeat(1, 1, 4)
    det = det or _detect()
    with torch.no_grad():
        out = det({'loc': loc.to(DEV), 'conf': conf.to(DEV), 'mask': mask.to(DEV), 'priors': priors.to(DEV)}, None)
    torch.cuda.synchronize()
    ref = T.detect_image(conf[0], loc[0], mask[0], priors, det.conf_thresh, det.nms_thresh, 100, 64)
    return out[0]['detection'], det.last_prior_idx[0], ref


def _priors_of(out_prior):
    return [int(v) for v in out_prior.cpu()]


def test_chain_suppressed_box_suppresses_nothing():
    """(a) A suppresses B, B would suppress C, C survives: greedy keeps A and C (Fast NMS drops C)."""
    with _max_size():
        g, pri, ref = _run_pixel_boxes([[0, 0, 19, 9], [5, 0, 24, 9], [10, 0, 29, 9]], [.9, .8, .7])
    assert _priors_of(pri) == [0, 2] == ref['prior'].tolist()
    assert g['score'].cpu().tolist() == pytest.approx([.9, .7])
    assert torch.equal(g['box'].cpu(), ref['box'])
    assert torch.equal(g['mask'].cpu()[:, 0], torch.tensor([0., 2.]))
    assert g['class'].cpu().tolist() == [0, 0]


def test_overlap_equal_to_threshold_suppresses():
    """(b) overlap exactly nms_thresh under the +1 convention: suppressed (>=)."""
    with _max_size():
        _, pri, ref = _run_pixel_boxes([[0, 0, 9, 9], [0, 0, 9, 4]], [.9, .8])
    assert _priors_of(pri) == [0] == ref['prior'].tolist()


def test_plus_one_convention_decides():
    """(c) overlap 0.444 without the +1, 0.5625 with it: suppressed."""
    with _max_size():
        _, pri, ref = _run_pixel_boxes([[0, 0, 3, 3], [0, 0, 2, 2]], [.9, .8])
    assert _priors_of(pri) == [0] == ref['prior'].tolist()


def test_no_top_k_cap():
    """(d) 250 candidates of one class, the best 200 one cluster: greedy returns detections ranked beyond 200."""
    boxes = [[0, 0, 31, 31]] * 200 + [[8 * (i % 8), 34 + 4 * (i // 8), 8 * (i % 8) + 3, 37 + 4 * (i // 8)] for i in range(50)]
    scores = [0.9 - 1e-3 * i for i in range(200)] + [0.5 - 1e-3 * i for i in range(50)]
    with _max_size():
        _, pri, ref = _run_pixel_boxes(boxes, scores)
    p = _priors_of(pri)
    assert p == ref['prior'].tolist()
    assert p[0] == 0 and len(p) > 1 and min(p[1:]) >= 200


def test_large_k_global_path():
    """(e) one class with K = P = 6000 candidates (> the 4096 keys held in LDS): index-exact against the host statement."""
    rng = np.random.default_rng(3)
    n = 6000
    xy = rng.integers(0, 56, (n, 2))
    wh = rng.integers(1, 9, (n, 2))
    boxes = np.concatenate([xy, np.minimum(xy + wh, 63)], 1)
    scores = 0.1 + 0.8 * rng.permutation(n) / n
    with _max_size():
        g, pri, ref = _run_pixel_boxes(boxes, scores)
    assert _priors_of(pri) == ref['prior'].tolist()
    assert torch.equal(g['box'].cpu(), ref['box'])
    assert torch.equal(g['score'].cpu(), ref['score'])


def test_no_candidates_is_none():
    """(f) no score above conf_thresh: None, as the reference."""
    with _max_size():
        g, pri, ref = _run_pixel_boxes([[0, 0, 9, 9], [20, 20, 29, 29]], [.04, .01])
    assert g is None and pri is None and ref is None


def _parity(name):
    from yolact_amd.layers.detection import Detect
    import yolact_amd
    from helpers import oracle_run
    m, _ = T.case(name)
    _, _, cfg, _, raw, _ = oracle_run(m['source'])
    yolact_amd.set_cfg(m['config'])
    det = Detect(cfg.num_classes, 0, cfg.nms_top_k, m['conf_thresh'], m['nms_thresh'])
    det.traditional_nms_on_device = True
    det.use_cross_class_nms = m['cross_class']
    with torch.no_grad():
        out = det({'loc': raw['loc'].to(DEV), 'conf': raw['conf'].to(DEV), 'mask': raw['mask'].to(DEV),
                   'priors': raw['priors'].to(DEV)}, None)
    torch.cuda.synchronize()
    ndec = 0
    for b, im in enumerate(m['images']):
        ref = T.golden_image(name, b)
        g = out[b]['detection']
        if ref is None:
            assert g is None
            continue
        assert g is not None and g['score'].shape[0] == ref['score'].shape[0]
        sc = g['score'].cpu()
        assert bool((sc[:-1] >= sc[1:]).all())
        if im['decidable']:
            ndec += 1
            assert T.tie_groups_equal(det.last_prior_idx[b].cpu(), g['class'].cpu(), ref['prior'], ref['class'], ref['score'])
            assert (sc - ref['score']).abs().max().item() <= 1e-4
            assert (g['box'].cpu() - ref['box']).abs().max().item() <= 1e-4
            assert (g['mask'].cpu() - ref['mask']).abs().max().item() <= 1e-4
    return ndec


def test_stage_isolated_parity_with_reference_fixture():
    """The oracle's head outputs through the device path: every decidable image of the reference-executed fixture index-exact,
    values within 1e-4; every image the same count and sorted scores."""
    ndec = sum(_parity(n) for n in ('r50_dense', 'r50_sparse', 'r50_few', 'im700', 'plus_r50', 'r50_cc'))
    assert ndec >= MIN_DECIDABLE


def test_stage_isolated_large_k_case_runs():
    """r50_largek: every prior a candidate of every class (K = P = 19 248, all 80 classes on the global-memory path)."""
    _parity('r50_largek')


def test_end_to_end_paths_agree():
    """Yolact.forward in greedy mode on r50_dense matches the fixture's counts and the host statement on the device's own head
    outputs; forward_device, BatchPipeline(depth=2) and YOLACT_AMD_GRAPH=1 return the same records bit for bit."""
    from gpu_utils import build_net
    from helpers import case_images, load_golden
    from yolact_amd import parallel
    from yolact_amd.pipeline import BatchPipeline
    meta, _ = load_golden('r50_dense')
    net = build_net(meta)
    net.detect.use_fast_nms = False
    net.detect.traditional_nms_on_device = True
    x = case_images(meta).to(DEV)
    with torch.no_grad():
        preds = net(x)
        raw = net.forward_raw(x)
        eager = parallel.pack_records(net.forward_device(x)).clone()
        torch.cuda.synchronize()
        cfg = net.cfg
        m, _ = T.case('r50_dense')
        for b in range(x.shape[0]):
            g = preds[b]['detection']
            ref = T.golden_image('r50_dense', b)
            assert g['score'].shape[0] == ref['score'].shape[0] == m['images'][b]['n']
            conf = torch.softmax(raw['conf_logits'][b].float().cpu(), -1)
            host = T.detect_image(conf, raw['loc'][b].cpu(), raw['mask'][b].cpu(), raw['priors'].cpu(), cfg.nms_conf_thresh,
                                  cfg.nms_thresh, cfg.max_num_detections, cfg.max_size)
            common = set(zip(net.detect.last_prior_idx[b].cpu().tolist(), g['class'].cpu().tolist())) & \
                set(zip(host['prior'].tolist(), host['class'].tolist()))
            assert len(common) >= 0.9 * len(host['prior'])
            assert (g['score'].cpu()[:10] - host['score'][:10]).abs().max().item() <= 1e-4
        pipe = BatchPipeline(net, 2)
        pipe.warm(x)
        outs = [pipe.submit(x) for _ in range(3)]
        recs = []
        for o in outs:
            o['done'].synchronize()
            recs.append(parallel.pack_records(o).clone())
        pipe.synchronize()
        for r in recs:
            assert torch.equal(r, eager)
        os.environ['YOLACT_AMD_GRAPH'] = '1'
        try:
            g1 = parallel.pack_records(net.forward_device(x)).clone()
            g2 = parallel.pack_records(net.forward_device(x)).clone()
            net.detect.use_fast_nms = True                 # another NMS mode must not replay the greedy graph
            gf = net.forward_device(x)
            torch.cuda.synchronize()
        finally:
            os.environ.pop('YOLACT_AMD_GRAPH', None)
        assert torch.equal(g1, eager) and torch.equal(g2, eager)
        fast = net.forward_device(x)
        torch.cuda.synchronize()
        assert torch.equal(gf['count'], fast['count'])
