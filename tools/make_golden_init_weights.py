"""Generate tests/golden/init_weights.json by EXECUTING THE REFERENCE's own Yolact.init_weights on the CPU (build container only).

    python tools/make_golden_init_weights.py          # needs the reference checkout; writes tests/golden/init_weights.json

The reference is imported with the stubs of oracle/make_golden._shim_reference under yolact_resnet50_config with the replacements of
tests/heads_train_ref.golden_cfg_overrides (32 features, 6 classes, max_size 96).  Its Yolact is built, the small backbone file of
tests/train_step_ref.backbone_file_state (legacy `layer*` names, an `fc` pair no backbone has, most of the backbone missing) is written
to a temporary directory, and, after torch.manual_seed(INIT_SEED), init_weights(that file) is called (yolact.py:492-547).  Stored: the
SHA-256 of the bytes of every state-dict tensor outside the backbone, and of the backbone tensors the file holds
(tests/train_step_ref.init_digest_keys).  Digests only: no weights.
"""
from __future__ import annotations

import json
import os
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    from oracle.make_golden import _shim_reference
    _shim_reference()
    from data import cfg, set_cfg
    import heads_train_ref as H
    import train_step_ref as T
    set_cfg('yolact_resnet50_config')
    o = H.golden_cfg_overrides()
    cfg.fpn = cfg.fpn.copy({'num_features': o.pop('num_features')})
    for k, v in o.items():
        setattr(cfg, k, v)
    import yolact as ref_yolact
    net = ref_yolact.Yolact()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'backbone.pth')
        torch.save(T.backbone_file_state(net.backbone), path)
        torch.manual_seed(T.INIT_SEED)
        net.init_weights(path)
    sd = net.state_dict()
    keys = T.init_digest_keys(net)
    out = dict(seed=T.INIT_SEED, file_seed=T.INIT_FILE_SEED, torch=torch.__version__, sha256={k: T.sha256(sd[k]) for k in keys})
    dst = os.path.join(ROOT, 'tests', 'golden', 'init_weights.json')
    with open(dst, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', dst, len(keys), 'digests')


if __name__ == '__main__':
    main()
