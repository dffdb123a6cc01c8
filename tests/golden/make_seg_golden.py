"""Writes tests/golden/seg_labels.npz from the reference's own label tables and metrics:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_seg_golden.py [--reference DIR]

The reference modules imported: seg_model.datasets.acdc (ACDCDataset: id_to_train_id, train_id_to_color,
encode_target, decode_target) and seg_model.metrics.stream_metrics (StreamSegMetrics).  stream_metrics imports
sklearn.metrics.confusion_matrix and never uses it; where sklearn (or torchvision, which the dataset module
imports for its transforms) is absent, that one import is served by an empty stub module.  Nothing in the
reference is modified and none of its code is written out: the file holds arrays only.

  id_to_train_id [35] int64, train_id_to_color [20, 3] int64     the reference's tables
  ids [24, 40] uint8        a recorded synthetic id map holding every id 0..33 (never above: the reference
                            raises there)
  encoded [24, 40] int64    encode_target(ids);  decoded [24, 40, 3] int64 = decode_target(a copy of encoded)
  true_k, pred_k (k = 0, 1) two recorded updates: int64 labels with 255, -1, 19 and 1000 mixed in and with
                            classes 3 and 17 absent from labels AND predictions (NaN IoU rows), predictions 0..18
  hist [19, 19] float64     the confusion matrix after both updates
  overall, mean_acc, fwavacc, mean_iu float64 scalars, class_iu [19] float64 (NaN for absent classes)
"""
import argparse
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def _import_or_stub(name: str, attrs=()):
    try:
        importlib.import_module(name)
    except Exception:
        parts = name.split('.')
        for i in range(1, len(parts) + 1):
            sub = '.'.join(parts[:i])
            if sub not in sys.modules:
                sys.modules[sub] = types.ModuleType(sub)
                if i > 1:
                    setattr(sys.modules['.'.join(parts[:i - 1])], parts[i - 1], sys.modules[sub])
        for a in attrs:
            setattr(sys.modules[name], a, None)


def synthetic_ids() -> np.ndarray:
    rng = np.random.default_rng(20261021)
    ids = rng.integers(0, 34, size=(24, 40)).astype(np.uint8)
    ids[0, :34] = np.arange(34, dtype=np.uint8)  # every id at least once
    ids[5:12, 8:30] = 7  # constant regions, as label maps have
    ids[12:20, 3:15] = 26
    return ids


def synthetic_updates():
    rng = np.random.default_rng(7)
    present = np.array([c for c in range(19) if c not in (3, 17)])
    out = []
    for shape in ((2, 16, 24), (1, 9, 13)):
        true = present[rng.integers(0, present.size, size=shape)].astype(np.int64)
        pred = np.where(rng.random(shape) < 0.7, true, present[rng.integers(0, present.size, size=shape)]).astype(np.int64)
        bad = rng.random(shape)
        true[bad < 0.05] = 255
        true[(bad >= 0.05) & (bad < 0.07)] = -1
        true[(bad >= 0.07) & (bad < 0.09)] = 19
        true[(bad >= 0.09) & (bad < 0.10)] = 1000
        out.append((true, pred))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default='/root/reference')
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    _import_or_stub('sklearn.metrics', ('confusion_matrix', ))
    _import_or_stub('torchvision.transforms.functional')
    _import_or_stub('torchvision.transforms')
    from seg_model.datasets.acdc import ACDCDataset
    from seg_model.metrics.stream_metrics import StreamSegMetrics

    out = {'id_to_train_id': np.asarray(ACDCDataset.id_to_train_id, dtype=np.int64),
           'train_id_to_color': np.asarray(ACDCDataset.train_id_to_color, dtype=np.int64)}
    ids = synthetic_ids()
    encoded = np.asarray(ACDCDataset.encode_target(ids))
    out['ids'], out['encoded'] = ids, encoded.astype(np.int64)
    out['decoded'] = np.asarray(ACDCDataset.decode_target(encoded.copy())).astype(np.int64)
    m = StreamSegMetrics(19)
    for k, (true, pred) in enumerate(synthetic_updates()):
        out[f'true_{k}'], out[f'pred_{k}'] = true, pred
        m.update(true, pred)
    with np.errstate(all='ignore'):
        r = m.get_results()
    out['hist'] = np.asarray(m.confusion_matrix, dtype=np.float64)
    out['overall'], out['mean_acc'] = np.float64(r['Overall Acc']), np.float64(r['Mean Acc'])
    out['fwavacc'], out['mean_iu'] = np.float64(r['FreqW Acc']), np.float64(r['Mean IoU'])
    out['class_iu'] = np.array([r['Class IoU'][c] for c in range(19)], dtype=np.float64)
    assert np.isnan(out['class_iu'][[3, 17]]).all() and np.isfinite(np.delete(out['class_iu'], [3, 17])).all()
    path = os.path.join(HERE, 'seg_labels.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
