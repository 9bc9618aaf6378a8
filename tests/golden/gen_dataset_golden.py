#!/usr/bin/env python3
"""Generate tests/golden/datasets.pt from the REFERENCE's dataset classes, run where the reference tree is mounted.

Producers of the expected values: datasets/s3dis.py `_S3DISDataset`, datasets/shapenet.py `_ShapeNetDataset`,
datasets/kitti/frustum.py `_FrustumKittiDataset` (their `__getitem__`) and torch's `default_collate`.  Tiny synthetic splits are written
to a temporary directory (pickles for Frustum-KITTI, text files for ShapeNet; for S3DIS a stand-in `h5py` module whose `File` returns
the arrays).  `np.random.choice` / `random` / `randn` are wrapped to RECORD every draw while `__getitem__` runs; the wrapper plants a
few values (|z| > 5 so the jitter clip is exercised, flip draws on both sides of 0.5 and one exactly 0.5).  Saved: the inputs, the
draws and the collated outputs.  Nothing of pvcnn_amd takes part in producing the expected values.
Run:  python tests/golden/gen_dataset_golden.py [reference root]     (rewrites datasets.pt)
"""
import importlib
import json
import os
import pickle
import sys
import tempfile
import types

import numpy as np
import torch
from torch.utils.data import default_collate

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else '/root/reference'
SEED = 1588147245

H5_FILES = {}          # path -> {'data', 'label_seg', 'data_num'}


def _stand_in_h5py():
    fake = types.ModuleType('h5py')
    fake.File = lambda name, mode='r': H5_FILES[name]
    return fake


class Recorder:
    """Wraps numpy's global draws: records them per item and plants the listed values."""

    def __init__(self):
        self.real = (np.random.choice, np.random.random, np.random.randn)
        self.flips = [0.7, 0.2, 0.5, 0.93, 0.5000001, 0.01]
        self.reset()

    def reset(self):
        self.choice, self.random, self.randn = [], [], []

    def __enter__(self):
        def choice(a, size=None, replace=True):
            c = self.real[0](a, size, replace=replace)
            self.choice.append(np.asarray(c).copy())
            return c

        def random():
            v = self.flips.pop(0) if self.flips else self.real[1]()
            self.random.append(float(v))
            return v

        def randn(*shape):
            z = self.real[2](*shape)
            if shape:
                z[0, 0], z[1, 1], z[2, -1] = 7.3, -6.1, 5.0
            self.randn.append(np.array(z, dtype=np.float64))
            return z
        np.random.choice, np.random.random, np.random.randn = choice, random, randn
        return self

    def __exit__(self, *exc):
        np.random.choice, np.random.random, np.random.randn = self.real


def run_items(ds, indices, rec):
    """[ds[i] for i in indices], collated, with the draws of every item."""
    draws, items = [], []
    with rec:
        for i in indices:
            rec.reset()
            items.append(ds[i])
            draws.append((rec.choice, rec.random, rec.randn))
    return default_collate(items), draws


def s3dis_cases(root, rng, rec):
    s3dis = importlib.import_module('datasets.s3dis')
    scene = os.path.join(root, 'Area_5', 'office_1')
    os.makedirs(scene)
    P, N = 48, 16
    nums = {'zero': [5, 16, 40], 'half': [1, 48, 17]}
    all_data, all_label, all_num = [], [], []
    for split in ('zero', 'half'):                   # the order the reference lists them in
        w = len(nums[split])
        data = rng.rand(w, P, 9).astype(np.float32) * 3
        label = rng.randint(0, 13, size=(w, P)).astype(np.uint8)
        num = np.array(nums[split], dtype=np.int32)
        H5_FILES[os.path.join(scene, f'{split}_0.h5')] = {'data': data, 'label_seg': label, 'data_num': num}
        all_data.append(data); all_label.append(label); all_num.append(num)
    out = {'data': torch.from_numpy(np.concatenate(all_data)), 'label_seg': torch.from_numpy(np.concatenate(all_label)),
           'data_num': torch.from_numpy(np.concatenate(all_num)), 'num_points': N, 'cases': []}
    for with_norm in (True, False):
        ds = s3dis._S3DISDataset(root, N, split='test', with_normalized_coords=with_norm, holdout_area=5)
        indices = [0, 1, 2, 3, 4, 5, 2, 3]
        (features, targets), draws = run_items(ds, indices, rec)
        out['cases'].append({'with_normalized_coords': with_norm, 'indices': indices,
                             'choices': torch.from_numpy(np.stack([d[0][0] for d in draws]).astype(np.int32)),
                             'features': features, 'targets': targets})
    return out


def shapenet_cases(root, rng, rec):
    shapenet = importlib.import_module('datasets.shapenet')
    N = 24
    dirs = [('Airplane', '02691156'), ('Bag', '02773838'), ('Cap', '02954340'), ('Table', '04379243')]
    with open(os.path.join(root, 'synsetoffset2category.txt'), 'w') as f:
        for name, d in dirs:
            f.write(f'{name}\t{d}\n')
    os.makedirs(os.path.join(root, 'train_test_split'))
    lists = {'train': [], 'val': [], 'test': []}
    clouds, shape_ids = [], []
    for i, n in enumerate([30, 24, 7, 55, 41]):
        sid = i % len(dirs)
        d = dirs[sid][1]
        os.makedirs(os.path.join(root, d), exist_ok=True)
        cloud = np.concatenate([rng.randn(n, 3) * 0.4 + 0.2, rng.randn(n, 3), rng.randint(0, 50, size=(n, 1))], axis=1)
        path = os.path.join(root, d, f'item{i}.txt')
        np.savetxt(path, cloud, fmt='%.6f')
        lists['train' if i < 3 else 'val'].append(f'shape_data/{d}/item{i}')
        clouds.append(torch.from_numpy(np.loadtxt(path)))              # what the reference reads back
        shape_ids.append(sid)
    for s, names in lists.items():
        with open(os.path.join(root, 'train_test_split', f'shuffled_{s}_file_list.json'), 'w') as f:
            json.dump(names, f)
    out = {'clouds': clouds, 'shape_ids': shape_ids, 'num_points': N, 'cases': []}
    for with_normal in (True, False):
        for with_hot in (True, False):
            for jitter in (True, False):
                ds = shapenet._ShapeNetDataset(root, N, split='train', with_normal=with_normal, with_one_hot_shape_id=with_hot,
                                               normalize=True, jitter=jitter)
                assert [sid for _, sid in ds.file_paths] == shape_ids
                indices = [0, 1, 2, 3, 4, 2]
                (features, targets), draws = run_items(ds, indices, rec)
                out['cases'].append({'with_normal': with_normal, 'with_one_hot_shape_id': with_hot, 'normalize': True, 'jitter': jitter,
                                     'indices': indices, 'choices': torch.from_numpy(np.stack([d[0][0] for d in draws]).astype(np.int32)),
                                     'jitter_draws': torch.from_numpy(np.stack([d[2][0] for d in draws])) if jitter else None,
                                     'features': features, 'targets': targets})
    ds = shapenet._ShapeNetDataset(root, N, split='train', with_normal=True, with_one_hot_shape_id=False, normalize=False, jitter=False)
    indices = [4, 0]
    (features, targets), draws = run_items(ds, indices, rec)
    out['cases'].append({'with_normal': True, 'with_one_hot_shape_id': False, 'normalize': False, 'jitter': False, 'indices': indices,
                         'choices': torch.from_numpy(np.stack([d[0][0] for d in draws]).astype(np.int32)), 'jitter_draws': None,
                         'features': features, 'targets': targets})
    return out


def frustum_cases(root, rng, rec):
    frustum = importlib.import_module('datasets.kitti.frustum')
    kitti = importlib.import_module('datasets.kitti.attributes').kitti_attributes
    N = 32
    names = ['Car', 'Pedestrian', 'Cyclist', 'Car', 'Cyclist', 'Pedestrian']
    counts = [10, 80, 32, 1, 45, 33]
    w = len(names)
    clouds = [np.concatenate([rng.randn(n, 3) * [2, 1, 5] + [0, 1, 20], rng.rand(n, 1)], axis=1).astype(np.float32) for n in counts]
    masks = [rng.randint(0, 2, size=n).astype(np.float64) for n in counts]
    boxes = [rng.randn(8, 3) * 1.5 + [1, 1, 20] for _ in range(w)]
    headings = [np.float64(x) for x in rng.uniform(-np.pi, np.pi, size=w)]
    sizes = [kitti.class_name_to_size_template[c] + rng.randn(3) * 0.2 for c in names]
    angles = [np.float64(x) for x in rng.uniform(-2.0, -1.0, size=w)]
    probs = [float(x) for x in rng.rand(w)]
    ids, boxes_2d = list(range(w)), [np.array([0., 0., 10., 10.])] * w
    with open(os.path.join(root, 'frustum_carpedcyc_train.pickle'), 'wb') as fp:
        for obj in (ids, boxes_2d, boxes, clouds, masks, names, headings, sizes, angles):
            pickle.dump(obj, fp)
    with open(os.path.join(root, 'frustum_carpedcyc_val_rgb_detection.pickle'), 'wb') as fp:
        for obj in (ids, boxes_2d, clouds, names, angles, probs):
            pickle.dump(obj, fp)
    classes = ('Car', 'Pedestrian', 'Cyclist')
    template_id = {cat: cls for cls, cat in enumerate(kitti.class_names)}
    out = {'point_clouds': [torch.from_numpy(c) for c in clouds], 'mask_logits': [torch.from_numpy(m) for m in masks],
           'boxes_3d': [torch.from_numpy(b) for b in boxes], 'heading_angles': [float(h) for h in headings], 'sizes': [torch.from_numpy(s) for s in sizes],
           'class_names': names, 'frustum_rotation_angles': [float(a) for a in angles], 'probs': probs, 'num_points': N, 'classes': classes,
           'num_heading_angle_bins': 12, 'class_name_to_size_template_id': template_id,
           'size_templates': {c: torch.from_numpy(kitti.class_name_to_size_template[c]) for c in classes}, 'cases': [], 'rgb_cases': []}
    indices = [0, 1, 2, 3, 4, 5, 1, 2]
    for rotate in (False, True):
        for flip in (False, True):
            for shift in (False, True):
                rec.flips = [0.7, 0.2, 0.5, 0.93, 0.5000001, 0.01]
                ds = frustum._FrustumKittiDataset(root, N, 'train', classes, 12, template_id, random_flip=flip, random_shift=shift,
                                                  frustum_rotate=rotate)
                (inputs, targets), draws = run_items(ds, indices, rec)
                out['cases'].append({'frustum_rotate': rotate, 'random_flip': flip, 'random_shift': shift, 'indices': indices,
                                     'choices': torch.from_numpy(np.stack([d[0][0] for d in draws]).astype(np.int32)),
                                     'flip': torch.tensor([d[1][0] for d in draws], dtype=torch.float64) if flip else None,
                                     'shift': torch.tensor([float(d[2][0]) for d in draws], dtype=torch.float64) if shift else None,
                                     'inputs': inputs, 'targets': targets})
    for rotate in (False, True):
        ds = frustum._FrustumKittiDataset(root, N, 'val', classes, 12, template_id, from_rgb_detection=True, frustum_rotate=rotate)
        (inputs, targets), draws = run_items(ds, indices, rec)
        out['rgb_cases'].append({'frustum_rotate': rotate, 'indices': indices,
                                 'choices': torch.from_numpy(np.stack([d[0][0] for d in draws]).astype(np.int32)),
                                 'inputs': inputs, 'targets': targets})
    return out


def main():
    sys.modules['h5py'] = _stand_in_h5py()
    sys.path.insert(0, REF)
    rng = np.random.RandomState(SEED)
    np.random.seed(SEED)
    rec = Recorder()
    golden = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, fn in (('s3dis', s3dis_cases), ('shapenet', shapenet_cases), ('frustum', frustum_cases)):
            root = os.path.join(tmp, name)
            os.makedirs(root)
            golden[name] = fn(root, rng, rec)
    path = os.path.join(HERE, 'datasets.pt')
    torch.save(golden, path)
    print(f'wrote {path}: {os.path.getsize(path)} bytes')


if __name__ == '__main__':
    main()
