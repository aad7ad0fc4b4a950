"""COCO-format reader (reference data_loaders/coco.py) on the annotation JSON alone (no pycocotools): class ids are the
category ids in sorted order; crowd annotations (iscrowd = 1) are excluded, as getAnnIds(iscrowd=False) does; boxes with
width < 1 or height < 1 are dropped; bbox [x, y, w, h] becomes [y, x, y + h, x + w]; images keep the JSON's order.  The
samples also carry 'image_size' (h, w) from the image entry's height / width.  Epoch order, sharding and resume:
data_loaders/files.py."""
import collections
import json
import os

import numpy as np

from data_loaders.files import FileDataset


class COCO(FileDataset):
    def __init__(self, ann_path, dataset_path):
        super(COCO, self).__init__()
        self._dataset_path = dataset_path
        with open(ann_path) as f:
            data = json.load(f)
        cats = {c['id']: c['name'] for c in data.get('categories', [])}
        self._category_ids = sorted(cats)
        self._class_names = [cats[i] for i in self._category_ids]
        index = {c: i for i, c in enumerate(self._category_ids)}
        anns = collections.defaultdict(list)
        for a in data.get('annotations', []):
            if not a.get('iscrowd', 0):
                anns[a['image_id']].append(a)
        records = []
        for image in data.get('images', []):
            boxes, class_ids = [], []
            for a in anns.get(image['id'], []):
                left, top, width, height = a['bbox']
                if height < 1 or width < 1:                        # some boxes have no width / height
                    continue
                boxes.append([top, left, top + height, left + width])
                class_ids.append(index[a['category_id']])
            records.append({'image_file': os.path.join(dataset_path, image['file_name']),
                            'boxes': np.array(boxes, np.float32).reshape(-1, 4),
                            'class_ids': np.array(class_ids, np.int32).reshape(-1),
                            'image_size': (int(image['height']), int(image['width']))})
        self._keep(records)
