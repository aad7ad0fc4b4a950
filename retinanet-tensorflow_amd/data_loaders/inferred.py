"""Dataset by name (reference data_loaders/inferred.py): Inferred('pascal', [root, subset]), Inferred('coco', [ann_json,
images_dir]), Inferred('shapes', [path, num_samples, size]).

The reference asserts that every sample has at least one box, as many boxes as class ids and y1 < y2, x1 < x2.  Here such a
sample is SKIPPED and counted in `skipped` instead -- the one deliberate deviation: a COCO image whose boxes were all dropped,
or a zero-width VOC box, would otherwise end a run.  For the file readers the check runs once over the parsed records, before
any epoch order is computed, so the order, sharding and `skip` arithmetic of data_loaders/files.py see only valid records."""
import numpy as np


def valid(sample):
    boxes, ids = np.asarray(sample['boxes']).reshape(-1, 4), np.asarray(sample['class_ids']).reshape(-1)
    if not boxes.shape[0] == ids.shape[0] != 0:
        return False
    return bool(np.all(boxes[:, :2] < boxes[:, 2:]))


class Inferred(object):
    def __init__(self, type, args):
        self.skipped = 0
        if type == 'coco':
            from data_loaders.coco import COCO
            self._dl = COCO(*args)
        elif type == 'pascal':
            from data_loaders.pascal import Pascal
            self._dl = Pascal(*args)
        elif type == 'shapes':
            from data_loaders.shapes import Shapes
            self._dl = Shapes(args[0], int(args[1]), (int(args[2]), int(args[2])))
        else:
            raise ValueError('unknown dataset type: {}'.format(type))
        self.type = type
        if hasattr(self._dl, 'records'):
            keep = [r for r in self._dl.records if valid(r)]
            self.skipped = len(self._dl.records) - len(keep)
            self._dl._keep(keep)
            self._dl.skipped = self.skipped

    @property
    def loader(self):
        return self._dl

    @property
    def class_names(self):
        return self._dl.class_names

    @property
    def num_classes(self):
        return self._dl.num_classes

    def configure(self, **kw):
        """data_loaders/files.py FileDataset.configure (file readers only); returns self."""
        self._dl.configure(**kw)
        return self

    def __getattr__(self, name):                     # configure / skip / epoch_length / max_objects / max_image_pixels / ...
        if name.startswith('_'):
            raise AttributeError(name)
        return getattr(self._dl, name)

    def __iter__(self):
        for x in self._dl:
            if not valid(x):
                self.skipped += 1
                continue
            yield x
