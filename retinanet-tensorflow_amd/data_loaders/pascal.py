"""Pascal VOC reader (reference data_loaders/pascal.py): ImageSets/Main/<subset>.txt names the images (first token of a
line), JPEGImages/<name>.jpg is the image, Annotations/<name>.xml its objects.  Every <object> is kept, `difficult` and
`truncated` ones included; a box is [ymin, xmin, ymax, xmax] exactly as the XML writes it (no 1-based shift); the class id
is the name's index in the fixed list of 20.  The samples also carry 'image_size' (h, w) from the XML's <size>.
Epoch order, sharding and resume: data_loaders/files.py."""
import os
import xml.etree.ElementTree as ET

import numpy as np

from data_loaders.files import FileDataset

CLASS_NAMES = [
    'aeroplane', 'bicycle', 'bird', 'boat', 'bottle', 'bus', 'car', 'cat', 'chair', 'cow', 'diningtable', 'dog',
    'horse', 'motorbike', 'person', 'pottedplant', 'sheep', 'sofa', 'train', 'tvmonitor'
]


class Pascal(FileDataset):
    def __init__(self, path, subset):
        super(Pascal, self).__init__()
        self._path = path
        self._subset = subset
        self._class_names = list(CLASS_NAMES)
        with open(os.path.join(path, 'ImageSets', 'Main', subset + '.txt')) as f:
            names = [line.strip().split()[0] for line in f if line.strip()]
        self._keep(self._read(name) for name in names)

    def _read(self, name):
        xml_file = os.path.join(self._path, 'Annotations', name + '.xml')
        root = ET.parse(xml_file).getroot()
        boxes, class_ids = [], []
        for obj in root.iter('object'):
            label = obj.find('name').text.strip()
            if label not in self._class_names:
                raise ValueError('%s: unknown class name %r' % (xml_file, label))
            boxes.append([float(obj.find('bndbox/' + k).text) for k in ('ymin', 'xmin', 'ymax', 'xmax')])
            class_ids.append(self._class_names.index(label))
        size = root.find('size')
        h, w = int(float(size.find('height').text)), int(float(size.find('width').text))
        return {'image_file': os.path.join(self._path, 'JPEGImages', name + '.jpg'),
                'boxes': np.array(boxes, np.float32).reshape(-1, 4), 'class_ids': np.array(class_ids, np.int32).reshape(-1),
                'image_size': (h, w)}
