"""Small VOC / COCO fixtures for the file-dataset tests, written at test time (no image data is committed): shapes samples
rendered at a few raw sizes, saved as JPEG, annotated once as a VOC tree and once as a COCO JSON."""
import json
import os

import numpy as np

VOC_NAMES = ['aeroplane', 'bicycle', 'bird']          # shapes class k -> VOC class k (indices 0, 1, 2 of the 20)
COCO_CATS = [11, 3, 7]                                # non-contiguous ids, listed unsorted; sorted: 3 -> 0, 7 -> 1, 11 -> 2


def render(sizes, seed=0):
    """One shapes sample per (h, w) of `sizes`: [(image uint8, boxes [O,4] pixel corners, class_ids [O])]."""
    from data_loaders.shapes import Shapes
    out = []
    for i, (h, w) in enumerate(sizes):
        s = next(iter(Shapes(None, 1, image_size=(h, w), seed=seed + i)))
        out.append((s['image'], np.asarray(s['boxes'], np.float32), np.asarray(s['class_ids'], np.int32)))
    return out


def write_voc(root, samples, subset='trainval', names=None, quality=95, extra_objects=None):
    """VOC tree: JPEGImages/<name>.jpg, Annotations/<name>.xml, ImageSets/Main/<subset>.txt.  Returns the image names."""
    from PIL import Image
    for d in ('JPEGImages', 'Annotations', os.path.join('ImageSets', 'Main')):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    names = names or ['%06d' % i for i in range(len(samples))]
    for name, (image, boxes, ids) in zip(names, samples):
        Image.fromarray(image).save(os.path.join(root, 'JPEGImages', name + '.jpg'), quality=quality)
        objs = ''.join(
            '<object><name>%s</name><difficult>%d</difficult><truncated>0</truncated><bndbox><xmin>%g</xmin><ymin>%g</ymin>'
            '<xmax>%g</xmax><ymax>%g</ymax></bndbox></object>' % (VOC_NAMES[c] if c < len(VOC_NAMES) else c, k % 2, b[1], b[0],
                                                                  b[3], b[2])
            for k, (b, c) in enumerate(zip(boxes, ids)))
        objs += (extra_objects or {}).get(name, '')
        xml = ('<annotation><filename>%s.jpg</filename><size><width>%d</width><height>%d</height><depth>3</depth></size>%s'
               '</annotation>' % (name, image.shape[1], image.shape[0], objs))
        with open(os.path.join(root, 'Annotations', name + '.xml'), 'w') as f:
            f.write(xml)
    with open(os.path.join(root, 'ImageSets', 'Main', subset + '.txt'), 'w') as f:
        f.write(''.join('%s %s\n' % (n, '1') for n in names))
    return names


def write_coco(path, image_dir, samples, names, extra_annotations=(), extra_images=()):
    """COCO JSON over the same images (file_name = <name>.jpg inside image_dir)."""
    sorted_cats = sorted(COCO_CATS)
    images, anns = [], []
    for i, (name, (image, boxes, ids)) in enumerate(zip(names, samples)):
        images.append({'id': 100 + i, 'file_name': name + '.jpg', 'height': int(image.shape[0]), 'width': int(image.shape[1])})
        for b, c in zip(boxes, ids):
            anns.append({'id': len(anns) + 1, 'image_id': 100 + i, 'category_id': sorted_cats[int(c)], 'iscrowd': 0,
                         'bbox': [float(b[1]), float(b[0]), float(b[3] - b[1]), float(b[2] - b[0])]})
    images += list(extra_images)
    for a in extra_annotations:
        anns.append(dict(a, id=len(anns) + 1))
    data = {'images': images, 'annotations': anns,
            'categories': [{'id': c, 'name': VOC_NAMES[sorted_cats.index(c)]} for c in COCO_CATS]}
    with open(path, 'w') as f:
        json.dump(data, f)
    return path
