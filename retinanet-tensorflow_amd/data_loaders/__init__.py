"""Loader protocol of the reference (data_loaders/base.py:1-11), the synthetic 'shapes' dataset and the Pascal VOC / COCO readers."""
