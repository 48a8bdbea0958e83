"""Architecture registry mirroring /root/reference/code/archs/__init__.py: the reference
builds a net with ``archs.__dict__[config.arch](config)`` (cluster_sobel.py:140)."""
from .cluster import ClusterNet5g, ClusterNet5gTwoHead  # noqa: F401
from .seg import SegmentationNet10a, SegmentationNet10aFeatures, SegmentationNet10aTwoHead  # noqa: F401
from .seg_baselines import SegmentationNet10aDoersch, SegmentationNet10aIsola  # noqa: F401
from .triplets import TripletsNet5g, TripletsNet6c  # noqa: F401
from .vgg import ClusterNet6c, ClusterNet6cTwoHead  # noqa: F401

__all__ = ["ClusterNet5g", "ClusterNet5gTwoHead", "ClusterNet6c", "ClusterNet6cTwoHead",
           "SegmentationNet10a", "SegmentationNet10aDoersch", "SegmentationNet10aFeatures", "SegmentationNet10aIsola",
           "SegmentationNet10aTwoHead", "TripletsNet5g", "TripletsNet6c"]
