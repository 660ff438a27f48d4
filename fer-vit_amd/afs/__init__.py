"""AFS (reference `afs/`): the style extractor runs natively; the rest of the package needs third-party
models this project does not contain, and says so when asked for."""
from .style_extractor import HighwayLayer, StyleBlock, StyleExtractor

__all__ = ["StyleExtractor"]

_MISSING = {
    "AFSLoss": "ArcFace (pSp's models.encoders.model_irse Backbone) and LPIPS (criteria.lpips)",
    "GeneratedImageProvider": "the pSp encoder's StyleGAN2 generator",
    "DiskImageProvider": "PIL / torchvision image loading and the pSp image pipeline",
    "PairLatentDataset": "the reference's paired pSp latent files",
}


def __getattr__(name):
    if name in _MISSING:
        raise ImportError(f"afs.{name} is not provided: it needs {_MISSING[name]}, which this project does not "
                          "include. Only afs.StyleExtractor has a native path.")
    raise AttributeError(f"module 'afs' has no attribute {name!r}")
