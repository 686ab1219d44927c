from ._features import SIFT, RootSIFT, DenseSIFT, DenseRootSIFT, KeypointSIFT, KeypointRootSIFT, DeepConvFeature, Lambda

__all__ = ["SIFT", "RootSIFT", "DenseSIFT", "DenseRootSIFT", "KeypointSIFT", "KeypointRootSIFT", "DeepConvFeature", "Lambda"]
