from ._features import SIFT, RootSIFT, DenseSIFT, DenseRootSIFT, DeepConvFeature, Lambda

__all__ = ["SIFT", "RootSIFT", "DenseSIFT", "DenseRootSIFT", "DeepConvFeature", "Lambda"]
