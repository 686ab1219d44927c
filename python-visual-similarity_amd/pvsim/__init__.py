"""pvsim -- an MI355X-native image-similarity engine with pyvisim's encoder API.

    from pvsim.encoders import VLADEncoder, FisherVectorEncoder, Pipeline, KMeansWeights, GMMWeights
    from pvsim.features import RootSIFT, SIFT, Lambda, DeepConvFeature
    from pvsim import eval                     # retrieve_top_k_similar, top_k_map, top_k_accuracy, rerank_spatial, expand_verified
    from pvsim import verify                   # LocalFeatureIndex, SpatialVerifier, match (spatial re-ranking)
    from pvsim import CompactIndex, ProductQuantizer   # product-quantised index, ADC search (m + 4 bytes per image)
    from pvsim import IVFCompactIndex                  # the same cut into inverted lists: a query scans nprobe of nlist lists
    from pvsim import Int8Index                        # one signed byte per dimension: a quarter of a DeviceIndex, near-exact lists
    from pvsim import IVFInt8Index                     # the same rows cut into inverted lists: the int8 score over nprobe of nlist lists
    from pvsim import QueryExpansion             # query expansion / database-side augmentation on a DeviceIndex
    from pvsim import Diffusion                        # diffusion re-ranking on the kNN graph of a DeviceIndex
    from pvsim import KReciprocal                      # k-reciprocal re-ranking on the kNN lists of a DeviceIndex
    from pvsim import ASMKIndex                        # local-descriptor retrieval: ASMK* with binary signatures, an inverted file
    from pvsim import ASMKExpansion                    # its query expansion: majority-vote signatures and words the results agree on
    from pvsim import find_duplicates                  # near-duplicate groups of a DeviceIndex: cosine threshold join + components
    from pvsim import Subset                           # an allowed set of images: index.rank(q, k, allowed=...) ranks within it

The arithmetic (centroid assignment, VLAD / Fisher aggregation, normalisation, cosine GEMM, top-k) runs in
hand-written HIP kernels for gfx950 behind a C-ABI (include/pvsim.h) bound with ctypes; there is no CPU
fallback.  Importing the package does not touch the GPU; the first computation does.
"""
from .engine import Context, default_context, pack_descriptors
from . import models
from ._errors import CapacityError
from .compact import CompactIndex, IVFCompactIndex, ProductQuantizer
from .quantized import Int8Index
from .ivf_int8 import IVFInt8Index
from .expand import QueryExpansion
from .diffusion import Diffusion
from .reciprocal import KReciprocal
from .asmk import ASMKExpansion, ASMKIndex
from .duplicates import DuplicateGroups, find_duplicates
from .subset import Subset

__version__ = "0.1.0"
__all__ = ["encoders", "features", "eval", "verify", "models", "Context", "default_context", "pack_descriptors", "CapacityError",
           "CompactIndex", "IVFCompactIndex", "ProductQuantizer", "Int8Index", "IVFInt8Index", "QueryExpansion", "Diffusion", "KReciprocal", "ASMKIndex", "ASMKExpansion",
           "DuplicateGroups", "find_duplicates", "Subset"]
