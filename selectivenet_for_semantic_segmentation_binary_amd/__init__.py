"""MI355X-native SelectiveUNet_B training path.

Drop-in replacements for the reference's hot path (yellofi/SelectiveNet_for_semantic_segmentation_binary):

* `UNet_B`, `CBR_2D`                    <- model.py:9-103
* `UNet` (CE variant)                   <- model.py:105-191
* `calc_selective_risk_image_b`         <- selective_loss.py:58-85
* `calc_selective_risk_image`           <- selective_loss.py:24-56
* `BCEWithLogitsLoss`                   <- torch.nn.BCEWithLogitsLoss (train.py:78)
* `CrossEntropyLoss`                    <- torch.nn.CrossEntropyLoss (train.py:80)
* `Adam`                                <- torch.optim.Adam (train.py:90)
* `SelectiveSweep`                       risk-coverage sweep of eval.py's --s_cut_off in one pass
* `PatchReport`                          per-patch counts, get_performance metrics and exact ROC AUC
                                        <- utils/compute_metric.py:93-148 (unused there)
* `BoundaryReport`,                      errors and rejections by distance to the label contour, Hausdorff distance
  `boundary_distance_sq`                 per patch; the exact Euclidean distance transform on the device
* `predict_image`, `TilePlan`             whole-image prediction: tiles gathered and stitched on the device,
                                        optionally averaged over the image's flips / D4 orientations (tta=)
* `label_regions`, `region_table`,       connected regions of a prediction mask, their exact table and the
  `clean_mask`                           small-region / hole clean-up, on the device (predict_image(regions=...))
* `tissue_plane`                         the glass / tissue mask of an image; predict_image(tissue=True) does not
                                        forward tiles without tissue and counts tumor over tissue
* `stain`, `StainFit`, `MACENKO_TARGET`  Macenko stain normalisation on the device: stain.fit / fit_many / normalize;
                                        predict_image(stain=target) normalises the image before it is tiled
* `parallel.init_data_parallel`        <- torch.nn.DataParallel (train.py:131-134)

All compute runs in libselunet.so (HIP, gfx950); there is no CPU fallback.
"""
from .layout import count_params, state_dict_keys  # noqa: F401
from .metrics import BoundaryReport, PatchReport, SelectiveSweep, boundary_distance_sq  # noqa: F401
from .model import CBR_2D, UNet, UNet_B  # noqa: F401
from .optim import Adam  # noqa: F401
from .predict import TilePlan, clean_mask, label_regions, predict_image, region_table, tissue_plane  # noqa: F401
from .selective_loss import (BCEWithLogitsLoss, CrossEntropyLoss, calc_selective_risk_image,  # noqa: F401
                             calc_selective_risk_image_b)
from .stain import MACENKO_TARGET, StainFit  # noqa: F401
from . import parallel, stain  # noqa: F401

__version__ = "0.1.0"
