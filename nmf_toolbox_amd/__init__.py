"""nmf_toolbox_amd -- MI355X-native drop-in for the multiplicative-update hot path of colinvaz/nmf-toolbox.

Only the path named by BASELINE.json's north_star lives here: nmf / cnmf / nmfsc (+ the two helpers
they call), the further toolbox functions lnmf / cnmfsc / constrainednmf / SortDictionary, and cmfwisa (complex NMF with
intra-source additivity: complex V, one phase matrix per source), seminmf (semi-NMF of mixed-sign V) nmf_batch / cnmf_batch (many small nmf / cnmf problems in one call) wnmf / wcnmf (nmf / cnmf with per-entry weights, for missing or unreliable data) and wnmf_batch / wcnmf_batch (many small wnmf / wcnmf problems in one call), and softmask / softmask_batch (per-source Wiener-style masks from W and H, applied to a mixture in one fused pass), and impute / holdout with impute_batch / holdout_batch (the masked entries of a weighted fit filled from W and H, and scored, in one fused pass), behind the C ABI of include/nmfx.h (libnmfx.so, hand-written HIP for gfx950).
"""
from .toolbox import ReconstructFromDecomposition, SortDictionary, cmfwisa, cnmf, cnmf_batch, constrainednmf, cnmfsc, lnmf, nmf, nmf_batch, nmfsc, projfunc, reconstruct_from_decomposition, seminmf, softmask, softmask_batch, impute, impute_batch, holdout, holdout_batch, wcnmf, wcnmf_batch, wnmf, wnmf_batch  # noqa: F401
from ._lib import NmfxError, device_count  # noqa: F401

__all__ = ["nmf", "nmf_batch", "cnmf", "cnmf_batch", "nmfsc", "cnmfsc", "lnmf", "constrainednmf", "cmfwisa", "seminmf", "wnmf", "wcnmf", "wnmf_batch", "wcnmf_batch", "softmask", "softmask_batch", "impute", "impute_batch", "holdout", "holdout_batch", "SortDictionary", "ReconstructFromDecomposition", "reconstruct_from_decomposition", "projfunc", "NmfxError", "device_count"]
