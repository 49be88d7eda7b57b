"""MI355X (gfx950) MSM / NTT backend for the halo2 hot path of 0xWOLAND/halo2-prover.

Python host layer over the C-ABI library libh2hip.so (include/h2hip.h).  Importing the
package does not touch the GPU; the first compute call (or `init()`) binds the process to
one device.  There is no CPU fallback.
"""
from .api import (Bases, ParamsKZG, base_sqrt_device, best_fft, best_fft_batch, best_fft_group, best_multiexp, g_to_lagrange,  # noqa: F401
                  generate_proofs, init, msm_points, msm_points_device, msm_points_plan, ntt_device, params_downsize,
                  pasta_points_decompress_device, points_decompress_device, verify_proofs)
from .expr import ExprProgram  # noqa: F401
from . import ipa  # noqa: F401
from .ipa import ParamsIPA, compute_b, compute_s, verify_proofs_bytes  # noqa: F401
from .lookup import lookup_product, permute_expression_pair  # noqa: F401
from .opening import gwc_open, poly_lincomb, shplonk_open_final, shplonk_open_h  # noqa: F401
from .permutation import permutation_product  # noqa: F401
from . import poseidon  # noqa: F401
from .transcript import Blake2bMidstate, Blake2bTranscript  # noqa: F401
from .lib import CURVES, H2Error, LIB_PATH, SYMBOLS, load  # noqa: F401
