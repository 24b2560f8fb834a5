"""Import shim: the package directory is `mini-stark_amd/` (not a valid Python
identifier), so `import mini_stark_amd` resolves here and this module points its
package path at that directory."""
import os as _os

__path__ = [_os.path.join(_os.path.dirname(_os.path.abspath(__file__)), "mini-stark_amd")]
from mini_stark_amd._native import (  # noqa: E402,F401
    Context, MsError, build_library, library_path, load_library, flatten_terms, terms_rows,
    AIR_PERIODIC, MsAir, flatten_air, air_struct, air_rows,
    AUX_SUM, AUX_PRODUCT, MsAux, flatten_aux, aux_struct, aux_constraints, flatten_aux_arg, instantiate_aux, aux_fractions, encode_aux,
    GOLDILOCKS, BABYBEAR, FLAG_ZERO_DISPLAY_EMPTY, FLAG_TRACE_MONT64, FLAG_LATENCY, FLAG_DIGEST_BLAKE2S, FLAG_DIGEST_BLAKE3, FLAG_DIGEST_KECCAK256, FLAG_DIGEST_SHA3_256,
    DIGEST_SHA256, DIGEST_BLAKE2S256, DIGEST_BLAKE3, DIGEST_KECCAK256, DIGEST_SHA3_256,
    TREE_TRACE, TREE_LDE, TREE_FRI, TREE_VALIDITY, TREE_LDE_STAGED, MsDeep, deep_struct,
    OK, ERR_SHAPE, ERR_LEAF_NOT_FOUND, ERR_OUT_OF_RANGE, ERR_STATE, ERR_ARG, ERR_HIP, ERR_NOMEM,
)
