"""ctypes binding of libnvf_hip.so, derived from include/nvf_hip.h (the C ABI) by _cabi.

The header is the one definition of the boundary: the compiler holds the .hip implementations to it, and the
prototypes, request structs and constants below are read out of it at import, from this tree (never from wherever
NVF_LIB points) and without loading the shared object.  An entry point added to the header is bound with no edit here.

The library is the only compute path: there is no CPU fallback.  ``lib()`` raises if the shared object is missing
(run ``python -m nvfpcc_amd.build`` or ``__graft_entry__.build()``).
"""
import ctypes as C
import os

from . import _cabi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NVF_LIB", os.path.join(_HERE, "libnvf_hip.so"))   # NVF_LIB: A/B a second build

_HEADER = _cabi.read_header("nvf_hip.h")
PROTOTYPES = _HEADER.prototypes     # name -> (restype, argtypes)
CONSTANTS = _HEADER.constants       # every object-like #define, e.g. CONSTANTS["NVF_ACT_RELU"]
NvfStepTail, NvfRateJob, NvfStemHead, NvfAdamFuse, NvfTrunkWgrads, NvfPcSparseIndex, NvfLayerDesc = (
    _HEADER.structs[n] for n in ("NvfStepTail", "NvfRateJob", "NvfStemHead", "NvfAdamFuse", "NvfTrunkWgrads",
                                 "NvfPcSparseIndex", "NvfLayerDesc"))

_lib = None


def lib():
    """Load (once) and return the ctypes handle with every prototype declared."""
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: the HIP extension has not been built "
                "(python -m nvfpcc_amd.build). There is no CPU fallback for the NVF hot path.")
        _lib = _cabi.bind(C.CDLL(LIB_PATH), PROTOTYPES)   # AttributeError if the .so is stale
    return _lib


class NvfError(RuntimeError):
    pass


def check(rc, what):
    if rc != 0:
        kind = {CONSTANTS["NVF_EINVAL"]: "NVF_EINVAL (rejected argument)",
                CONSTANTS["NVF_EWORKSPACE"]: "NVF_EWORKSPACE (workspace too small)"}.get(rc, f"hipError_t {rc}")
        raise NvfError(f"{what} failed: {kind}")
