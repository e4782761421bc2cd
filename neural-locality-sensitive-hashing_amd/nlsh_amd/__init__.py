"""nlsh_amd: MI355X-native query-time hot path of Neural LSH.

Mirrors the reference's Python surface (`Indexer`, `build_index`, `MultivariateBernoulli`,
`hash_codes`, `calculate_recall`, `SIFT.distance` / `Glove.distance`) on top of a C-ABI HIP
library (`include/nlsh_hip.h`).  Submodules are imported lazily so that `nlsh_amd.synth`
and `nlsh_amd.metrics` stay usable where the HIP library has not been built.
"""
__version__ = "0.1.0"

_LAZY = {"MultiTableIndexer": "multitable", "MultiRowFilter": "multitable", "RefineStore": "refine"}


def __getattr__(name):
    """`nlsh_amd.MultiTableIndexer` / `nlsh_amd.MultiRowFilter`, imported on first use (the module needs torch; see above)."""
    if name in _LAZY:
        import importlib
        return getattr(importlib.import_module(f"{__name__}.{_LAZY[name]}"), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
