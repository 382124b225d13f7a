"""cleora_amd — MI355X-native implementation of pycleora's Markov-propagation hot path.

  cleora_amd.pycleora.SparseMatrix   drop-in for pycleora.pycleora.SparseMatrix (src/lib.rs)
  cleora_amd.embed                   device-resident embed()/whitening loop (pycleora/__init__.py:51-164)
  cleora_amd.variants                device-resident embed variants + predict_links (pycleora/__init__.py:206-410, 636-681, 784-852)
  cleora_amd.sharded                 column- / row-partitioned multi-GPU propagation (one process per GPU)
  cleora_amd.compress                product quantisation on the device: product_quantize / PQIndex (pycleora/compress.py:32-181)
  cleora_amd.search                  approximate nearest neighbours on the device: IVFIndex / ANNIndex (pycleora/search.py:101-215)
  cleora_amd._hip                    ctypes binding of libcleora_hip.so (include/cleora_hip.h)
"""
__version__ = "0.1.0"


def install(devices=None, hub_segments=None, iterate_dtype=None, gather_dtype=None, stats_dtype=None):
    """Make this package's SparseMatrix the reference's compiled module: after this call
    `import pycleora` (the reference's unmodified Python package) binds
    `from .pycleora import SparseMatrix` (pycleora/__init__.py:4) to cleora_amd.pycleora.

    devices: HIP device indices, e.g. range(8) — the graph is then row-partitioned over them INSIDE this process for
    embed_fast*, left / symmetric_markov_propagate and (after accelerate()) pycleora.embed(); None keeps what
    CLEORA_DEVICES / CLEORA_DEVICE say (default: device 0).
    hub_segments: True = the loops sum rows of more than 256 edges in segments (CLEORA_F_HUB_SEGMENTS: not the reference's bits,
    within 2e-6 of the sum of |terms|) — the way out for a graph whose longest row is an in-order chain of 10^7 additions; None keeps
    what CLEORA_HUB_SEGMENTS says (default: the reference's order).
    iterate_dtype: "f16" = embed_fast / embed_fast_convergence on one GPU keep their iterates in f16 between iterations
    (CLEORA_F_ITERATE_F16: half the SpMM's gathered bytes, f32 arithmetic, NOT the reference's bits; rows longer than 256 edges take
    the segmented sum); "f32" restores the default; None keeps the current setting.  Not combinable with `devices`.
    gather_dtype: "f16" = the whitened one-call loop of cleora_amd.embed.embed() on one GPU gathers an f16 copy of its normalised rows
    in every SpMM after the first (CLEORA_F_GATHER_F16: half the gathered bytes; sums, statistics and projections stay f32; NOT the
    reference's bits).  A preference: calls with a convergence threshold or a callback run in f32 as before.  "f32" restores the
    default; None keeps the current setting.  Not combinable with `devices`.
    stats_dtype: "f16" = with gather_dtype="f16", the loop keeps its intermediate normalised rows ONLY as f16 (CLEORA_F_STATS_F16:
    statistics from the f16 matrix cores on the stored values, no f32 copy of the rows, one iterate-sized buffer fewer).  A preference
    like gather_dtype: it also needs residual_weight == 0.  "f32" restores the default; None keeps the current setting.  Not
    combinable with `devices`."""
    import importlib.util
    import sys

    from . import pycleora as _mod
    if iterate_dtype is not None:
        if iterate_dtype not in ("f16", "f32"):
            raise ValueError(f"iterate_dtype must be 'f16' or 'f32', got {iterate_dtype!r}")
        if devices is not None:
            raise ValueError("iterate_dtype is served on one GPU only: do not combine it with devices=[...]")
        _mod.set_iterate_dtype(iterate_dtype)
    if gather_dtype is not None:
        if gather_dtype not in ("f16", "f32"):
            raise ValueError(f"gather_dtype must be 'f16' or 'f32', got {gather_dtype!r}")
        if devices is not None:
            raise ValueError("gather_dtype is served on one GPU only: do not combine it with devices=[...]")
        _mod.set_gather_dtype(gather_dtype)
    if stats_dtype is not None:
        if stats_dtype not in ("f16", "f32"):
            raise ValueError(f"stats_dtype must be 'f16' or 'f32', got {stats_dtype!r}")
        if devices is not None:
            raise ValueError("stats_dtype is served on one GPU only: do not combine it with devices=[...]")
        _mod.set_stats_dtype(stats_dtype)
    if devices is not None:
        _mod.set_devices(devices)
    if hub_segments is not None:
        _mod.set_hub_segments(hub_segments)
    sys.modules["pycleora.pycleora"] = _mod
    # pickles name the class by module path; use the reference's (src/sparse_matrix.rs:56) when its
    # Python package is importable so pickles interchange with real pycleora, else keep ours
    if "pycleora" in sys.modules or importlib.util.find_spec("pycleora") is not None:
        _mod.SparseMatrix.__module__ = "pycleora.pycleora"
    return _mod


def accelerate(package=None):
    """Optional second step after install(): rebind the reference package's own hot-path entry
    points to the device-resident versions, so that its CLI / benchmark / CleoraEmbedder (which all
    call `pycleora.embed`, pycleora/cli.py:148, __init__.py:885) keep the iterate in HBM instead of
    crossing PCIe twice per iteration and whitening in numpy:
        pycleora.embed              -> cleora_amd.embed.embed           (same signature)
        pycleora.whiten_embeddings  -> cleora_amd.embed.whiten_embeddings
        pycleora.embed_multiscale / embed_weighted / embed_directed / embed_with_attention /
        embed_edge_features / predict_links -> cleora_amd.variants.* (same signatures)
        pycleora.community.detect_communities_kmeans -> cleora_amd.variants.detect_communities_kmeans (when the package
        object has a `community` attribute with that function; k above the device's cap goes to the original)
        pycleora.compress.product_quantize -> cleora_amd.compress.product_quantize (when the package object has a `compress`
        attribute with that function; shapes beyond the device's limits go to the original)
    The one normalisation the device path does not run — 'spectral', a full SVD per iteration
    (pycleora/__init__.py:951-956) — is forwarded to the original."""
    import importlib

    from . import embed as _dev
    pkg = package if package is not None else importlib.import_module("pycleora")
    original_embed = pkg.embed

    def embed(graph, *args, **kwargs):
        norm = kwargs.get("normalization", args[3] if len(args) > 3 else "l2")
        if norm not in ("l2", "l1", "none") or not isinstance(graph, _dev.SparseMatrix):
            return original_embed(graph, *args, **kwargs)
        return _dev.embed(graph, *args, **kwargs)

    embed.__wrapped__ = original_embed
    pkg.embed = embed
    pkg.whiten_embeddings = _dev.whiten_embeddings

    # the embed variants and link prediction: same signatures, device-resident loop
    import inspect

    from . import variants as _var

    def rebind(name, owner=pkg, served=lambda bound: True):
        original = getattr(owner, name, None)
        device_fn = getattr(_var, name)
        if original is None:
            return
        sig = inspect.signature(device_fn)

        def wrapper(*args, **kwargs):
            try:
                bound = sig.bind(*args, **kwargs).arguments
            except TypeError:
                return original(*args, **kwargs)
            graph = bound.get("graph")
            if bound.get("normalization", "l2") not in ("l2", "l1", "none") or \
                    (graph is not None and not isinstance(graph, _dev.SparseMatrix)) or not served(bound):
                return original(*args, **kwargs)
            return device_fn(*args, **kwargs)

        wrapper.__wrapped__ = original
        wrapper.__name__ = name
        setattr(owner, name, wrapper)

    for name in ("embed_multiscale", "embed_weighted", "embed_directed", "embed_with_attention",
                 "embed_edge_features", "predict_links"):
        rebind(name)
    # pycleora.community.detect_communities_kmeans (pycleora/community.py:5-48) -> the device k-means, up to its cluster cap
    community = getattr(pkg, "community", None)
    if community is not None:
        rebind("detect_communities_kmeans", community, lambda bound: bound["k"] <= _var.KMEANS_MAX_K)
    # pycleora.compress.product_quantize (pycleora/compress.py:101-181) -> the device product quantisation, within its limits
    compress = getattr(pkg, "compress", None)
    original_pq = getattr(compress, "product_quantize", None)
    if original_pq is not None:
        from . import compress as _pq
        sig = inspect.signature(_pq.product_quantize)

        def product_quantize(*args, **kwargs):
            try:
                bound = sig.bind(*args, **kwargs)
                bound.apply_defaults()
                shape = getattr(bound.arguments["embeddings"], "shape", ())
                M, kc = bound.arguments["num_subspaces"], bound.arguments["num_centroids"]
                served = len(shape) == 2 and M > 0 and shape[1] % M == 0 and _pq._device_serves(shape[0], M, kc, shape[1] // M)
            except TypeError:
                served = False
            return _pq.product_quantize(*args, **kwargs) if served else original_pq(*args, **kwargs)

        product_quantize.__wrapped__ = original_pq
        compress.product_quantize = product_quantize
    return pkg
