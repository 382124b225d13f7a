"""Measures the IVF index (cleora_amd/search.py, csrc/ivf.hip) against the exact fused kNN on an embedding WITH cluster structure:
the whitened embedding (cleora_embed_dev + CLEORA_F_WHITEN, 4 iterations) of synth.power_law_graph(--nodes, 10 pairs per node).
Random unit rows have no clusters and say nothing about an IVF index.

For nprobe in 1, 2, 4, 8, 16, 32 with every row a query (k = 10, exclude_self): recall@k against cleora_knn_cosine_dev on the same
rows, the time of the search alone, the work of the scan (2 d flop per (query slot, list slot) of every work item: 64 query slots
x the list's whole tiles, padding included — arithmetic from probes_out and the list sizes) over the time of the WHOLE search (probe
selection, grouping, scan, merge: a lower bound on the scan kernel's own rate) against the 157.3 Tflop/s f32 MFMA roof, and the
largest list's share of that work.  Then 64-, 1024- and 16384-query batches against the fused and the batched exact paths.
Times: host clock around the call and a device synchronise, median of --runs (>= 5) after one warm-up call of each, the paths of a
comparison alternating in one process.  The build (upload, k-means, layout) is timed once."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cleora_amd import _hip, search, synth  # noqa: E402

ROOF_TFLOPS = 157.3


def timed(fns, runs):
    L = _hip.lib()
    ms = {name: [] for name in fns}
    for fn in fns.values():
        fn()
    _hip.check(L.cleora_stream_sync(None))
    for _ in range(runs):
        for name, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            _hip.check(L.cleora_stream_sync(None))
            ms[name].append((time.perf_counter() - t0) * 1e3)
    return {name: statistics.median(v) for name, v in ms.items()}


def embedding(n, d, dev):
    L = _hip.lib()
    g = synth.power_law_graph(n, 10 * n, 7, dev)
    n = g["n"]
    gr = _hip.Graph.from_device(n, n, g["nnz"], g["rowptr"].data_ptr(), g["col"].data_ptr(), g["val_left"].data_ptr(), None, dev.index or 0,
                                keepalive=g)
    x = torch.empty((n, d), dtype=torch.float32, device=dev)
    _hip.check(L.cleora_init_dev(synth.entity_hashes(n, 3, dev).data_ptr(), n, d, 0, x.data_ptr(), d, None))
    _hip.check(L.cleora_embed_dev(gr.handle, x.data_ptr(), _hip.LEFT, d, 4, 0.0, 0.0, _hip.F_WHITEN, None))
    torch.cuda.synchronize()
    return x.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=262144)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--nlist", type=int, default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ivf_probe: no GPU")
    L, k, d = _hip.lib(), a.k, a.dim
    x = embedding(a.nodes, d, torch.device("cuda:0"))
    n = len(x)
    t0 = time.perf_counter()
    ivf = search.IVFIndex(x, nlist=a.nlist)
    build_s = time.perf_counter() - t0
    sizes = ivf.list_sizes
    res = {"device": torch.cuda.get_device_name(0), "n": n, "d": d, "k": k, "nlist": ivf.nlist, "kmeans_iterations": ivf.iterations,
           "build_s_incl_upload_and_kmeans": build_s, "list_rows_min_mean_max": [int(sizes.min()), float(sizes.mean()), int(sizes.max())],
           "nprobe": {}, "batches": {}}

    rows = _hip.DevArray.from_host(np.arange(n, dtype=np.uint32))
    oi, os_ = _hip.DevArray((n, k), np.uint32), _hip.DevArray((n, k), np.float32)
    ei, es = _hip.DevArray((n, k), np.uint32), _hip.DevArray((n, k), np.float32)
    probes = _hip.DevArray((n, 32), np.uint32)
    kws = _hip.DevArray((L.cleora_knn_workspace(n, d, k, n),), np.uint8)
    iws = _hip.DevArray((L.cleora_ivf_search_workspace(n, d, ivf.nlist, min(32, ivf.nlist), k, n),), np.uint8)
    tws = _hip.DevArray((L.cleora_topk_workspace(n, k),), np.uint8)

    def exact(nq):
        return lambda: _hip.check(L.cleora_knn_cosine_dev(None, ivf._x.ptr, d, n, d, rows.ptr, nq, k, 1, 0, ei.ptr, es.ptr, kws.ptr, None))

    def batched(nq):
        return lambda: _hip.check(L.cleora_topk_cosine_dev(None, ivf._x.ptr, d, n, d, rows.ptr, nq, k, 1, 0, ei.ptr, es.ptr, tws.ptr, None))

    def approx(nq, nprobe):
        return lambda: _hip.check(L.cleora_ivf_search_dev(ivf._list_ptr.ptr, ivf._list_rows.ptr, ivf._xs.ptr, ivf._x.ptr, d, n, d,
                                                          ivf._centroids.ptr, ivf.nlist, None, rows.ptr, nq, nprobe, k, 1, oi.ptr, os_.ptr,
                                                          probes.ptr, iws.ptr, 0, None))

    tiles = (sizes + 127) // 128 * 128
    want = None
    for nprobe in (1, 2, 4, 8, 16, 32):
        if nprobe > ivf.nlist:
            break
        ms = timed({"exact": exact(n), "ivf": approx(n, nprobe)}, a.runs)
        want = ei.to_host() if want is None else want
        got = oi.to_host()
        recall = float((got[:, :, None] == want[:, None, :]).any(2).mean())
        hits = np.bincount(probes.to_host().ravel()[: n * nprobe].astype(np.int64), minlength=ivf.nlist)   # [n][nprobe] dense at the front
        work = (hits + 63) // 64 * 64 * tiles * 2.0 * d
        res["nprobe"][nprobe] = {"recall_at_k": recall, "ivf_ms": ms["ivf"], "exact_ms": ms["exact"],
                                 "scan_tflops_over_whole_search": work.sum() / ms["ivf"] / 1e9,
                                 "fraction_of_roof": work.sum() / ms["ivf"] / 1e9 / ROOF_TFLOPS,
                                 "largest_list_share_of_scan_work": float(work[np.argmax(sizes)] / work.sum())}
        print(json.dumps({nprobe: res["nprobe"][nprobe]}), flush=True)
    for nq in (64, 1024, 16384):
        res["batches"][nq] = timed({"fused_exact": exact(nq), "batched_exact": batched(nq), "ivf_nprobe8": approx(nq, min(8, ivf.nlist))}, a.runs)
        print(json.dumps({nq: res["batches"][nq]}), flush=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
