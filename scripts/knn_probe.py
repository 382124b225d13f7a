#!/usr/bin/env python3
"""The fused kNN kernel (cleora_knn_cosine_dev, csrc/knn.hip) against the batched top-k path it relieves (cleora_topk_cosine_dev,
csrc/similarity.hip), both entry points in ONE process on the same device arrays, alternating:

    timeout -k 10 900 python scripts/knn_probe.py --part sources   [--out profiles/knn_probe.json]
    timeout -k 10 600 python scripts/knn_probe.py --part threshold
    timeout -k 10 600 python scripts/knn_probe.py --part masked
    timeout -k 10 600 rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/knn_probe.py --part trace

  sources    every row a query (d = 256, k = 10, exclude_self, no graph) at n = 65 536 and 262 144, random unit rows: ms of both,
             their ratio, the largest score difference and the share of equal indices between the two results, and the fused
             call's f32 matrix-core rate (2 n^2 d flop over the WHOLE call) against the roof of v_mfma_f32_32x32x2_f32
  threshold  n = 262 144, n_queries in {64, 256, 1024, 4096, 16384}: KNN_FUSED_MIN_QUERIES is the smallest of these from which
             the fused call is at least 10 % faster (and not below 257)
  masked     the n = 262 144 all-sources call with exclude_existing on a synth.power_law_graph of 10 pairs per node (the
             benchmark's degree law scaled down) beside the unmasked call on the same rows; states the longest row
  trace      one warm-up and one fused all-sources call at n = 262 144, for a kernel trace
Times: host clock around the call and a device synchronise, median of --runs (>= 5) after one warm-up call of each."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from cleora_amd import _hip, synth  # noqa: E402

F32_MFMA_ROOF = 157.3e12      # flop/s: 256 CUs x 256 flop/clk x 2.4 GHz


def calls(L, x, n, d, k, queries, graph, exclude_existing):
    """(fused, batched): closures that enqueue one call each into their own outputs and workspaces."""
    dev = x.device
    nq = n if queries is None else queries.numel()
    q_all = torch.arange(n, dtype=torch.int32, device=dev) if queries is None else queries
    out = {name: (torch.empty((nq, k), dtype=torch.int32, device=dev), torch.empty((nq, k), dtype=torch.float32, device=dev))
           for name in ("fused", "batched")}
    ws_f = torch.empty(L.cleora_knn_workspace(n, d, k, nq), dtype=torch.uint8, device=dev)
    ws_b = torch.empty(L.cleora_topk_workspace_for(n, k, min(nq, 2**32 - 1)), dtype=torch.uint8, device=dev)
    g = graph.handle if exclude_existing else None

    def fused():
        _hip.check(L.cleora_knn_cosine_dev(g, x.data_ptr(), d, n, d, None if queries is None else queries.data_ptr(), nq, k, 1,
                                           1 if exclude_existing else 0, out["fused"][0].data_ptr(), out["fused"][1].data_ptr(),
                                           ws_f.data_ptr(), None))

    def batched():
        _hip.check(L.cleora_topk_cosine_dev(g, x.data_ptr(), d, n, d, q_all.data_ptr(), nq, k, 1, 1 if exclude_existing else 0,
                                            out["batched"][0].data_ptr(), out["batched"][1].data_ptr(), ws_b.data_ptr(), None))

    return {"fused": fused, "batched": batched}, out


def timed(fns, runs):
    ms = {name: [] for name in fns}
    for name, fn in fns.items():          # warm-up
        fn()
        torch.cuda.synchronize()
    for _ in range(runs):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    return {name: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for name, v in ms.items()}


def unit_rows(n, d, dev, seed=1):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    x = torch.randn((n, d), generator=g, device=dev, dtype=torch.float32)
    return x / x.norm(dim=1, keepdim=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["sources", "threshold", "masked", "trace"], required=True)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("knn_probe: no GPU")
    dev, L, d, k = torch.device("cuda:0"), _hip.lib(), 256, 10
    rec = {"part": a.part, "d": d, "k": k, "runs": a.runs}
    if a.part == "sources":
        for n in (65536, 262144):
            x = unit_rows(n, d, dev)
            fns, out = calls(L, x, n, d, k, None, None, False)
            t = timed(fns, a.runs)
            t["batched_over_fused"] = t["batched"]["median_ms"] / t["fused"]["median_ms"]
            t["max_score_difference"] = float((out["fused"][1] - out["batched"][1]).abs().max())
            t["equal_index_share"] = float((out["fused"][0] == out["batched"][0]).float().mean())
            t["fused_flop_per_s_whole_call"] = 2.0 * n * n * d / (t["fused"]["median_ms"] * 1e-3)
            t["fused_share_of_f32_mfma_roof"] = t["fused_flop_per_s_whole_call"] / F32_MFMA_ROOF
            rec[f"n={n}"] = t
            print(json.dumps({f"n={n}": t}), flush=True)
    elif a.part == "threshold":
        n = 262144
        x = unit_rows(n, d, dev)
        for nq in (64, 256, 1024, 4096, 16384):
            gq = torch.Generator(device=dev)
            gq.manual_seed(nq)
            queries = torch.randint(0, n, (nq,), generator=gq, device=dev, dtype=torch.int32)
            fns, _ = calls(L, x, n, d, k, queries, None, False)
            t = timed(fns, a.runs)
            t["batched_over_fused"] = t["batched"]["median_ms"] / t["fused"]["median_ms"]
            rec[f"nq={nq}"] = t
            print(json.dumps({f"nq={nq}": t}), flush=True)
    elif a.part == "masked":
        csr = synth.power_law_graph(262144, 10 * 262144, 7, dev)
        n = csr["n"]
        graph = _hip.Graph.from_device(n, n, csr["nnz"], csr["rowptr"].data_ptr(), csr["col"].data_ptr(), csr["val_left"].data_ptr(),
                                       None, keepalive=csr)
        x = unit_rows(n, d, dev)
        plain, _ = calls(L, x, n, d, k, None, None, False)
        masked, out = calls(L, x, n, d, k, None, graph, True)
        t = timed({"fused": plain["fused"], "fused_exclude_existing": masked["fused"]}, a.runs)
        rec.update(n=n, nnz=csr["nnz"], longest_row=int(csr["rowptr"].diff().max()), **t)
        print(json.dumps(rec), flush=True)
    else:
        n = 262144
        fns, _ = calls(L, unit_rows(n, d, dev), n, d, k, None, None, False)
        for _ in range(2):
            fns["fused"]()
            torch.cuda.synchronize()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
