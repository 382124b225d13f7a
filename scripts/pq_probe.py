#!/usr/bin/env python3
"""The device product quantisation (csrc/pq.hip) beside a plain torch-ROCm restatement of the same steps, both in ONE process on the
same device arrays, alternating:

    timeout -k 10 900 python scripts/pq_probe.py [--out profiles/pq_probe.json] [--n 1048576 9999997] [--nq 1 64 4096]

For d = 256, M = 8 subspaces, kc = 256 centroids and every n: ms of
  assign   cleora_pq_assign_dev (codes of all subspaces, no distances)    | per chunk of 262144 rows: bmm over the subspaces, + ||c||^2, argmin
  update   cleora_pq_update_dev                                           | index_add_ of the sub-rows, bincount, mean
  scan     cleora_pq_search_dev, top_k = 10, per nq (tables included)     | per chunk of queries: gather-and-sum over the subspaces, topk
the number of unequal codes between the two assigns, the assign call's f32 matrix-core rate (2 n d kc flop), the largest centroid
difference between the two updates (both from OUR codes), and for the scan its
achieved share of two bounds over the WHOLE call: HBM for the codes (every query tile streams n M bytes) and LDS reads (n M nq / 4
lookups of 16 bytes).  Times: host clock around the call and a device synchronise, median of --runs (>= 5) after one warm-up call
of each."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from cleora_amd import _hip  # noqa: E402

F32_MFMA_ROOF = 157.3e12      # flop/s: 256 CUs x 256 flop/clk x 2.4 GHz
HBM_ROOF = 8.0e12             # B/s
LDS_ROOF = 78.6e12            # B/s: 256 CUs x 128 B/clk x 2.4 GHz
ROW_CHUNK = 262144


def timed(fns, runs):
    ms = {name: [] for name in fns}
    for fn in fns.values():               # warm-up
        fn()
        torch.cuda.synchronize()
    for _ in range(runs):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    out = {name: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for name, v in ms.items()}
    out["torch_over_ours"] = out["torch"]["median_ms"] / out["ours"]["median_ms"]
    return out


def torch_assign(x, cb):
    M, kc, ds = cb.shape
    cn, cbt = (cb * cb).sum(dim=2).unsqueeze(1), cb.transpose(1, 2)
    parts = []
    for r in range(0, x.shape[0], ROW_CHUNK):
        sub = x[r:r + ROW_CHUNK].view(-1, M, ds).transpose(0, 1)
        parts.append((cn - 2.0 * torch.bmm(sub, cbt)).argmin(dim=2).transpose(0, 1))
    return torch.cat(parts)


def torch_update(x, codes, cb):
    M, kc, ds = cb.shape
    flat = (codes + torch.arange(M, device=x.device) * kc).reshape(-1)
    sums = torch.zeros((M * kc, ds), dtype=x.dtype, device=x.device).index_add_(0, flat, x.view(-1, ds))
    counts = torch.bincount(flat, minlength=M * kc).to(x.dtype).unsqueeze(1)
    return torch.where(counts > 0, sums / counts.clamp(min=1.0), cb.view(M * kc, ds)).view(M, kc, ds)


def torch_scan(codes, cb, queries, top_k):
    M, kc, ds = cb.shape
    unit = cb / cb.norm(dim=2, keepdim=True).clamp(min=1e-10)
    qn = queries.norm(dim=1, keepdim=True)
    tables = torch.einsum("mcj,qmj->qmc", unit, torch.where(qn > 1e-10, queries / qn.clamp(min=1e-30), queries).view(-1, M, ds))
    step = max(1, (1 << 28) // codes.shape[0])             # at most 1 GiB of scores at a time
    found = []
    for q in range(0, queries.shape[0], step):
        scores = torch.zeros((min(step, queries.shape[0] - q), codes.shape[0]), dtype=torch.float32, device=codes.device)
        for m in range(M):
            scores += tables[q:q + step, m][:, codes[:, m]]
        found.append(scores.topk(top_k, dim=1))
    return found


def probe(L, n, d, M, kc, nqs, runs, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(n)
    ds = d // M
    x = torch.randn((n, d), generator=g, device=dev, dtype=torch.float32) * (0.5 + 4.0 * torch.rand((n, 1), generator=g, device=dev))
    cb = x[torch.randperm(n, generator=g, device=dev)[:kc]].view(kc, M, ds).transpose(0, 1).contiguous()
    ws = torch.empty(L.cleora_pq_workspace(n, d, M, kc), dtype=torch.uint8, device=dev)
    codes = torch.zeros((n, M), dtype=torch.uint8, device=dev)
    close = torch.zeros(M, dtype=torch.int32, device=dev)
    cb_ours, out, res = cb.clone(), {}, {}

    def ours_assign():
        _hip.check(L.cleora_pq_assign_dev(x.data_ptr(), d, n, d, cb.data_ptr(), M, kc, codes.data_ptr(), None, ws.data_ptr(), None))

    def ours_update():
        cb_ours.copy_(cb)
        _hip.check(L.cleora_pq_update_dev(x.data_ptr(), d, n, d, codes.data_ptr(), cb_ours.data_ptr(), M, kc, close.data_ptr(), ws.data_ptr(), None))

    res["assign"] = timed({"ours": ours_assign, "torch": lambda: out.update(assign=torch_assign(x, cb))}, runs)
    codes64 = codes.to(torch.int64)       # OUR codes: both updates and both scans start from them
    res["assign"]["unequal_codes"] = int((codes64 != out.pop("assign")).sum())
    res["assign"]["flop_per_s_whole_call"] = 2.0 * n * d * kc / (res["assign"]["ours"]["median_ms"] * 1e-3)
    res["assign"]["share_of_f32_mfma_roof"] = res["assign"]["flop_per_s_whole_call"] / F32_MFMA_ROOF
    res["update"] = timed({"ours": ours_update, "torch": lambda: out.update(update=torch_update(x, codes64, cb))}, runs)
    res["update"]["max_centroid_difference"] = float((cb_ours - out.pop("update")).abs().max())
    for nq in nqs:
        queries = x[torch.randperm(n, generator=g, device=dev)[:nq]].contiguous()
        sws = torch.empty(L.cleora_pq_search_workspace(n, M, kc, nq, 10), dtype=torch.uint8, device=dev)
        oi, os_ = torch.zeros((nq, 10), dtype=torch.int32, device=dev), torch.zeros((nq, 10), dtype=torch.float32, device=dev)

        def ours_scan():
            _hip.check(L.cleora_pq_search_dev(codes.data_ptr(), n, cb.data_ptr(), M, kc, ds, queries.data_ptr(), nq, 10, oi.data_ptr(),
                                              os_.data_ptr(), None, sws.data_ptr(), None))

        part = timed({"ours": ours_scan, "torch": lambda: out.update(scan=torch_scan(codes64, cb, queries, 10))}, runs)
        ref = torch.cat([f.values for f in out.pop("scan")])
        seconds, tiles = part["ours"]["median_ms"] * 1e-3, (nq + 7) // 8
        part["max_score_difference"] = float((os_ - ref).abs().max())
        part["share_of_hbm_bound"] = tiles * n * M / seconds / HBM_ROOF
        part["share_of_lds_bound"] = n * M * nq / 4 * 16 / seconds / LDS_ROOF
        res[f"scan,nq={nq}"] = part
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1048576, 9999997])
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 64, 4096])
    ap.add_argument("--d", type=int, default=256)
    ap.add_argument("--subspaces", type=int, default=8)
    ap.add_argument("--centroids", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pq_probe: no GPU")
    dev, L = torch.device("cuda:0"), _hip.lib()
    rec = {"d": a.d, "subspaces": a.subspaces, "centroids": a.centroids, "runs": a.runs, "top_k": 10}
    for n in a.n:
        rec[f"n={n}"] = probe(L, n, a.d, a.subspaces, a.centroids, a.nq, a.runs, dev)
        print(json.dumps({f"n={n}": rec[f"n={n}"]}), flush=True)
        if a.out:                         # after every shape: a later shape that fails loses nothing
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
