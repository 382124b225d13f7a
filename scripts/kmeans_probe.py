#!/usr/bin/env python3
"""The device k-means (csrc/kmeans.hip) beside a plain torch-ROCm restatement of the same steps, both in ONE process on the same
device arrays, alternating:

    timeout -k 10 900 python scripts/kmeans_probe.py [--out profiles/kmeans_probe.json] [--n 262144 1048576] [--k 16 256 1024 4096]

For d = 256 and every (n, k): ms of
  assign   cleora_kmeans_assign_dev (labels + changed count, no cosine)   | (x @ c.T).argmax(1) and the count of changed labels
  update   cleora_kmeans_update_dev                                       | index_add_ of the normalised rows, mean, normalise
  loop     cleora_kmeans_cosine, --iterations assigns from random rows    | the same number of assign / .item() / update rounds
the share of equal labels between the two assigns, the largest centroid difference between the two updates, and the assign call's
f32 matrix-core rate (2 n k d flop over the WHOLE call) against the roof of v_mfma_f32_32x32x2_f32.
Times: host clock around the call and a device synchronise, median of --runs (>= 5) after one warm-up call of each."""
import argparse
import ctypes
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
    return {name: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for name, v in ms.items()}


def torch_assign(xn, cent, labels):
    new = (xn @ cent.T).argmax(dim=1)
    return new, (new != labels).sum()


def torch_update(xn, labels, cent):
    k = cent.shape[0]
    sums = torch.zeros_like(cent).index_add_(0, labels, xn)
    counts = torch.bincount(labels, minlength=k).to(xn.dtype).unsqueeze(1)
    mean = sums / counts.clamp(min=1.0)
    norm = mean.norm(dim=1, keepdim=True)
    return torch.where((counts > 0) & (norm > 1e-10), mean / norm.clamp(min=1e-10), cent)


def probe(L, n, d, k, iterations, runs, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(n + k)
    x = torch.randn((n, d), generator=g, device=dev, dtype=torch.float32) * (0.5 + 4.0 * torch.rand((n, 1), generator=g, device=dev))
    xn = x / x.norm(dim=1, keepdim=True).clamp(min=1e-10)
    start = xn[torch.randperm(n, generator=g, device=dev)[:k]].contiguous()
    ws = torch.empty(L.cleora_kmeans_workspace(n, d, k), dtype=torch.uint8, device=dev)
    labels_in = torch.randint(0, k, (n,), generator=g, device=dev, dtype=torch.int32)
    labels = labels_in.clone()
    changed = torch.zeros(1, dtype=torch.int64, device=dev)
    cent_ours, cent_loop = start.clone(), start.clone()
    ran = ctypes.c_uint32(0)
    res = {}

    def ours_assign():
        _hip.check(L.cleora_kmeans_assign_dev(x.data_ptr(), d, n, d, start.data_ptr(), k, labels.data_ptr(), None, changed.data_ptr(),
                                              ws.data_ptr(), None))

    def ours_update():
        _hip.check(L.cleora_kmeans_update_dev(x.data_ptr(), d, n, d, labels.data_ptr(), cent_ours.data_ptr(), k, ws.data_ptr(), None))

    def ours_loop():
        cent_loop.copy_(start)
        _hip.check(L.cleora_kmeans_cosine(x.data_ptr(), d, n, d, cent_loop.data_ptr(), k, iterations, labels.data_ptr(), ctypes.byref(ran),
                                          ws.data_ptr(), None))

    def ref_loop():
        cent, lab = start.clone(), torch.zeros(n, dtype=torch.int64, device=dev)
        for _ in range(iterations):
            new, moved = torch_assign(xn, cent, lab)
            if int(moved.item()) == 0:
                break
            lab, cent = new, torch_update(xn, new, cent)

    out = {}
    res["assign"] = timed({"ours": ours_assign, "torch": lambda: out.update(assign=torch_assign(xn, start, labels_in))}, runs)
    ours_assign()                         # labels now hold OUR assignment of `start` (the timed calls already left it there)
    torch.cuda.synchronize()
    ref_labels = out["assign"][0]
    res["assign"]["equal_label_share"] = float((labels.to(torch.int64) == ref_labels).float().mean())
    res["assign"]["flop_per_s_whole_call"] = 2.0 * n * k * d / (res["assign"]["ours"]["median_ms"] * 1e-3)
    res["assign"]["share_of_f32_mfma_roof"] = res["assign"]["flop_per_s_whole_call"] / F32_MFMA_ROOF
    del out["assign"]
    lab64 = labels.to(torch.int64)
    res["update"] = timed({"ours": lambda: (cent_ours.copy_(start), ours_update()),
                           "torch": lambda: out.update(update=torch_update(xn, lab64, start))}, runs)
    res["update"]["max_centroid_difference"] = float((cent_ours - out["update"]).abs().max())
    res["loop"] = timed({"ours": ours_loop, "torch": ref_loop}, runs)
    res["loop"]["assigns_run"] = int(ran.value)
    for part in res.values():
        part["torch_over_ours"] = part["torch"]["median_ms"] / part["ours"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[262144, 1048576])
    ap.add_argument("--k", type=int, nargs="+", default=[16, 256, 1024, 4096])
    ap.add_argument("--d", type=int, default=256)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kmeans_probe: no GPU")
    dev, L = torch.device("cuda:0"), _hip.lib()
    rec = {"d": a.d, "runs": a.runs, "iterations": a.iterations}
    for n in a.n:
        for k in a.k:
            rec[f"n={n},k={k}"] = probe(L, n, a.d, k, a.iterations, a.runs, dev)
            print(json.dumps({f"n={n},k={k}": rec[f"n={n},k={k}"]}), flush=True)
            if a.out:                     # after every shape: a later shape that fails loses nothing
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "w") as f:
                    json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
