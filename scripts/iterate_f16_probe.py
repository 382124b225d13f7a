#!/usr/bin/env python3
"""f16-stored iterates against the f32 SpMM on the benchmark's own graph, in ONE process on one GPU:

    python scripts/iterate_f16_probe.py [--config C3] [--launches 20] [--out profiles/iterate_f16_c3.json]

Builds the workload with bench.py's generator, then alternates cleora_propagate_dev (L2NORM | HUB_SEGMENTS, f32 rows) and
cleora_propagate_h_dev (L2NORM, f16 rows) on the same graph handle: warm-up launches first (the hot-column marks arm on the third
launch), then `--launches` of each interleaved, every launch between two HIP events on the launch stream, the device synchronised
at both ends.  Reports both medians with their spreads, the ratio, and each kernel's bytes/s on its OWN gather model as a fraction
of the 8 TB/s peak; then one `--iterations`-iteration plain loop (cleora_embed_dev) with and without CLEORA_F_ITERATE_F16.
--vgprs / --scratch / --occupancy: what hipcc -Rpass-analysis=kernel-resource-usage reports for the d = 256 kernel
(spmm_rows_h_kernel<64, 1, 4, true>), copied into the record."""
import argparse
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the workload generator and the byte model of the headline)
import torch  # noqa: E402
from cleora_amd import _hip  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3", choices=sorted(bench.CONFIGS))
    ap.add_argument("--nodes", type=int, default=0)
    ap.add_argument("--pairs", type=int, default=0)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--iterations", type=int, default=40)
    ap.add_argument("--vgprs", type=int, default=43)
    ap.add_argument("--scratch", type=int, default=0)
    ap.add_argument("--occupancy", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iterate_f16_c3.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    L = _hip.lib()
    wl = types.SimpleNamespace(config=args.config, nodes=args.nodes, pairs=args.pairs, hyperedges=0, products=0)
    g, hashes, label, cfg = bench.make_workload(wl, dev, 0, 1, False)
    n, nnz, d = int(g["n"]), int(g["nnz"]), int(cfg["dim"])
    graph = _hip.Graph.from_device(n, n, nnz, g["rowptr"].data_ptr(), g["col"].data_ptr(), g["val_left"].data_ptr(), None, 0, keepalive=g)

    x32 = torch.empty((n, d), dtype=torch.float32, device=dev)
    y32 = torch.empty_like(x32)
    x16 = torch.empty((n, d), dtype=torch.float16, device=dev)
    y16 = torch.empty_like(x16)
    f32_flags = _hip.F_L2NORM | _hip.F_HUB_SEGMENTS

    def run32():
        _hip.check(L.cleora_propagate_dev(graph.handle, _hip.LEFT, x32.data_ptr(), d, d, y32.data_ptr(), d, f32_flags, 0.0, None, None, None, None))

    def run16():
        _hip.check(L.cleora_propagate_h_dev(graph.handle, _hip.LEFT, x16.data_ptr(), d, d, y16.data_ptr(), d, _hip.F_L2NORM, 0.0, None, None, None))

    # a unit-row iterate, as inside the loop: E_1 in f32, and the same rows rounded to f16
    _hip.check(L.cleora_init_dev(hashes.data_ptr(), n, d, 0, y32.data_ptr(), d, None))
    _hip.check(L.cleora_propagate_dev(graph.handle, _hip.LEFT, y32.data_ptr(), d, d, x32.data_ptr(), d, f32_flags, 0.0, None, None, None, None))
    _hip.check(L.cleora_convert_f32_to_f16_dev(x32.data_ptr(), d, n, d, x16.data_ptr(), d, None))
    for _ in range(args.warmup):
        run32()
        run16()
    torch.cuda.synchronize()
    times = {"f32": [], "f16": []}
    for _ in range(args.launches):
        for name, run in (("f32", run32), ("f16", run16)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    torch.cuda.synchronize()
    # what one f16 rounding of the iterate costs the next one: the two outputs side by side
    max_abs_diff = float((y16.float() - y32).abs().max())

    model = {"f32": bench.algorithmic_bytes(nnz, n, n, d), "f16": nnz * 8 + (n + 1) * 8 + nnz * d * 2 + n * d * 2}
    rec = {"workload": label, "n": n, "nnz": nnz, "d": d, "launches": args.launches, "max_abs_diff_f16_vs_f32_output": max_abs_diff}
    for name, ms in times.items():
        med = statistics.median(ms)
        rec[name] = {"median_ms": med, "min_ms": min(ms), "max_ms": max(ms), "model_bytes": model[name],
                     "fraction_of_8TBps": model[name] / (med * 1e-3) / (bench.HBM_PEAK_GBPS * 1e9)}
    rec["f32_over_f16"] = rec["f32"]["median_ms"] / rec["f16"]["median_ms"]
    rec["byte_model_ratio"] = model["f32"] / model["f16"]
    rec["kernel"] = {"name": "spmm_rows_h_kernel<64, 1, 4, true>", "vgprs": args.vgprs, "scratch_bytes_per_lane": args.scratch,
                     "waves_per_simd": args.occupancy}

    # the plain loop, device-resident, with and without the f16 iterates
    del y32, x16, y16
    loop = {}
    for name, flag in (("f32", 0), ("f16", _hip.F_ITERATE_F16)):
        _hip.check(L.cleora_init_dev(hashes.data_ptr(), n, d, 0, x32.data_ptr(), d, None))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _hip.check(L.cleora_embed_dev(graph.handle, x32.data_ptr(), _hip.LEFT, d, args.iterations, 0.0, 0.0, flag, None))
        loop[name] = {"wall_ms": (time.perf_counter() - t0) * 1e3, "loop_ms": float(L.cleora_last_embed_loop_ms())}
    rec["embed_loop"] = {"iterations": args.iterations, **loop}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
