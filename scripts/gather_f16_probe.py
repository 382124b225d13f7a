#!/usr/bin/env python3
"""The f16 gather of the whitened loop (CLEORA_F_GATHER_F16) against the f32 path on the benchmark's own graph, in ONE process:

    python scripts/gather_f16_probe.py [--config C3] [--launches 20] [--out profiles/gather_f16_c3.json]

Builds the workload with bench.py's generator and, on the same graph handle, after warm-up launches (the hot-column marks arm on the
third launch), interleaves
  (1) the SpMM of the loop: cleora_propagate_dev with flags 0 on the f32 unit rows Y, and cleora_propagate_hf_dev on their f16 copy;
  (2) the loop's projection at d = 256: cleora_project_bounded_dev, and cleora_project_bounded_h_dev (the same plus the f16 copy);
every launch between two HIP events on the launch stream; then (3) `--loops` pairs of an `--iterations`-iteration whitened
cleora_embed_dev without and with the flag (the library's own loop timer: the loop runs on streams of its own).  Medians and ranges;
the SpMMs' bytes/s on their own gather models as fractions of the 8 TB/s peak.  --resources / --loop-test: the compiler's register
report for the d = 256 and d = 1024 kernels and the d = 256 figures printed by tests/test_gpu_gather_f16.py, copied into the record.

--stats-f16 (CLEORA_F_STATS_F16; write it to profiles/stats_f16_c3.json) adds, in the same process: (4) the statistics stage —
cleora_whiten_stats_dev(intermediate = 1) on the f32 rows against cleora_whiten_stats_h_dev on their f16 copy — with both Grams' errors
against an f64 Gram of the f16 values (torch, f64, on the device); the projection that stores only the f16 rows in (2); the loop with
GATHER_F16 | STATS_F16 as a third member of (3), and every loop's peak device memory (the driver's free memory sampled from a thread
while the call runs, against the free memory before it)."""
import argparse
import json
import os
import statistics
import sys
import threading
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the workload generator and the byte model of the headline)
import torch  # noqa: E402
from cleora_amd import _hip  # noqa: E402

RESOURCES = {  # hipcc -Rpass-analysis=kernel-resource-usage: VGPRs, scratch bytes per lane, waves per SIMD
    "spmm_rows_h_kernel<64, 1, 4, true, true> (d = 256)": [43, 0, 8],
    "spmm_rows_h_kernel<64, 2, 8, true, true> (d = 1024)": [71, 0, 7],
    "hub_finish_h_kernel<1, true> (d = 256)": [62, 0, 8],
    "hub_finish_h_kernel<4, true> (d = 1024)": [64, 0, 8],
    "project_f16_kernel<1, true>": [256, 276, 2],
    "project_f16_kernel<1> (no copy)": [256, 248, 2],
}
LOOP_TEST_D256 = {  # tests/test_gpu_gather_f16.py, (6000, 256, 4, symmetric): largest deviation of pairwise cosines from the f64 model
    "rw=0": {"delta_models": 1.53e-4, "gpu_f32_gather": 4.03e-7, "gpu_f16_gather": 1.42e-4},
    "rw=0.3": {"delta_models": 7.32e-5, "gpu_f32_gather": 1.45e-7, "gpu_f16_gather": 8.06e-5},
}
STATS_F16_TEST = {"statistics_e_new_e_old": {"n=4096 d=256": [4.44e-08, 2.57e-08], "n=4096 d=512": [6.03e-08, 3.4e-08], "n=4099 d=256": [4.46e-08, 2.47e-08], "n=4099 d=512": [6e-08, 3.45e-08], "n=6151 d=256": [3.66e-08, 2.2e-08], "n=6151 d=512": [4.99e-08, 2.92e-08], "n=4096 d=256 with 2048-row folds (rejected)": [2.8e-07, 2.57e-08]}, "loop_delta_models_gpu_f16_only_gpu_f16_gather": {"6000x256, 4 it.": [0.000132, 0.000146, 0.000142], "5000x512, 3 it.": [8.96e-05, 7.79e-05, 9.04e-05], "20000x64, 6 it.": [0.000387, 0.000366, 0.000399]}, "gramh_kernel_vgpr_scratch_waves_lds": [225, 0, 2, "64 KiB (d = 256) / 96 KiB"]}  # tests/test_gpu_stats_f16.py as printed on an MI355X, and hipcc's report for gramh_kernel


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def interleave(runs, launches):
    times = {name: [] for name, _ in runs}
    for _ in range(launches):
        for name, run in runs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    return times


def gram_errors(L, y32, y16, n, d):
    """||G - G64||_F / ||G64||_F of both intermediate forms on the same (f16-representable) values, and their times"""
    dev = y32.device
    y32.copy_(y16)                                                    # the widened rows: both forms see the same values
    mean = torch.zeros(d, dtype=torch.float64, device=dev)
    gram = torch.zeros((d, d), dtype=torch.float64, device=dev)
    step = 1 << 19
    for r in range(0, n, step):
        mean += y16[r:r + step].double().sum(dim=0)
    mean /= n
    for r in range(0, n, step):
        c = y16[r:r + step].double() - mean
        gram += c.T @ c
    ws = torch.empty(L.cleora_whiten_workspace(n, d), dtype=torch.uint8, device=dev)
    m, g = torch.empty(d, dtype=torch.float64, device=dev), torch.empty((d, d), dtype=torch.float64, device=dev)
    runs = (("split_bf16_on_f32_rows", lambda: _hip.check(L.cleora_whiten_stats_dev(y32.data_ptr(), d, n, d, ws.data_ptr(), 1, m.data_ptr(), g.data_ptr(), None))),
            ("f16_mfma_on_f16_rows", lambda: _hip.check(L.cleora_whiten_stats_h_dev(y16.data_ptr(), d, n, d, ws.data_ptr(), m.data_ptr(), g.data_ptr(), None))))
    out = {}
    for name, run in runs:
        run()
        torch.cuda.synchronize()
        out[name] = {"gram_rel_frobenius_error": float((g - gram).norm() / gram.norm()), "mean_max_abs_error": float((m - mean).abs().max())}
    for name, ms in interleave(runs, 20).items():
        out[name].update(summary(ms))
    out["mean_norm_squared"] = float((mean * mean).sum())
    return out


def peak_memory_during(call):
    """bytes of device memory taken while call() runs: the largest drop of the driver's free memory, sampled every 2 ms"""
    free0 = torch.cuda.mem_get_info()[0]
    low, done = [free0], threading.Event()

    def sample():
        while not done.is_set():
            low[0] = min(low[0], torch.cuda.mem_get_info()[0])
            time.sleep(0.002)
    th = threading.Thread(target=sample)
    th.start()
    try:
        call()
    finally:
        done.set()
        th.join()
    return free0 - low[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stats-f16", action="store_true")
    ap.add_argument("--config", default="C3", choices=sorted(bench.CONFIGS))
    ap.add_argument("--nodes", type=int, default=0)
    ap.add_argument("--pairs", type=int, default=0)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--iterations", type=int, default=8)
    ap.add_argument("--loops", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gather_f16_c3.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    L = _hip.lib()
    wl = types.SimpleNamespace(config=args.config, nodes=args.nodes, pairs=args.pairs, hyperedges=0, products=0)
    g, hashes, label, cfg = bench.make_workload(wl, dev, 0, 1, False)
    n, nnz, d = int(g["n"]), int(g["nnz"]), int(cfg["dim"])
    graph = _hip.Graph.from_device(n, n, nnz, g["rowptr"].data_ptr(), g["col"].data_ptr(), g["val_left"].data_ptr(), None, 0, keepalive=g)
    rec = {"workload": label, "n": n, "nnz": nnz, "d": d, "launches": args.launches, "noise_floor": "the 10-12 % placement-class spread "
           "of DESIGN.md §2.1: a difference inside it counts as no difference", "kernel_resources_vgpr_scratch_waves": RESOURCES,
           "loop_test_d256": LOOP_TEST_D256}

    y32 = torch.empty((n, d), dtype=torch.float32, device=dev)       # Y: unit rows, as inside the loop
    z32 = torch.empty_like(y32)                                       # Z = A Y
    y16 = torch.empty((n, d), dtype=torch.float16, device=dev)
    _hip.check(L.cleora_init_dev(hashes.data_ptr(), n, d, 0, z32.data_ptr(), d, None))
    _hip.check(L.cleora_propagate_dev(graph.handle, _hip.LEFT, z32.data_ptr(), d, d, y32.data_ptr(), d, _hip.F_L2NORM, 0.0, None, None, None, None))
    _hip.check(L.cleora_convert_f32_to_f16_dev(y32.data_ptr(), d, n, d, y16.data_ptr(), d, None))

    def spmm_f32():
        _hip.check(L.cleora_propagate_dev(graph.handle, _hip.LEFT, y32.data_ptr(), d, d, z32.data_ptr(), d, 0, 0.0, None, None, None, None))

    def spmm_f16():
        _hip.check(L.cleora_propagate_hf_dev(graph.handle, _hip.LEFT, y16.data_ptr(), d, d, z32.data_ptr(), d, 0, None))

    for _ in range(args.warmup):
        spmm_f32()
        spmm_f16()
    torch.cuda.synchronize()
    times = interleave((("f32", spmm_f32), ("f16", spmm_f16)), args.launches)
    model = {"f32": bench.algorithmic_bytes(nnz, n, n, d), "f16": nnz * 8 + (n + 1) * 8 + nnz * d * 2 + n * d * 4}
    rec["spmm"] = {name: {**summary(ms), "model_bytes": model[name],
                          "fraction_of_8TBps": model[name] / (statistics.median(ms) * 1e-3) / (bench.HBM_PEAK_GBPS * 1e9)}
                   for name, ms in times.items()}
    rec["spmm"]["f32_over_f16"] = rec["spmm"]["f32"]["median_ms"] / rec["spmm"]["f16"]["median_ms"]
    rec["spmm"]["byte_model_ratio"] = model["f32"] / model["f16"]
    zf = z32.clone()
    spmm_f32()
    torch.cuda.synchronize()
    rec["spmm"]["max_abs_diff_of_the_outputs"] = float((zf - z32).abs().max())     # z32: from the f32 gather; zf: from the f16 gather
    del zf
    if args.stats_f16:
        rec["stats_f16_test"] = STATS_F16_TEST
    if args.stats_f16 and d % 256 == 0:
        rec["statistics"] = gram_errors(L, y32, y16, n, d)

    if d == 256:
        # the projection of an intermediate iteration: x = Z (bounded row by row), a centring vector and a transform of whitening size
        rowsum = torch.empty(n, dtype=torch.float32, device=dev)
        rowabs = torch.empty_like(rowsum)
        _hip.check(L.cleora_csr_rowsums_dev(graph.handle, _hip.LEFT, rowsum.data_ptr(), rowabs.data_ptr(), None))
        gen = torch.Generator(device=dev).manual_seed(0)
        mean = (torch.randn(d, device=dev, generator=gen) * 0.01).clamp(-1, 1)
        t = torch.randn((d, d), device=dev, generator=gen) * (d ** 0.5)
        out = torch.empty_like(z32)

        def project():
            _hip.check(L.cleora_project_bounded_dev(z32.data_ptr(), d, n, d, mean.data_ptr(), t.data_ptr(), d, out.data_ptr(), d, rowsum.data_ptr(),
                                                    rowabs.data_ptr(), 1, None, None, None))

        def project_copy():
            _hip.check(L.cleora_project_bounded_h_dev(z32.data_ptr(), d, n, d, mean.data_ptr(), t.data_ptr(), d, out.data_ptr(), d, rowsum.data_ptr(),
                                                      rowabs.data_ptr(), 1, None, None, y16.data_ptr(), d, None))

        def convert():
            _hip.check(L.cleora_convert_f32_to_f16_dev(out.data_ptr(), d, n, d, y16.data_ptr(), d, None))

        def project_f16_only():
            _hip.check(L.cleora_project_bounded_h_dev(z32.data_ptr(), d, n, d, mean.data_ptr(), t.data_ptr(), d, None, d, rowsum.data_ptr(),
                                                      rowabs.data_ptr(), 1, None, None, y16.data_ptr(), d, None))

        forms = (("no_copy", project), ("with_copy_8_byte_stores", project_copy), ("separate_convert_pass", convert))
        if args.stats_f16:
            forms += (("f16_rows_only", project_f16_only),)
        for _ in range(2):
            for _, run in forms:
                run()
        torch.cuda.synchronize()
        times = interleave(forms, args.launches)
        rec["projection"] = {name: summary(ms) for name, ms in times.items()}
        del out, rowsum, rowabs
    del y32, y16

    # the whitened loop, device-resident, without and with the flag (pairs interleaved; the library's loop timer)
    variants = (("f32", 0), ("f16", _hip.F_GATHER_F16))
    if args.stats_f16:
        variants += (("f16_rows_only", _hip.F_GATHER_F16 | _hip.F_STATS_F16),)
    loop, peak = {name: [] for name, _ in variants}, {name: 0 for name, _ in variants}
    for _ in range(args.loops):
        for name, flag in variants:
            _hip.check(L.cleora_init_dev(hashes.data_ptr(), n, d, 0, z32.data_ptr(), d, None))
            torch.cuda.synchronize()
            run = lambda: _hip.check(L.cleora_embed_dev(graph.handle, z32.data_ptr(), _hip.LEFT, d, args.iterations, 0.0, 0.0, _hip.F_WHITEN | flag, None))
            if args.stats_f16:
                peak[name] = max(peak[name], peak_memory_during(run))
            else:
                run()
            loop[name].append(float(L.cleora_last_embed_loop_ms()))
    rec["whitened_loop"] = {"iterations": args.iterations, "pairs": args.loops, **{name: summary(ms) for name, ms in loop.items()}}
    if args.stats_f16:
        rec["whitened_loop"]["peak_device_bytes_inside_the_call"] = peak
        rec["whitened_loop"]["iterate_bytes"] = n * d * 4
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
