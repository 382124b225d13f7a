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
report for the d = 256 and d = 1024 kernels and the d = 256 figures printed by tests/test_gpu_gather_f16.py, copied into the record."""
import argparse
import json
import os
import statistics
import sys
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


def main():
    ap = argparse.ArgumentParser()
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

        for _ in range(2):
            project()
            project_copy()
            convert()
        torch.cuda.synchronize()
        times = interleave((("no_copy", project), ("with_copy_8_byte_stores", project_copy), ("separate_convert_pass", convert)), args.launches)
        rec["projection"] = {name: summary(ms) for name, ms in times.items()}
        del out, rowsum, rowabs
    del y32, y16

    # the whitened loop, device-resident, without and with the flag (pairs interleaved; the library's loop timer)
    loop = {"f32": [], "f16": []}
    for _ in range(args.loops):
        for name, flag in (("f32", 0), ("f16", _hip.F_GATHER_F16)):
            _hip.check(L.cleora_init_dev(hashes.data_ptr(), n, d, 0, z32.data_ptr(), d, None))
            torch.cuda.synchronize()
            _hip.check(L.cleora_embed_dev(graph.handle, z32.data_ptr(), _hip.LEFT, d, args.iterations, 0.0, 0.0, _hip.F_WHITEN | flag, None))
            loop[name].append(float(L.cleora_last_embed_loop_ms()))
    rec["whitened_loop"] = {"iterations": args.iterations, "pairs": args.loops, **{name: summary(ms) for name, ms in loop.items()}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
