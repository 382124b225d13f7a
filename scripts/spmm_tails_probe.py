#!/usr/bin/env python3
"""The row kernels' batched tail (csrc/spmm_rows.h, BATCH_TAIL) against a build of the parent commit, in ONE process on the SAME buffers
(placement classes move the same launch by ~10 % between processes and between buffers: DESIGN.md §2.1):

    python scripts/spmm_tails_probe.py PARENT_LIB.so [--config C3] [--buffers 4] [--repeats 5] [--out profiles/spmm_tails_c3.json]

PARENT_LIB.so: libcleora_hip.so built from the parent commit.  Three launches on bench.py's own graph — the f32 SpMM + L2 of the
headline (cleora_propagate_dev), the f16 gather into f32 rows (cleora_propagate_hf_dev) and the f16-stored iterate
(cleora_propagate_h_dev) — each on one X and `--buffers` candidate Y buffers.  Per (X, Y) pair: `--repeats` rounds of (parent, new),
a round's figure the mean of 6 launches between two HIP events; reported per pair: both medians over the rounds, the parent's spread
(max - min over its rounds) and whether the new build wins by more than that.  The outputs of both builds are compared bit for bit."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import torch  # noqa: E402
from cleora_amd import _hip  # noqa: E402


def load(path):
    L = ctypes.CDLL(os.path.abspath(path))
    for name, (res, a) in _hip.SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, a
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("--config", default="C3", choices=sorted(bench.CONFIGS))
    ap.add_argument("--nodes", type=int, default=0)
    ap.add_argument("--pairs", type=int, default=0)
    ap.add_argument("--buffers", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spmm_tails_c3.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    wl = types.SimpleNamespace(config=args.config, nodes=args.nodes, pairs=args.pairs, hyperedges=0, products=0, dim=0, seed=2)
    g, hashes, label, cfg = bench.make_workload(wl, dev, 0, 1, False)
    n, nnz, d = int(g["n"]), int(g["nnz"]), int(cfg["dim"])
    S = torch.cuda.current_stream().cuda_stream
    libs = {"parent": load(args.parent), "new": _hip.lib()}
    graphs = {}
    for name, L in libs.items():
        h = ctypes.c_void_p()
        rc = L.cleora_graph_create_dev(0, n, n, nnz, g["rowptr"].data_ptr(), g["col"].data_ptr(), g["val_left"].data_ptr(), None, 0, 0, ctypes.byref(h))
        assert rc == 0, (name, rc)
        graphs[name] = h

    x = torch.empty((n, d), device=dev)
    _hip.check(libs["new"].cleora_init_dev(hashes.data_ptr(), n, d, 0, x.data_ptr(), d, S))
    x /= x.norm(dim=1, keepdim=True)                                   # unit rows, as inside the loop
    x16 = x.to(torch.float16)
    ys = [torch.empty((n, d), device=dev) for _ in range(args.buffers)]
    ys16 = [torch.empty((n, d), device=dev, dtype=torch.float16) for _ in range(args.buffers)]
    F = _hip.F_L2NORM
    launches = {
        "f32 (cleora_propagate_dev, L2NORM)": (ys, lambda L, h, y: L.cleora_propagate_dev(h, _hip.LEFT, x.data_ptr(), d, d, y.data_ptr(), d, F, 0.0, None, None, None, S)),
        "f16 gather, f32 rows out (cleora_propagate_hf_dev, L2NORM)": (ys, lambda L, h, y: L.cleora_propagate_hf_dev(h, _hip.LEFT, x16.data_ptr(), d, d, y.data_ptr(), d, F, S)),
        "f16 iterate (cleora_propagate_h_dev, L2NORM)": (ys16, lambda L, h, y: L.cleora_propagate_h_dev(h, _hip.LEFT, x16.data_ptr(), d, d, y.data_ptr(), d, F, 0.0, None, None, S)),
    }
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(call, L, h, y, reps=6):
        ev[0].record()
        for _ in range(reps):
            assert call(L, h, y) == 0
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / reps

    rec = {"workload": label, "n": n, "nnz": nnz, "d": d, "repeats": args.repeats, "launches_per_repeat": 6, "launches": {}}
    for lname, (bufs, call) in launches.items():
        pairs = []
        for k, y in enumerate(bufs):
            outs = {}
            for name, L in libs.items():                               # (the gather cache policy arms on the third launch)
                timed(call, L, graphs[name], y, 4)
                outs[name] = y.clone() if k == 0 else None
            t = {"parent": [], "new": []}
            for _ in range(args.repeats):
                for name, L in libs.items():
                    t[name].append(timed(call, L, graphs[name], y))
            row = {"y": hex(y.data_ptr()), "parent_ms": [round(v, 3) for v in t["parent"]], "new_ms": [round(v, 3) for v in t["new"]],
                   "parent_median_ms": round(statistics.median(t["parent"]), 3), "new_median_ms": round(statistics.median(t["new"]), 3),
                   "parent_spread_ms": round(max(t["parent"]) - min(t["parent"]), 3)}
            row["gain_ms"] = round(row["parent_median_ms"] - row["new_median_ms"], 3)
            row["new_wins_by_more_than_parent_spread"] = row["gain_ms"] > row["parent_spread_ms"]
            if k == 0:
                row["outputs_bit_equal"] = bool(torch.equal(outs["parent"].view(torch.int16 if y.dtype == torch.float16 else torch.int32),
                                                            outs["new"].view(torch.int16 if y.dtype == torch.float16 else torch.int32)))
            del outs
            pairs.append(row)
            print(lname, json.dumps(row), flush=True)
        rec["launches"][lname] = {"x": hex((x16 if "f16" in lname else x).data_ptr()), "pairs": pairs,
                                  "new_wins_every_pair_by_more_than_parent_spread": all(p["new_wins_by_more_than_parent_spread"] for p in pairs),
                                  "new_slower_on_some_pair": any(p["gain_ms"] < 0 for p in pairs)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
