#!/bin/bash
# Builds libcleora_hip.so for gfx950 (cross-compiles without a GPU).
#   -ffp-contract=off : the SpMM must keep the reference's separate f32 multiply + add
#                       (src/embedding.rs:80-82); never let the compiler form FMAs.
set -euo pipefail
cd "$(dirname "$0")"
OUT=../libcleora_hip.so
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wall -Wno-unused-function"
mkdir -p obj
pids=()
for f in spmm spmm_h rowops whiten gram_h project_f16 project_f16_copy eigh hot attention comm peer sharded colsharded multi stager similarity knn kmeans pq ivf abi; do
  if [ ! -f obj/$f.o ] || [ $f.hip -nt obj/$f.o ] || [ common.h -nt obj/$f.o ] || [ project_common.h -nt obj/$f.o ] || [ gram32_common.h -nt obj/$f.o ] || [ project_f16.hip -nt obj/$f.o ] || [ row_epilogue.h -nt obj/$f.o ] || [ spmm_rows.h -nt obj/$f.o ] || [ comm_internal.h -nt obj/$f.o ] || [ shm_barrier.h -nt obj/$f.o ] || [ row_inv_norm.h -nt obj/$f.o ] || [ member_lists.h -nt obj/$f.o ] || [ knn_select.h -nt obj/$f.o ] || [ ../../include/cleora_hip.h -nt obj/$f.o ]; then
    # whiten.hip: MFMA accumulators in the VGPR form — hipcc otherwise parks loop-carried accumulators in VGPRs and copies
    # them to AGPRs and back around every chunk of MFMAs (256 v_accvgpr moves per 64 MFMAs in the Gram kernel)
    extra=""; [ $f = whiten ] && extra="-mllvm -amdgpu-mfma-vgpr-form"
    # spmm_h.hip: no packed f32 arithmetic — every element keeps its own v_mul_f32 + v_add_f32 between the f16 load and store
    [ $f = spmm_h ] && extra="-Xclang -target-feature -Xclang -packed-fp32-ops"
    # project_f16_copy.hip (includes project_f16.hip): the same for the kernels that round their output to f16
    [ $f = project_f16_copy ] && extra="-Xclang -target-feature -Xclang -packed-fp32-ops"
    # gram_h.hip: both — loop-carried MFMA accumulators, and plain v_add_f32 for the stage sums
    [ $f = gram_h ] && extra="-mllvm -amdgpu-mfma-vgpr-form -Xclang -target-feature -Xclang -packed-fp32-ops"
    # knn.hip: the loop-carried MFMA accumulator of the score tile stays in VGPRs (the selection reads it there), and plain
    # v_mul_f32 for the 1 / ||x_r|| scale of the accumulators
    [ $f = knn ] && extra="-mllvm -amdgpu-mfma-vgpr-form -Xclang -target-feature -Xclang -packed-fp32-ops"
    # kmeans.hip: the two loop-carried score accumulators per wave stay in VGPRs (the arg-max reads them there)
    [ $f = kmeans ] && extra="-mllvm -amdgpu-mfma-vgpr-form"
    # pq.hip: the same for the two score accumulators of the encode kernel
    [ $f = pq ] && extra="-mllvm -amdgpu-mfma-vgpr-form"
    # ivf.hip: the score accumulator of the list-scan kernel stays in VGPRs like knn.hip's (no scale in its epilogue: the plain flag)
    [ $f = ivf ] && extra="-mllvm -amdgpu-mfma-vgpr-form"
    hipcc $FLAGS $extra -c $f.hip -o obj/$f.o &
    pids+=($!)
  fi
done
# host-only math (the d x d step of the intermediate whitened iterations for small d): plain C++, multi-versioned for AVX2 / AVX-512
if [ ! -f obj/dxd_host.o ] || [ dxd_host.cpp -nt obj/dxd_host.o ]; then g++ -O3 -std=c++17 -fPIC -c dxd_host.cpp -o obj/dxd_host.o; fi
for p in "${pids[@]:-}"; do [ -n "$p" ] && wait $p; done
hipcc --offload-arch=gfx950 -shared -fPIC obj/dxd_host.o obj/spmm.o obj/spmm_h.o obj/rowops.o obj/whiten.o obj/gram_h.o obj/project_f16.o obj/project_f16_copy.o obj/eigh.o obj/hot.o obj/attention.o obj/comm.o obj/peer.o obj/sharded.o obj/colsharded.o obj/multi.o obj/stager.o obj/similarity.o obj/knn.o obj/kmeans.o obj/pq.o obj/ivf.o obj/abi.o -ldl -lpthread -lrt -o $OUT
echo "built $(realpath $OUT)"
