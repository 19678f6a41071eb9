#!/bin/bash
# builds an A/B copy of the library with extra -D flags: mk_ab.sh <outdir> <flags...>
OUT=$1; shift
mkdir -p $OUT
OUT=$(cd $OUT && pwd)
SRC=${MK_AB_SRC:-$(cd "$(dirname "$0")/.." && pwd)/carmel_amd/csrc}  # (MK_AB_SRC: another checkout's csrc, e.g. the parent commit's)
cd $SRC
HIPFLAGS="--offload-arch=gfx950 -munsafe-fp-atomics"
CXX="-O3 -std=c++17 -fPIC -Wno-unused-function -Wno-unused-result"
pids=()
for f in kernels.hip tile_sweep.hip engine.cpp engine_unrolled.cpp compose.hip matrix_fb.hip lattice_gpu.hip comm.cpp exchange.cpp dense.hip unrolled.hip; do
  /opt/rocm/bin/hipcc $CXX $HIPFLAGS "$@" -c $f -o $OUT/${f%.*}.o & pids+=($!)
done
/opt/rocm/bin/hipcc $CXX $HIPFLAGS -mllvm -disable-machine-licm "$@" -c mstep_wide.hip -o $OUT/mstep_wide.o & pids+=($!)  # (Makefile: WIDEFLAGS)
for f in gibbs_exact.hip gibbs_lane.hip gibbs.hip forest_exact.hip forest.hip forest_host.cpp forest_gibbs.cpp decode.hip decode_paths.hip decode_kbest.hip decode_sum.hip decode_sample.hip decode_posterior.hip decode_pairs.hip decode_pairs_posterior.hip decode_pairs_sample.hip decode_pairs_kbest.hip decode_generate.hip decode_generate_tables.cpp decode_tables.cpp decode_best_paths.hip decode_best_paths_tables.cpp decode_prune.hip consolidate.hip decode_machine_sums.hip; do
  /opt/rocm/bin/hipcc $CXX $HIPFLAGS -ffp-contract=off "$@" -c $f -o $OUT/${f%.*}.o & pids+=($!)
done
/opt/rocm/bin/hipcc $CXX "$@" -c unrolled.cpp -o $OUT/unrolled_host.o & pids+=($!)
/opt/rocm/bin/hipcc $CXX "$@" -c lattice.cpp -o $OUT/lattice.o & pids+=($!)
/opt/rocm/bin/hipcc $CXX "$@" -c host_api.cpp -o $OUT/host_api.o & pids+=($!)
/opt/rocm/bin/hipcc $CXX "$@" -c options.cpp -o $OUT/options.o & pids+=($!)
for p in "${pids[@]}"; do wait $p || exit 1; done
/opt/rocm/bin/hipcc -shared -fPIC $HIPFLAGS -o $OUT/libcarmel_hip.so $OUT/*.o -lpthread -ldl -lrt
ls -la $OUT/libcarmel_hip.so
