#!/bin/bash
# Variant builds of libgnerf_hip.so for A/B timing and ablation (g-nerf_amd/gnerf_hip/variants/libgnerf_<v>.so, selected with
# GNERF_HIP_LIB): the render group (compile_unit.sh: RENDER_UNITS; or the one unit $VARIANT_UNIT) recompiled with the variant's macros, in
# parallel, through the same assembly pass as the product build; every other object taken from the product build (run
# g-nerf_amd/csrc/build.sh first).  A variant is a '+'-joined list of parts: `base`,
# `STAMPS` (-DGNERF_STAMPS), `D:MACRO[=v]` (-DMACRO[=v]), anything else X -> -DGNERF_ABLATE_X (timing only: outputs are WRONG).
set -euo pipefail
root="$(cd "$(dirname "$0")/.." && pwd)"
here="$root/g-nerf_amd/csrc"
out="$root/g-nerf_amd/gnerf_hip/variants"
mkdir -p "$out"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
FLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -I$root/include -I$here -Wno-unused-value -Wno-unused-command-line-argument"
. "$here/compile_unit.sh"
group="${VARIANT_UNIT:-$RENDER_UNITS}"  # the translation units that are recompiled with the variant's macros
for v in "$@"; do
  defs=""
  IFS='+' read -ra parts <<< "$v"
  for p in "${parts[@]}"; do if [ "$p" = STAMPS ]; then defs="$defs -DGNERF_STAMPS"; elif [ "${p#D:}" != "$p" ]; then defs="$defs -D${p#D:}"; elif [ "$p" != base ]; then defs="$defs -DGNERF_ABLATE_$p"; fi; done
  ( mine=(); pids=()
    for u in $group; do compile_unit $u "$out/${u}_$v.o" "$defs" > /dev/null & pids+=($!); mine+=("$out/${u}_$v.o"); done
    for pid in "${pids[@]}"; do wait "$pid" || { echo "[variant] $v: a compile failed" >&2; exit 1; }; done
    others=(); for u in $UNITS; do case " $group " in *" $u "*) ;; *) others+=("$here/$u.o");; esac; done
    $HIPCC -shared -fPIC --offload-arch=gfx950 "${others[@]}" "${mine[@]}" -o "$out/libgnerf_$v.so"
    for o in "${mine[@]}"; do python3 "$root/tools/kernel_resources.py" "$o" 2>/dev/null || true; done > "$out/resources_$v.txt"
    rm -f "${mine[@]}"; echo "[variant] $v" ) &
done
wait
