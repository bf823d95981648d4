#!/bin/bash
# Code-object metadata of every kernel of bio_ik_amd/libbioik_hip.so (registers, spilled registers, scratch bytes per lane, LDS): extracts the gfx950 code
# object from the library's fat binary and reads its notes with llvm-readelf.  No GPU needed.  usage: tools/kernel_metadata.sh [library] > profiles/rNN_kernel_metadata.txt
LIB=${1:-bio_ik_amd/libbioik_hip.so}
T=$(mktemp -d)
L=/opt/rocm/lib/llvm/bin
$L/llvm-objcopy --dump-section .hip_fatbin=$T/fat.bin "$LIB" /dev/null 2>/dev/null || $L/llvm-objcopy --dump-section .hip_fatbin=$T/fat.bin "$LIB"
# (the section holds one bundle per translation unit with device code -- bioik_hip.hip, bioik_bounded.hip --, each starting with the bundler's magic string)
python3 - "$T" <<'PY'
import re, sys
d = open(sys.argv[1] + "/fat.bin", "rb").read()
offs = [m.start() for m in re.finditer(b"__CLANG_OFFLOAD_BUNDLE__", d)]
for j, o in enumerate(offs):
    open("%s/bundle%d.bin" % (sys.argv[1], j), "wb").write(d[o:offs[j + 1] if j + 1 < len(offs) else len(d)])
PY
echo "# $(basename $LIB): llvm-readelf --notes of the gfx950 code objects ($(sha256sum "$LIB" | cut -c1-16)); sources $(cd $(dirname $0)/.. && python -c 'import bench; print(bench.kernel_sources_hash()[:16])' 2>/dev/null)"
printf "%-28s %6s %12s %6s %12s %8s\n" kernel vgprs vgpr_spills sgprs sgpr_spills scratch_B
for B in $T/bundle*.bin; do
$L/clang-offload-bundler --unbundle --type=o --input=$B --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output=$T/k.co
$L/llvm-readelf --notes $T/k.co | awk '
/\.name:/ {name=$2}
/\.private_segment_fixed_size:/ {scr=$2}
/\.sgpr_count:/ {sg=$2}
/\.sgpr_spill_count:/ {sgs=$2}
/\.vgpr_count:/ {vg=$2}
/\.vgpr_spill_count:/ {vgs=$2; cmd="c++filt " name; cmd | getline dn; close(cmd); sub(/\(.*/,"",dn); printf "%-28s %6s %12s %6s %12s %8s\n", dn, vg, vgs, sg, sgs, scr}'
done
rm -rf $T
