#!/bin/bash
# Compare the gfx950 code of kernels in two builds of one HIP translation unit:
# per kernel the VGPR / SGPR / scratch figures of both objects and the number
# of differing lines between their mnemonic sequences (operands dropped: a
# kernel argument block that grew changes offsets, not instructions).
#
#   tools/kernel_isa_diff.sh OLD.hip.o NEW.hip.o [NAME-SUBSTRING ...]
#
# e.g. after a change to csrc/jxg_front_kernel.h, against objects kept from the
# commit before (the search instantiations of front_kernel must
# not change when another unit's do), for each of the three units that include it:
#   tools/kernel_isa_diff.sh old/jxg_front.hip.o build/jxg_front.hip.o front_kernelILb1 front_kernelILb0 homog_kernel
#   tools/kernel_isa_diff.sh old/jxg_front_forced.hip.o build/jxg_front_forced.hip.o front_kernelILb0
#   tools/kernel_isa_diff.sh old/jxg_front_trace.hip.o build/jxg_front_trace.hip.o front_kernelILb1 front_kernelILb0
# or after a unit was split (jxg_merge.hip into eval, the rest of the stage and
# vb_list), every kernel of the old object against the object it now lives in;
# the kernels that moved elsewhere print "not in both objects" and the run
# exits 1, so name them:
#   tools/kernel_isa_diff.sh old/jxg_merge.hip.o build/jxg_merge.hip.o merge_eval_kernel
#   tools/kernel_isa_diff.sh old/jxg_merge.hip.o build/jxg_merge_write.hip.o merge_resolve_kernel force_list_kernel merge_write_kernel
#   tools/kernel_isa_diff.sh old/jxg_merge.hip.o build/jxg_vb_list.hip.o vb_list_kernel
# and jxg_ac.hip into the walk, the prefix-code emitter and the rANS coder:
#   tools/kernel_isa_diff.sh old/jxg_ac.hip.o build/jxg_ac_hist.hip.o ac_hist_kernelILi32 ac_hist_kernelILi8
#   tools/kernel_isa_diff.sh old/jxg_ac.hip.o build/jxg_ac_emit.hip.o ac_emit_kernel
#   tools/kernel_isa_diff.sh old/jxg_ac.hip.o build/jxg_ans.hip.o ans_encode_kernel ans_encode_diag_kernel ans_sums_kernel ans_emit_kernel
# A template's mangled name changes with its parameter list and namespace
# (jxg12front_kernelILb1ELb0EEE became jxg9search_tu12front_kernelILb1ELb0ELb0EEE):
# substrings are matched, first match per object.
# Without names every kernel of OLD is compared with the kernel of the same name.
set -euo pipefail
LLVM=${LLVM:-/opt/rocm/llvm/bin}
ARCH=${ARCH:-gfx950}
[ $# -ge 2 ] || { sed -n 2,29p "$0"; exit 2; }
old=$1; new=$2; shift 2
tmp=$(mktemp -d); trap 'rm -rf "$tmp"' EXIT
for v in old new; do
  o=${!v}
  "$LLVM/llvm-objcopy" --dump-section .hip_fatbin="$tmp/$v.fat" "$o"
  "$LLVM/clang-offload-bundler" --unbundle --type=o --input="$tmp/$v.fat" \
    --targets=hipv4-amdgcn-amd-amdhsa--$ARCH --output="$tmp/$v.co"
  "$LLVM/llvm-objdump" -d "$tmp/$v.co" > "$tmp/$v.s"
  "$LLVM/llvm-readelf" --notes "$tmp/$v.co" |
    grep -E "\.name:|\.vgpr_count|\.sgpr_count|\.private_segment_fixed_size" | paste - - - - |
    sed -E 's/[[:space:]]+/ /g' > "$tmp/$v.res"
done
# file, symbol, count file: the kernel's mnemonics without the s_nop padding
# behind its end (up to the next kernel's alignment; a whole block behind the
# object's last kernel, whichever that is); the padding's length goes to the
# count file
mnemonics() {
  awk -v n="$2" '/^[0-9a-f]+ <.*>:/{p=($0 ~ "<" n ">:")} p' "$1" | grep -v '^[0-9a-f]* <' |
    grep -E '^[[:space:]]+[a-z_][a-z0-9_]*([[:space:]]|$)' |  # instructions only (objdump ends some listings with "..." for elided zeros)
    sed -E 's/^[[:space:]]+//' | awk 'NF{print $1}' |
    awk -v pad="$3" '{l[NR]=$0} END{n=NR; while (n && l[n]=="s_nop") n--;
                     for (i=1;i<=n;i++) print l[i]; print NR-n > pad}'
}
# (no match prints nothing and is no error: the loop reports it and goes on)
symbol() { { grep -oE "^[0-9a-f]+ <[^>]*$2[^>]*>:" "$1" || true; } | head -1 | sed -E 's/^[0-9a-f]+ <(.*)>:/\1/'; }
[ $# -gt 0 ] || set -- $(grep -oE '^[0-9a-f]+ <[^>]+>:' "$tmp/old.s" | sed -E 's/^[0-9a-f]+ <(.*)>:/\1/')
rc=0
for name in "$@"; do
  so=$(symbol "$tmp/old.s" "$name"); sn=$(symbol "$tmp/new.s" "$name")
  if [ -z "$so" ] || [ -z "$sn" ]; then echo "$name: not in both objects"; rc=1; continue; fi
  mnemonics "$tmp/old.s" "$so" "$tmp/pa" > "$tmp/a"; mnemonics "$tmp/new.s" "$sn" "$tmp/pb" > "$tmp/b"
  d=$(diff "$tmp/a" "$tmp/b" | grep -c '^[<>]' || true)
  echo "$so -> $sn"
  echo "  old:$(grep -F " $so " "$tmp/old.res" | sed -E 's/ \.name: [^ ]+//')  instructions $(wc -l < "$tmp/a") (+$(cat "$tmp/pa") padding)"
  echo "  new:$(grep -F " $sn " "$tmp/new.res" | sed -E 's/ \.name: [^ ]+//')  instructions $(wc -l < "$tmp/b") (+$(cat "$tmp/pb") padding)"
  echo "  differing mnemonic lines: $d"
  [ "$d" = 0 ] || rc=1
done
exit $rc
