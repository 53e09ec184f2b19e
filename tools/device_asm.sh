#!/bin/bash
# Device assembly of every source in the csrc Makefile's SRCS, with that Makefile's own flags (per-file ones included) plus --cuda-device-only -S:
#   tools/device_asm.sh TREE OUTDIR            -> OUTDIR/<name>.s for each source of TREE and OUTDIR/SHA256 (one line per file)
#   tools/device_asm.sh --diff OUTDIR_A OUTDIR_B   -> `cmp` of every file of A with B's; exit status 1 if any differs or is missing
# A refactor that must not move an instruction is checked by emitting a parent checkout and the branch and diffing the two (profiles/retired_switches.txt).
# (-fuse-cuid=none: the compilation-unit id is a hash of the source path and would make two checkouts of the same code differ in one symbol name.)
# It only writes, hashes and compares; it needs no GPU.
set -e
if [ "$1" = --diff ]; then
  rc=0
  for a in "$2"/*.s; do
    cmp -s "$a" "$3/$(basename "$a")" && echo "same    $(basename "$a")" || { echo "DIFFERS $(basename "$a")"; rc=1; }
  done
  exit $rc
fi
tree=$(cd "$1" && pwd); mkdir -p "$2"; out=$(cd "$2" && pwd)
make -C "$tree/spoofsv_amd/csrc" -j16 -f Makefile -f - ASMDIR="$out" device_asm <<'EOF'
device_asm: $(SRCS:%.hip=$(ASMDIR)/%.s)
$(ASMDIR)/%.s: %.hip FORCE
	$(HIPCC) $(FLAGS) $(FLAGS_$*) --cuda-device-only -S -fuse-cuid=none $< -o $@
FORCE:
.PHONY: device_asm FORCE
EOF
(cd "$out" && sha256sum *.s > SHA256)
echo "wrote $(ls "$out"/*.s | wc -l) files to $out"
