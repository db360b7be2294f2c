#!/bin/bash
# kernels whose VGPR / scratch usage differs between HEAD and the working tree: scripts/regs_diff.sh name.hip
f=$1; d=$(mktemp -d); R=$(cd "$(dirname "$0")/.." && pwd); C=vub_image_denoising_amd/csrc
mkdir -p $d/$C $d/include
git -C $R show HEAD:include/rdunet_hip.h > $d/include/rdunet_hip.h
# (every header HEAD has in csrc/, and the file itself)
for h in $(git -C $R ls-tree --name-only HEAD $C/ | grep '\.h$') $C/$f; do git -C $R show HEAD:$h > $d/$h; done
$R/scripts/regs.sh $d/$C/$f | awk '{print $3, $1, $2}' | sort > $d/old
$R/scripts/regs.sh $R/$C/$f | awk '{print $3, $1, $2}' | sort > $d/new
join $d/old $d/new | awk '{ if ($2!=$4 || $3!=$5) printf "%4d %4d -> %4d %4d  %s\n", $2, $3, $4, $5, $1 }'
rm -rf $d
