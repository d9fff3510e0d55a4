#!/bin/bash
# One md5 per device function of one csrc/*.hip file (kernels and the __noinline__ helpers they call): the text from the symbol's
# label to its end marker plus, for a kernel, its .amdhsa_kernel block, with comments and the function's index in the file taken out
# (.LBB<function>_<n> -> .LBB_<n>; the comments' column follows the label's width), so that two commits compare per symbol and as a set. Needs no GPU; CSRC = another checkout's csrc.
cd "${CSRC:-$(dirname "$0")/../safe-grid-agents_amd/csrc}" || exit 1
set -o pipefail
${HIPCC:-/opt/rocm/bin/hipcc} --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fvisibility=hidden $EXTRA --cuda-device-only -S "$1" -o - |
  sed -E 's/[[:space:]]*;.*$//; s/BB[0-9]+_/BB_/g; s/\.Lfunc_(begin|end)[0-9]+/.Lfunc_\1/g' |
  awk '/^\t\.type\t[^,]+,@function/ { split($2, a, ","); fn[a[1] ":"] = a[1] }
       ($1 in fn) && !cur { cur = fn[$1] }
       /^\t\.amdhsa_kernel / { cur = $2 }
       cur { print cur "\t" $0 }
       /^\.Lfunc_end:/ || /^\t\.end_amdhsa_kernel/ { cur = "" }' |
  LC_ALL=C sort -s -t "$(printf '\t')" -k1,1 |
  awk -F '\t' '$1 != cur { if (cur) close(cmd); cur = $1; cmd = "md5sum | sed s/-\\$/" cur "/" } { print substr($0, length($1) + 2) | cmd }'
