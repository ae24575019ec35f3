#!/bin/bash
# tools/disc_select_check/run.sh -- builds the test network's launch wrappers host-only (AddressSanitizer + UBSan; no GPU, no Python,
# no HIP runtime) with the kernel launch as a recorder and runs them, in ONE process, under all eight settings of the library
# switches disc_vin_lds, disc_dynamic, disc_rec_tsum (include/xnwan_switches.h): every call's kernel, grid and arguments against
# fwd_select / rec_select evaluated directly.  One table row per setting; the last line must say "0 disagreements".  Then once
# more with --wrong (the expectation takes the switches inverted): that run must find disagreements, or the check cannot fail.
set -e -o pipefail
cd "$(dirname "$0")"
C=../../xnode_wan_pde_solver_amd/csrc
out=${TMPDIR:-/tmp}/disc_select_check.$$
mkdir -p "$out"
trap 'rm -rf "$out"' EXIT
F="--cuda-host-only -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I../../include -I$C -I. -Wno-unused-function -Wno-unused-variable"
/opt/rocm/bin/hipcc $F -c check.hip -o "$out/check.o" & p1=$!
/opt/rocm/bin/hipcc $F -c $C/xw_switches.hip -o "$out/switches.o" & p2=$!
wait $p1; wait $p2
/opt/rocm/bin/hipcc -fsanitize=address,undefined "$out/check.o" "$out/switches.o" -o "$out/check"
"$out/check"
"$out/check" --wrong | tail -1
