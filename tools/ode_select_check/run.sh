#!/bin/bash
# tools/ode_select_check/run.sh -- builds ode_select_check.hip (host code only, AddressSanitizer + UBSan; no GPU, no Python) in its three
# configurations and runs each with XW_DUO_SPREAD unset, 0 and 1.  Every line must end in "0 disagreements, 0 table slots never reached";
# the exit status is 0 only then (a build that fails, a disagreement and a slot never reached all end the script with a status that is not 0).
set -e -o pipefail
cd "$(dirname "$0")"
C=../../xnode_wan_pde_solver_amd/csrc
out=${TMPDIR:-/tmp}/ode_select_check.$$
mkdir -p "$out"
trap 'rm -rf "$out"' EXIT
F="--cuda-host-only -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I../../include -I$C -I. -Wno-unused-function"
build() {
  name=$1; shift
  /opt/rocm/bin/hipcc $F "$@" -c ode_select_check.hip -o "$out/$name.o"
  /opt/rocm/bin/hipcc -fsanitize=address,undefined "$out/$name.o" "$out/switches.o" -o "$out/$name"
}
/opt/rocm/bin/hipcc $F -c $C/xw_switches.hip -o "$out/switches.o"      # (the library's switches: main sets duo_spread through them)
build m4 -DXW_ODE_H=20 -DXW_ODE_K=10 & p1=$!
build m16 -DXW_ODE_H=64 -DXW_ODE_K=16 -DXW_ODE_WIDE16 -DXW_ODE_FWD_WAVES=1 & p2=$!
build recomp -DXW_ODE_H=64 -DXW_ODE_K=16 -DXW_ODE_WIDE16 -DXW_ODE_FWD_WAVES=1 -DXW_ODE_PART_RECOMP & p3=$!
wait $p1; wait $p2; wait $p3
for n in m4 m16 recomp; do
  env -u XW_DUO_SPREAD "$out/$n" | tail -1
  XW_DUO_SPREAD=0 "$out/$n" | tail -1
  XW_DUO_SPREAD=1 "$out/$n" | tail -1
done
