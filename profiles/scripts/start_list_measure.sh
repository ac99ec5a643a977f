#!/bin/bash
# The measurements behind profiles/r11_start_list_ab.json, on one GPU in one session.
#   start_list_measure.sh STEP OUTDIR PARENT_LIB
#     STEP        headline | in_context | profile | legs
#     OUTDIR      where the samples' JSON files and logs go
#     PARENT_LIB  librsem_hip.so built from the parent commit (python -m rsem_amd.build in a checkout of it)
# Every sample is a process of its own under a time limit; the first step that fails ends the script.
set -u
step=$1; O=$2; PARENT=$3
here="$(cd "$(dirname "$0")" && pwd)"
cd "$here/../.."
mkdir -p "$O"
export RSEM_WL_CACHE="${RSEM_WL_CACHE:-$(mktemp -d /dev/shm/rsem_wl_XXXXXX)}"
trap 'rm -rf "$RSEM_WL_CACHE"' EXIT
sample() {  # TAG OPT NAME CONFIG [DUMPDIR]; $LIB: the library
  local tag=$1 opt=$2 name=$3 cfg=$4 dump=${5:-}
  RSEM_HIP_LIB=${LIB:-} timeout -k 10 400 python "$here/start_list_sample.py" $tag $opt "$O/$name.json" $cfg $dump > "$O/$name.log" 2>&1 ||
    { echo "$name failed: rc $?"; tail -5 "$O/$name.log"; exit 1; }
}
case $step in
headline)  # parent / new / new with the option off, alternated five times; theta and counts of three parent and three new samples
  for i in 1 2 3 4 5; do
    LIB=$PARENT sample parent -1 parent_$i C3 "$O/dump_parent_$i"
    LIB= sample new 1 new_$i C3 "$O/dump_new_$i"
    LIB= sample off 0 off_$i C3
  done ;;
in_context)
  for i in 1 2; do
    timeout -k 10 400 python "$here/start_list_in_context.py" "$O/in_context_C3_$i.json" C3 > "$O/in_context_C3_$i.log" 2>&1 || { echo "in_context $i failed: rc $?"; exit 1; }
  done ;;
profile)   # kernel trace and the FETCH_SIZE counter, each in a run of its own, parent and new
  for arm in parent new; do
    if [ $arm = parent ]; then export RSEM_HIP_LIB=$PARENT; else unset RSEM_HIP_LIB; fi
    timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/trace_$arm" -o $arm -- python "$here/start_list_profile_run.py" 100 > "$O/trace_$arm.log" 2>&1 ||
      { echo "trace $arm failed: rc $?"; exit 1; }
    timeout -k 10 400 rocprofv3 --pmc FETCH_SIZE --output-format csv -d "$O/pmc_$arm" -o $arm -- python "$here/start_list_profile_run.py" 20 > "$O/pmc_$arm.log" 2>&1 ||
      { echo "pmc $arm failed: rc $?"; exit 1; }
  done ;;
legs)      # side legs, parent / new alternated P N P N P, two regions per sample
  export START_LIST_REGIONS=2
  for leg in C2 C2R C3X C3X30 C3Q32; do
    cfg=$leg; unset START_LIST_VALUE_BITS
    if [ $leg = C3Q32 ]; then cfg=C3; export START_LIST_VALUE_BITS=32; fi
    for i in 1 2 3; do
      LIB=$PARENT sample parent -1 ${leg}_parent_$i $cfg
      [ $i = 3 ] && break
      LIB= sample new 1 ${leg}_new_$i $cfg
    done
    rm -rf "$RSEM_WL_CACHE"/*
  done ;;
*) echo "unknown step $step"; exit 2 ;;
esac
echo "$step done: $O"
