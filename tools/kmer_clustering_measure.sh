#!/bin/bash
# rsem-for-ebseq-calculate-clustering-info on a generated FASTA: whole-program wall clock of three fresh processes, the library's
# upload_ms / kernel_ms from the program's own lines, one run cut into batches, and (with "trace") a rocprofv3 kernel trace of one
# more run.  The output file's checksum is printed for the comparison with the reference program's file for the same FASTA
# (tools/gen_shared_fasta.py gives the same file for the same arguments on any host).
#   tools/kmer_clustering_measure.sh OUTDIR [ENTRIES BASES K [trace]]
set -o pipefail
out=$1; entries=${2:-100000}; bases=${3:-200000000}; k=${4:-25}; trace=$5
here=$(cd "$(dirname "$0")/.." && pwd)
prog=$here/rsem_amd/bin/rsem-for-ebseq-calculate-clustering-info
tmp=$(mktemp -d); trap 'rm -rf "$tmp"' EXIT
mkdir -p "$out"
python "$here/tools/gen_shared_fasta.py" "$tmp/in.fa" --entries "$entries" --bases "$bases" --seed 1 > "$out/gen.log" 2>&1 || { cat "$out/gen.log"; exit 1; }
sha256sum "$tmp/in.fa" | cut -d' ' -f1 > "$out/fasta.sha256"
(grep -m1 'model name' /proc/cpuinfo; /opt/rocm/bin/rocminfo | grep -m1 gfx) > "$out/host.log" 2>&1
for r in 1 2 3; do
  s=$(date +%s%N)
  timeout -k 10 600 "$prog" "$k" "$tmp/in.fa" "$tmp/out.$r.ump" > "$out/run$r.log" 2>&1 || { echo "run $r failed: $?"; tail -5 "$out/run$r.log"; exit 1; }
  e=$(date +%s%N)
  echo "run $r wall $(( (e - s) / 1000000 )) ms" | tee -a "$out/wall.log"
  grep -E '^\[device\]|mers are sorted' "$out/run$r.log"
done
sha256sum "$tmp"/out.?.ump | cut -d' ' -f1 | sort -u > "$out/ump.sha256"
cat "$out/ump.sha256"
kmers=$(sed -n 's/^All \([0-9]*\) .*/\1/p' "$out/run1.log")
RSEM_KMER_BATCH_ITEMS=$(( kmers / 6 + 1 )) timeout -k 10 600 "$prog" "$k" "$tmp/in.fa" "$tmp/out.b.ump" > "$out/run_batched.log" 2>&1 || { echo "batched run failed: $?"; exit 1; }
grep -E '^\[device\]|mers are sorted' "$out/run_batched.log"
cmp "$tmp/out.1.ump" "$tmp/out.b.ump" && echo "batched output identical"
if [ "$trace" == "trace" ]; then
  timeout -k 10 900 rocprofv3 --kernel-trace --stats -d "$out/trace" -o kmer --output-format csv -- "$prog" "$k" "$tmp/in.fa" "$tmp/out.t.ump" -q > "$out/trace.log" 2>&1 || { echo "trace run failed: $?"; tail -5 "$out/trace.log"; exit 1; }
  f=$(find "$out/trace" -name '*kernel_stats.csv' | head -1)
  [ -n "$f" ] && cut -c1-160 "$f" | head -20
  find "$out/trace" -name '*kernel_trace.csv' -delete
fi
