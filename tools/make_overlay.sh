#!/bin/bash
# An RSEM installation directory in which some programs are the drop-ins of this repo.
#   tools/make_overlay.sh <rsem_dir> <out_dir> [program ... | --none]      default programs: the four pipeline drop-ins, rsem-tbam2gbam, rsem-bam2wig, rsem-bam2readdepth
#                                                                           the three reference-preparation programs, rsem-sam-validator, rsem-get-unique,
#                                                                           rsem-scan-for-paired-end-reads and rsem-simulate-reads
# rsem-calculate-expression, rsem-prepare-reference, convert-sam-for-rsem and rsem-plot-transcript-wiggles each put THEIR OWN
# directory first in PATH (rsem-calculate-expression:12, convert-sam-for-rsem:7-12: FindBin::RealBin, symlinks resolved) and run bare
# program names, so a drop-in has to sit next to the driver: <out_dir> gets COPIES of these four Perl scripts and of the *.pm
# modules (a symlinked script would resolve back to <rsem_dir> and run the programs there), symlinks to everything else in
# <rsem_dir>, and symlinks to rsem_amd/bin/<program> for the named programs (their rpath $ORIGIN/.. finds librsem_hip.so through
# the resolved path).
set -e
src=$(cd "$1" && pwd); out=$2; shift 2
here=$(cd "$(dirname "$0")/.." && pwd)
progs=("$@"); [ ${#progs[@]} -eq 0 ] && progs=(rsem-parse-alignments rsem-run-em rsem-run-gibbs rsem-calculate-credibility-intervals rsem-tbam2gbam rsem-bam2wig rsem-bam2readdepth rsem-extract-reference-transcripts rsem-synthesis-reference-transcripts rsem-preref rsem-sam-validator rsem-get-unique rsem-scan-for-paired-end-reads rsem-simulate-reads)
[ "${progs[0]}" == "--none" ] && progs=()
mkdir -p "$out"
for f in "$src"/*; do
  b=$(basename "$f")
  case "$b" in
    *.pm|rsem-calculate-expression|rsem-prepare-reference|convert-sam-for-rsem|rsem-plot-transcript-wiggles) cp "$f" "$out/$b" ;;
    obj|gen|*.a) ;;
    *) ln -sfn "$f" "$out/$b" ;;
  esac
done
for p in "${progs[@]}"; do
  [ -x "$here/rsem_amd/bin/$p" ] || { echo "make_overlay: $here/rsem_amd/bin/$p is missing (python -m rsem_amd.build)" >&2; exit 1; }
  ln -sfn "$here/rsem_amd/bin/$p" "$out/$p"
done
echo "$out: ${progs[*]} from $here/rsem_amd/bin, the rest from $src"
