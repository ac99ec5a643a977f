#!/bin/bash
# End-to-end: rsem-simulate-reads, the reference program against the drop-in in both of its streams, on one MI355X host.
# usage: tools/e2e_simulate.sh [n_reads] [M] [out.json]        default: 1 000 000 reads, 200 000 transcripts, profiles/simulate_1m.json
# Input: the reference files tools/bin/gen_temp writes for M transcripts, a hand-written model of 100-base reads (the layout of
# tests/golden/make_fixtures.py) and a log-normal TPM table with a third of the transcripts at 0; single-end reads with qualities and
# read pairs with qualities.  The reference runs on its one thread, the drop-in with -p 16.  The reference stream's files must equal
# the reference program's (SHA-256); the counter stream's are only counted.  (At 200 000 transcripts a few values of the result files differ in their last digit: the
# reference's simulation.o is built with -ffast-math; the script lists the files and goes on.)  Each GPU step runs under its own time limit, and the
# script ends at the first step that fails.
set -o pipefail
N=${1:-1000000}; M=${2:-200000}; OUT=${3:-profiles/simulate_1m.json}; D=/tmp/e2esim_${N}_$M
here=$(cd "$(dirname "$0")/.." && pwd); cd "$here" || exit 1
REF=oracle/_ref/rsem-simulate-reads; NEW=rsem_amd/bin/rsem-simulate-reads
[ -x $REF ] && [ -x $NEW ] && [ -x tools/bin/gen_temp ] || { echo "e2e_simulate: build first (python __graft_entry__.py)" >&2; exit 1; }
rm -rf $D; mkdir -p $D
tools/bin/gen_temp $D 1000 $M 1 7 100 nosam | tail -1 || exit 1
python3 - "$D" <<'EOF' || exit 1
import os, sys
import numpy as np
sys.path.insert(0, os.path.join("tests", "golden"))
from make_fixtures import write_sim_model
d = sys.argv[1]
rng = np.random.default_rng(7)
write_sim_model(os.path.join(d, "se_q.model"), 1, rng, 100, 100)
write_sim_model(os.path.join(d, "pe_q.model"), 3, rng, 100, 100, frag_lo=150, frag_hi=450)
with open(os.path.join(d, "ref.ti")) as f:
    lines = f.read().split("\n")
M = int(lines[0].split()[0])
tpm = np.exp(rng.normal(0, 2, M))
tpm[rng.random(M) < 0.33] = 0.0
tpm = tpm / tpm.sum() * 1e6
with open(os.path.join(d, "tpm.results"), "w") as f:
    f.write("transcript_id\tgene_id\tlength\teffective_length\texpected_count\tTPM\tFPKM\tIsoPct\n")
    for i in range(M):
        rec = lines[1 + 6 * i: 7 + 6 * i]
        f.write("%s\t%s\t%s\t0\t0\t%.4f\t0\t0\n" % (rec[0].split("\t")[0], rec[1].split("\t")[0], rec[3].split()[1], tpm[i]))
EOF
export RSEM_SIM_TIMES=1
now() { date +%s.%N; }
for T in se_q pe_q; do
  a=$(now); $REF $D/ref $D/$T.model $D/tpm.results 0.05 $N $D/${T}_ref --seed 17 -q > $D/${T}_ref.stdout || exit 1; b=$(now)
  echo "$T reference_s $(awk "BEGIN{print $b - $a}")" | tee -a $D/times.txt
  a=$(now); timeout -k 10 600 $NEW $D/ref $D/$T.model $D/tpm.results 0.05 $N $D/${T}_new --seed 17 -q -p 16 > $D/${T}_new.stdout 2> $D/${T}_new.stderr || { cat $D/${T}_new.stderr; exit 1; }; b=$(now)
  echo "$T dropin_reference_stream_s $(awk "BEGIN{print $b - $a}")" | tee -a $D/times.txt
  grep "times:" $D/${T}_new.stderr | sed "s/^/$T reference_stream /" | tee -a $D/times.txt
  a=$(now); timeout -k 10 600 $NEW $D/ref $D/$T.model $D/tpm.results 0.05 $N $D/${T}_ctr --seed 17 -q -p 16 --sim-stream counter > $D/${T}_ctr.stdout 2> $D/${T}_ctr.stderr || { cat $D/${T}_ctr.stderr; exit 1; }; b=$(now)
  echo "$T dropin_counter_stream_s $(awk "BEGIN{print $b - $a}")" | tee -a $D/times.txt
  grep "times:" $D/${T}_ctr.stderr | sed "s/^/$T counter_stream /" | tee -a $D/times.txt
  same=1
  for f in $(cd $D && ls ${T}_ref*); do
    g=${f/${T}_ref/${T}_new}
    [ "$(sha256sum < $D/$f)" == "$(sha256sum < $D/$g)" ] || { echo "DIFF $f $g"; same=0; }
  done
  echo "$T files_equal $same" | tee -a $D/times.txt
  per=4; [ $T == pe_q ] && per=8
  echo "$T counter_reads $(( $(cat $D/${T}_ctr*.fq | wc -l) / per ))" | tee -a $D/times.txt
done
mkdir -p "$(dirname "$OUT")"
python3 - "$D/times.txt" "$OUT" "$N" "$M" <<'EOF' || exit 1
import json, sys
out = {"n_reads": int(sys.argv[3]), "M": int(sys.argv[4]), "host": "both sides on the same MI355X host", "reference_threads": 1, "dropin_threads": 16, "seed": 17,
       "note": "seconds are wall clock of the whole program; *_ms are summed over the batches: words on the host's generator thread, upload / search / body by HIP events"}
for line in open(sys.argv[1]):
    w = line.split()
    c = out.setdefault(w[0], {})
    if w[2] == "rsem-simulate-reads":  # "<type> <stream>_stream rsem-simulate-reads times: k v k v ..."
        c[w[1]] = {k: float(v) for k, v in zip(w[4::2], w[5::2])}
    else:
        c[w[1]] = float(w[2])
json.dump(out, open(sys.argv[2], "w"), indent=1)
print(open(sys.argv[2]).read())
EOF
rm -rf $D
