// rsem-simulate-reads on MI355X: same argv, same files and same stdout as the reference program (simulation.cpp), whose reads
// every fixture and every end-to-end workload of this repository starts from.
//
//   rsem-simulate-reads reference_name estimated_model_file estimated_isoform_results theta0 N output_name [--seed seed] [-q]
//                       [--device d] [-p threads] [--sim-stream reference|counter]
//
// writes  output_name.fa | .fq | _1.fa _2.fa | _1.fq _2.fq   the reads, named rid_dir_sid_pos[_insertL] (simulation.cpp:60-84,158-165)
//         output_name.sim.isoforms.results, .sim.genes.results [, .sim.alleles.results]   (WriteResults.h:481-635)
//
// The reference draws read after read from one MT19937 stream on one thread.  Here the tables of the model go to the GPU once
// (rsem_sim_create, rsem_amd/csrc/simulate.hip) and the reads come back in batches, which -p threads turn into text while the device
// draws the next batch.
//   --sim-stream reference (the default): the reference's own stream, searched on the device for the attempts it holds: every file
//       equals the reference program's for the same --seed, byte for byte.
//   --sim-stream counter: every uniform is a Philox4x32-10 word at counter (read, attempt, draw / 4) keyed by the seed: the same draw
//       program, the reference's distribution and not its reads; a pure function of the seed, whatever the batch size and -p.
// Where the reference leaves defined ground the program stops with a message: a paired-end insert shorter than
// every mate length, a read longer than the no-quality profile, a quality above 93, a read that fails 2^20 attempts in a row.
#include <ctime>
#include <thread>

#include "../../../include/rsem_hip.h"
#include "simulate_host.hpp"

using namespace rsemh;

namespace {

void check(int rc, const char* what) {
    if (rc != RSEM_OK) die("%s failed: %s (%s)", what, rsem_hip_strerror(rc), rsem_hip_last_error());
}

// the arrays of one batch on the host
struct HostBatch {
    rsem_sim_batch b{};
    std::vector<int32_t> i32;
    std::vector<uint32_t> attempts;
    std::vector<uint8_t> bytes;
    void size(int64_t n, int stride) {
        i32.resize((size_t)n * 6);
        attempts.resize((size_t)n);
        bytes.resize((size_t)n * stride * 4);
        b.capacity = n; b.stride = stride;
        b.sid = i32.data(); b.dir = b.sid + n; b.pos = b.dir + n; b.insert_l = b.pos + n; b.len1 = b.insert_l + n; b.len2 = b.len1 + n;
        b.attempts = attempts.data();
        b.seq1 = bytes.data(); b.qual1 = b.seq1 + (size_t)n * stride; b.seq2 = b.qual1 + (size_t)n * stride; b.qual2 = b.seq2 + (size_t)n * stride;
    }
};

char* put_number(char* p, long long v) {
    char tmp[24];
    int n = 0;
    if (v < 0) { *p++ = '-'; v = -v; }
    do { tmp[n++] = (char)('0' + v % 10); v /= 10; } while (v);
    while (n) *p++ = tmp[--n];
    return p;
}

// the text of reads [lo, hi) of a batch (SingleRead.h:52-55, SingleReadQ.h:57-60 and the paired classes)
void format_reads(const rsem_sim_batch& b, int64_t lo, int64_t hi, long long rid0, bool fastq, bool paired, std::string out[2]) {
    char name[128];
    for (int64_t i = lo; i < hi; i++) {
        char* p = name;
        p = put_number(p, rid0 + i); *p++ = '_';
        p = put_number(p, b.dir[i]); *p++ = '_';
        p = put_number(p, b.sid[i]); *p++ = '_';
        p = put_number(p, b.pos[i]);
        if (paired) { *p++ = '_'; p = put_number(p, b.insert_l[i]); }
        const size_t nl = (size_t)(p - name), at = (size_t)i * (size_t)b.stride;
        for (int k = 0; k < (paired ? 2 : 1); k++) {
            std::string& o = out[k];
            const uint8_t* seq = (k ? b.seq2 : b.seq1) + at;
            const uint8_t* qual = (k ? b.qual2 : b.qual1) + at;
            const size_t len = (size_t)(k ? b.len2[i] : b.len1[i]);
            o.push_back(fastq ? '@' : '>');
            o.append(name, nl);
            if (paired) { o.push_back('/'); o.push_back((char)('1' + k)); }
            o.push_back('\n');
            o.append((const char*)seq, len);
            o.push_back('\n');
            if (fastq) {
                o.append("+\n");
                o.append((const char*)qual, len);
                o.push_back('\n');
            }
        }
    }
}

double now_s() {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

// writeResultsSimulation (WriteResults.h:481-635)
void write_results_simulation(int M, const std::string& refName, const std::string& outName, const Transcripts& T, const std::vector<double>& eel,
                              const std::vector<double>& counts) {
    GroupInfo genes, gt, ta;
    if (!genes.load(refName + ".grp")) die("Cannot open %s.grp! It may not exist.", refName.c_str());
    const bool alleleS = is_allele_specific(refName);
    if (alleleS && (!gt.load(refName + ".gt") || !ta.load(refName + ".ta"))) die("Cannot load %s.gt / %s.ta!", refName.c_str(), refName.c_str());
    for (int i = 1; i <= M; i++)
        if (!(eel[i] > kEpsilon || counts[i] <= kEpsilon)) die("An isoform whose effecitve length < %.6f got sampled!", kMinEel);  // WriteResults.h:506
    std::vector<double> tpm, fpkm;
    calc_expression(M, counts, eel, tpm, fpkm);
    std::vector<int> tlens(M + 1, 0);
    for (int j = 1; j <= M; j++) tlens[j] = T.t[j].length;
    const int m = genes.m;
    const Level G = roll_up(genes.starts, m, (size_t)M + 1, counts.data(), tpm.data(), fpkm.data(), tlens.data(), eel.data());
    auto open_out = [&](const char* suffix) {
        const std::string path = outName + suffix;
        FILE* fo = fopen(path.c_str(), "w");
        if (!fo) die("Cannot open %s for writing!", path.c_str());
        return fo;
    };
    Level A;
    std::vector<double> gt_pct;
    if (alleleS) {
        const int mt = ta.m;
        A = roll_up(ta.starts, mt, (size_t)M + 1, counts.data(), tpm.data(), fpkm.data(), tlens.data(), eel.data());
        gt_pct.assign(mt, 0.0);
        for (int g = 0; g < m; g++)
            if (G.tpm[g] >= kEpsilon)
                for (int t = gt.starts[g]; t < gt.starts[g + 1]; t++) gt_pct[t] = A.tpm[t] / G.tpm[g];
        FILE* fo = open_out(".sim.alleles.results");
        fprintf(fo, "allele_id\ttranscript_id\tgene_id\tlength\teffective_length\tcount\tTPM\tFPKM\tAlleleIsoPct\tAlleleGenePct\n");
        for (int i = 1; i <= M; i++)
            fprintf(fo, "%s\t%s\t%s\t%d\t%.2f\t%.2f\t%.2f\t%.2f\t%.2f\t%.2f\n", T.t[i].seqname.c_str(), T.t[i].transcript_id.c_str(), T.t[i].gene_id.c_str(), tlens[i], eel[i],
                    counts[i], tpm[i], fpkm[i], A.share[i] * 1e2, G.share[i] * 1e2);
        fclose(fo);
    }
    FILE* fo = open_out(".sim.isoforms.results");
    fprintf(fo, "transcript_id\tgene_id\tlength\teffective_length\tcount\tTPM\tFPKM\tIsoPct\n");
    if (!alleleS) {
        for (int i = 1; i <= M; i++)
            fprintf(fo, "%s\t%s\t%d\t%.2f\t%.2f\t%.2f\t%.2f\t%.2f\n", T.t[i].transcript_id.c_str(), T.t[i].gene_id.c_str(), tlens[i], eel[i], counts[i], tpm[i], fpkm[i],
                    G.share[i] * 1e2);
    } else {
        for (int i = 0; i < ta.m; i++) {
            const TranscriptInfo& t = T.t[ta.starts[i]];
            fprintf(fo, "%s\t%s\t%.2f\t%.2f\t%.2f\t%.2f\t%.2f\t%.2f\n", t.transcript_id.c_str(), t.gene_id.c_str(), A.len[i], A.eel[i], A.counts[i], A.tpm[i], A.fpkm[i],
                    gt_pct[i] * 1e2);
        }
    }
    fclose(fo);
    fo = open_out(".sim.genes.results");
    fprintf(fo, "gene_id\ttranscript_id(s)\tlength\teffective_length\tcount\tTPM\tFPKM\n");
    for (int g = 0; g < m; g++) {
        const int b = genes.starts[g], e = genes.starts[g + 1];
        fprintf(fo, "%s\t", T.t[b].gene_id.c_str());
        const std::string* prev = nullptr;
        for (int j = b; j < e; j++) {
            const std::string& tid = T.t[j].transcript_id;
            if (prev && *prev == tid) continue;
            if (prev) fputc(',', fo);
            fputs(tid.c_str(), fo);
            prev = &tid;
        }
        fprintf(fo, "\t%.2f\t%.2f\t%.2f\t%.2f\t%.2f\n", G.len[g], G.eel[g], G.counts[g], G.tpm[g], G.fpkm[g]);
    }
    fclose(fo);
}

void usage() {  // simulation.cpp:144-169
    printf("Usage: rsem-simulate-reads reference_name estimated_model_file estimated_isoform_results theta0 N output_name [--seed seed] [-q]\n\n");
    printf("Parameters:\n\n");
    printf("reference_name: The name of RSEM references, which should be already generated by 'rsem-prepare-reference'\n");
    printf("estimated_model_file: This file describes how the RNA-Seq reads will be sequenced given the expression levels. It determines what kind of reads will be simulated (single-end/paired-end, w/o quality score) and includes parameters for fragment length distribution, read start position distribution, sequencing error models, etc. Normally, this file should be learned from real data using 'rsem-calculate-expression'. The file can be found under the 'sample_name.stat' folder with the name of 'sample_name.model'\n");
    printf("estimated_isoform_results: This file contains expression levels for all isoforms recorded in the reference. It can be learned using 'rsem-calculate-expression' from real data. The corresponding file users want to use is 'sample_name.isoforms.results'. If simulating from user-designed expression profile is desired, start from a learned 'sample_name.isoforms.results' file and only modify the 'TPM' column. The simulator only reads the TPM column. But keeping the file format the same is required. If the RSEM references built are aware of allele-specific transcripts, 'sample_name.alleles.results' should be used instead.\n");
    printf("theta0: This parameter determines the fraction of reads that are coming from background \"noise\" (instead of from a transcript). It can also be estimated using 'rsem-calculate-expression' from real data. Users can find it as the first value of the third line of the file 'sample_name.stat/sample_name.theta'.\n");
    printf("N: The total number of reads to be simulated. If 'rsem-calculate-expression' is executed on a real data set, the total number of reads can be found as the 4th number of the first line of the file 'sample_name.stat/sample_name.cnt'.\n");
    printf("output_name: Prefix for all output files.\n");
    printf("--seed seed: Set seed for the random number generator used in simulation. The seed should be a 32-bit unsigned integer.\n");
    printf("-q: Set it will stop outputting intermediate information.\n\n");
    printf("Outputs:\n\n");
    printf("output_name.sim.isoforms.results, output_name.sim.genes.results: Expression levels estimated by counting where each simulated read comes from.\n");
    printf("output_name.sim.alleles.results: Allele-specific expression levels estimated by counting where each simulated read comes from.\n\n");
    printf("output_name.fa if single-end without quality score;\noutput_name.fq if single-end with quality score;\noutput_name_1.fa & output_name_2.fa if paired-end without quality score;\noutput_name_1.fq & output_name_2.fq if paired-end with quality score.\n\n");
    printf("Format of the header line: Each simulated read's header line encodes where it comes from. The header line has the format:\n\n");
    printf("\t{>/@}_rid_dir_sid_pos[_insertL]\n\n");
    printf("{>/@}: Either '>' or '@' must appear. '>' appears if FASTA files are generated and '@' appears if FASTQ files are generated\n");
    printf("rid: Simulated read's index, numbered from 0\n");
    printf("dir: The direction of the simulated read. 0 refers to forward strand ('+') and 1 refers to reverse strand ('-')\n");
    printf("sid: Represent which transcript this read is simulated from. It ranges between 0 and M, where M is the total number of transcripts. If sid=0, the read is simulated from the background noise. Otherwise, the read is simulated from a transcript with index sid. Transcript sid's transcript name can be found in the 'transcript_id' column of the 'sample_name.isoforms.results' file (at line sid + 1, line 1 is for column names)\n");
    printf("pos: The start position of the simulated read in strand dir of transcript sid. It is numbered from 0\n");
    printf("insertL: Only appear for paired-end reads. It gives the insert length of the simulated read.\n\n");
    printf("Example:\n\n");
    printf("Suppose we want to simulate 50 millon single-end reads with quality scores and use the parameters learned from [Example](#example). In addition, we set theta0 as 0.2 and output_name as 'simulated_reads'. The command is:\n\n");
    printf("\trsem-simulate-reads /ref/mouse_125 mmliver_single_quals.stat/mmliver_single_quals.model mmliver_single_quals.isoforms.results 0.2 50000000 simulated_reads\n");
    exit(-1);
}

const char* status_text(int s) {
    switch (s) {
        case RSEM_SIM_ATTEMPT_CAP: return "a read failed every one of its attempts (2^20 unless RSEM_SIM_ATTEMPT_CAP says otherwise): with this model and these transcripts it cannot be drawn";
        case RSEM_SIM_SHORT_INSERT: return "an insert shorter than every mate length was drawn: the fragment length distribution starts below the mate length distribution";
        case RSEM_SIM_PAST_PROFILE: return "a read longer than the model's profile was drawn";
        case RSEM_SIM_QUALITY_RANGE: return "a quality score above 93 was drawn";
        default: return "unknown status";
    }
}

}  // namespace

int main(int argc, char* argv[]) {
    // this program's own options come out of the argument list first; what is left is the reference's (simulation.cpp:143,172-186)
    int device = 0, threads = 1;
    bool counter = false;
    std::vector<char*> av;
    for (int i = 0; i < argc; i++) {
        if (i >= 7 && !strcmp(argv[i], "--device") && i + 1 < argc) device = atoi(argv[++i]);
        else if (i >= 7 && !strcmp(argv[i], "-p") && i + 1 < argc) threads = std::max(1, atoi(argv[++i]));
        else if (i >= 7 && !strcmp(argv[i], "--sim-stream") && i + 1 < argc) {
            const char* v = argv[++i];
            if (!strcmp(v, "counter")) counter = true;
            else if (!strcmp(v, "reference")) counter = false;
            else die("--sim-stream: 'reference' or 'counter' is expected, not '%s'", v);
        } else av.push_back(argv[i]);
    }
    const int ac = (int)av.size();
    if (ac < 7 || ac > 10) usage();
    bool quiet = false, have_seed = false;
    unsigned int seed = 0;
    for (int i = 7; i < ac; i++) {
        if (!strcmp(av[i], "-q")) quiet = true;
        if (!strcmp(av[i], "--seed")) {
            char* end = nullptr;
            if (i + 1 >= ac) die("--seed needs a value");
            seed = (unsigned int)strtoul(av[i + 1], &end, 10);
            if (end == av[i + 1]) die("--seed: a 32-bit unsigned integer is expected, not '%s'", av[i + 1]);
            have_seed = true;
        }
    }
    if (!have_seed) seed = (unsigned int)time(NULL);  // simulation.cpp:186
    const bool verbose = !quiet;
    const std::string refName = av[1], modelF = av[2], resultsF = av[3], outName = av[6];

    SimInputs in;
    load_sim_inputs(in, refName, modelF, resultsF, av[4], verbose);
    const int M = in.R.M;
    const Model& model = in.model;
    const Transcripts& T = in.T;
    const std::vector<double>& eel = in.eel;
    const rsem_sim_model& sm = in.sm;
    const bool fastq = model.hasQ(), paired = model.paired();
    const long long N = atoi(av[5]);  // simulation.cpp:207
    rsem_sim_knobs knobs;
    check(rsem_sim_read_knobs(&knobs), "reading the RSEM_SIM_* knobs");
    rsem_sim* sim = nullptr;
    check(rsem_sim_create(&sim, &sm, device), "rsem_sim_create");
    int32_t max_len = 0, plain = 0;
    check(rsem_sim_info(sim, &max_len, &plain), "rsem_sim_info");
    fprintf(stderr, "rsem-simulate-reads: --sim-stream %s (%s), seed %u\n", counter ? "counter" : "reference",
            counter ? "Philox4x32-10 per read and attempt: the reference's distribution, not its reads" : "the reference's MT19937 stream: its reads", seed);
    if (!counter) check(rsem_sim_reference_begin(sim, seed), "rsem_sim_reference_begin");

    // the read files (simulation.cpp:60-84)
    const int n_os = paired ? 2 : 1;
    FILE* os[2] = {nullptr, nullptr};
    for (int k = 0; k < n_os; k++) {
        char suffix[16];
        if (paired) snprintf(suffix, sizeof suffix, "_%d.%s", k + 1, fastq ? "fq" : "fa");
        else snprintf(suffix, sizeof suffix, ".%s", fastq ? "fq" : "fa");
        const std::string path = outName + suffix;
        os[k] = fopen(path.c_str(), "w");
        if (!os[k]) die("Cannot open %s for writing!", path.c_str());
        setvbuf(os[k], nullptr, _IOFBF, 1 << 20);
    }

    // batches: the device draws batch k + 1 while the threads format batch k and this side writes it
    const long long batch = (long long)std::min<uint64_t>(knobs.batch_reads, (uint64_t)std::max<long long>(N, 1));
    HostBatch hb[2];
    hb[0].size(batch, max_len);
    hb[1].size(batch, max_len);
    double t_device = 0, t_format = 0, t_write = 0, words_ms = 0, upload_ms = 0, search_ms = 0, body_ms = 0, download_ms = 0;
    long long n_chunks = 0;
    std::thread writer;
    auto flush = [&](const HostBatch* h, long long rid0) {
        const rsem_sim_batch& b = h->b;
        const double t0 = now_s();
        const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(threads, b.n_reads / 256 + 1));
        std::vector<std::string> part((size_t)nt * 2);
        parallel_for(nt, [&](int t) {
            const int64_t lo = b.n_reads * t / nt, hi = b.n_reads * (t + 1) / nt;
            part[2 * t].reserve((size_t)(hi - lo) * (size_t)(2 * max_len + 40));
            if (paired) part[2 * t + 1].reserve((size_t)(hi - lo) * (size_t)(2 * max_len + 40));
            format_reads(b, lo, hi, rid0, fastq, paired, &part[2 * t]);
        });
        const double t1 = now_s();
        for (int t = 0; t < nt; t++)
            for (int k = 0; k < n_os; k++) fwrite(part[2 * t + k].data(), 1, part[2 * t + k].size(), os[k]);
        t_format += t1 - t0;
        t_write += now_s() - t1;
    };
    long long done = 0;
    for (int turn = 0; done < N; turn ^= 1) {
        HostBatch& h = hb[turn];
        const long long n = std::min(batch, N - done);
        const double t0 = now_s();
        if (counter) check(rsem_sim_counter_batch(sim, (uint64_t)seed, (uint64_t)done, n, &h.b), "rsem_sim_counter_batch");
        else check(rsem_sim_reference_batch(sim, n, &h.b), "rsem_sim_reference_batch");
        t_device += now_s() - t0;
        if (h.b.status != RSEM_SIM_OK) {
            if (writer.joinable()) writer.join();
            die("rsem-simulate-reads: %s (reads %lld to %lld).", status_text(h.b.status), done, done + n - 1);
        }
        if (h.b.n_reads != n) die("rsem-simulate-reads: a batch of %lld reads came back with %lld", n, (long long)h.b.n_reads);
        words_ms += h.b.words_ms; upload_ms += h.b.upload_ms; search_ms += h.b.search_ms; body_ms += h.b.body_ms; download_ms += h.b.download_ms;
        n_chunks += h.b.n_chunks;
        if (writer.joinable()) writer.join();
        const long long rid0 = done;
        writer = std::thread(flush, &h, rid0);
        if (verbose)
            for (long long g = (done / 1000000 + 1) * 1000000; g <= done + n; g += 1000000) { printf("GEN %lld\n", g); fflush(stdout); }  // simulation.cpp:125
        done += n;
    }
    if (writer.joinable()) writer.join();
    for (int k = 0; k < n_os; k++) fclose(os[k]);

    std::vector<uint64_t> icounts(M + 1, 0);
    uint64_t resim = 0;
    check(rsem_sim_totals(sim, icounts.data(), &resim), "rsem_sim_totals");
    printf("Total number of resimulation is %llu\n", (unsigned long long)resim);  // simulation.cpp:129
    std::vector<double> counts(M + 1, 0.0);
    for (int i = 0; i <= M; i++) counts[i] = (double)icounts[i];
    write_results_simulation(M, refName, outName, T, eel, counts);
    rsem_sim_destroy(sim);
    if (getenv("RSEM_SIM_TIMES"))  // one line for tools/e2e_simulate.sh
        fprintf(stderr, "rsem-simulate-reads times: device_calls_s %.3f format_s %.3f write_s %.3f words_ms %.1f upload_ms %.1f search_ms %.1f body_ms %.1f download_ms %.1f chunks %lld "
                        "threads %d plain %d\n", t_device, t_format, t_write, words_ms, upload_ms, search_ms, body_ms, download_ms, n_chunks, threads, plain);
    return 0;
}
