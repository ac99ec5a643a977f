// rsem-extract-reference-transcripts on MI355X: same argv, same files as the reference program (extractRef.cpp).
//
//   rsem-extract-reference-transcripts refName quiet gtfF sources hasMappingFile [mappingFile] chromosome_file_1 [...] [--device d]
//
// writes  refName.grp, refName.ti, refName.chrlist, refName.transcripts.fa
//
// The reference reads every chromosome line by line into a std::string and cuts the exons out of it on one thread.  Here the host
// finds the header lines and parses the GTF; the chromosomes' bytes go to the GPU a batch at a time, where the line ends are dropped,
// the letters checked and mapped (rsem_refseq_load) and the exons written -- reverse-complemented on the '-' strand -- to the places
// the transcripts have in one output store (rsem_refseq_gather), which is downloaded once (host/refprep_host.hpp,
// rsem_amd/csrc/refseq.hip).  Errors come in the reference's order: record after record, a record's first bad character before its
// transcripts' boundary checks.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "refprep_host.hpp"

using namespace rsemh;

int main(int argc, char* argv[]) {
    Stages stages;
    const int device = strip_device(argc, argv);
    int has_mapping = 0;
    if (argc < 7 || ((has_mapping = atoi(argv[5])) && argc < 8)) {
        printf("Usage: rsem-extract-reference-transcripts refName quiet gtfF sources hasMappingFile [mappingFile] chromosome_file_1 [chromosome_file_2 ...]\n");
        exit(-1);
    }
    const bool verbose = !atoi(argv[2]);
    std::map<std::string, std::string> mi_table, unused;
    if (has_mapping) load_mapping_info(1, argv[6], mi_table, unused);
    std::set<std::string> sources;
    if (strcmp(argv[4], "None")) {  // parseSources (extractRef.cpp:59-65): strtok on ','
        std::string s = argv[4];
        for (char* p = strtok(&s[0], ","); p; p = strtok(nullptr, ",")) sources.insert(p);
    }
    GtfResult G = parse_gtf(argv[3], sources, has_mapping != 0, mi_table, verbose);
    const int M0 = (int)G.tr.size() - 1;

    // where every transcript lies in the output store: fixed by the exon structures alone
    std::vector<uint64_t> off((size_t)M0 + 2, 0);
    for (int i = 1; i <= M0; i++) off[i + 1] = off[i] + (uint64_t)G.tr[i].length;
    std::vector<uint8_t> extracted((size_t)M0 + 1, 0);
    rsem_refseq* h = nullptr;
    refseq_try(rsem_refseq_create(&h, device, off[M0 + 1]), "rsem_refseq_create");

    struct Chr { std::string name; uint64_t len; };
    std::vector<Chr> chrvec;
    std::string seqname;  // lives across records AND files: a header without a name keeps the one before (extractRef.cpp:322,338-339)
    std::vector<int64_t> s_src;
    std::vector<uint32_t> s_first, s_len, s_flags;
    std::vector<uint64_t> s_dst;
    auto flush = [&]() {  // the segments ascend in the store, as one writer a byte asks for
        const size_t n = s_src.size();
        if (!n) return;
        std::vector<size_t> order(n);
        for (size_t i = 0; i < n; i++) order[i] = i;
        std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return s_dst[a] < s_dst[b]; });
        std::vector<int64_t> src(n);
        std::vector<uint32_t> first(n), len(n), flags(n);
        std::vector<uint64_t> dst(n);
        for (size_t i = 0; i < n; i++) { src[i] = s_src[order[i]]; first[i] = s_first[order[i]]; len[i] = s_len[order[i]]; flags[i] = s_flags[order[i]]; dst[i] = s_dst[order[i]]; }
        refseq_try(rsem_refseq_gather(h, (int64_t)n, src.data(), first.data(), len.data(), dst.data(), flags.data()), "rsem_refseq_gather");
        s_src.clear(); s_first.clear(); s_len.clear(); s_flags.clear(); s_dst.clear();
    };

    const int start = has_mapping ? 7 : 6;
    for (int i = start; i < argc; i++) {
        MappedFile f;
        if (!f.open(argv[i])) die("Cannot open %s! It may not exist.", argv[i]);
        const std::vector<FastaRecord> recs = frame_fasta(f.data, f.size);
        std::vector<std::string> names(recs.size());
        std::vector<uint8_t> keep(recs.size());
        for (size_t r = 0; r < recs.size(); r++) {
            first_token(f.data + recs[r].head_lo, f.data + recs[r].head_hi, seqname);
            names[r] = seqname;
            keep[r] = G.sn2tr.count(seqname) ? 1 : 0;
        }
        stages.device_begin();
        std::set<std::string> in_batch;  // a name that comes again gathers again, behind the earlier one: the last occurrence wins
        load_file(h, RSEM_REFSEQ_CHECKED, f.data, recs, &keep,
                  [&](int64_t r, uint64_t n_bases, int64_t bad) {
                      if (bad >= 0) die_bad_character(argv[i], f.data, (uint64_t)bad);
                      if (recs[r].hi == recs[r].lo || (keep[r] && n_bases == 0) || (!keep[r] && std::all_of(f.data + recs[r].lo, f.data + recs[r].hi, [](char c) { return c == '\n'; })))
                          die("FASTA file %s: the record %s has an empty sequence!", argv[i], names[r].c_str());  // (the reference stops at an assert here)
                      if (!keep[r]) return;
                      chrvec.push_back({names[r], n_bases});
                      if (!in_batch.insert(names[r]).second) flush();
                      for (int id : G.sn2tr[names[r]]) {
                          const RefTranscript& t = G.tr[id];
                          const int s = (int)t.structure.size();
                          if (t.structure[0].start < 1 || (uint64_t)t.structure[s - 1].end > n_bases) {  // Transcript.h:95-98
                              fprintf(stderr, "Transcript %s is out of chromosome %s's boundary!\n", t.transcript_id.c_str(), t.seqname.c_str());
                              exit(-1);
                          }
                          uint64_t d = off[id];
                          for (int k = 0; k < s; k++) {
                              const Interval& iv = t.structure[t.strand == '+' ? k : s - 1 - k];
                              const uint32_t len = (uint32_t)(iv.end - iv.start + 1);
                              s_src.push_back(r); s_first.push_back((uint32_t)(iv.start - 1)); s_len.push_back(len);
                              s_flags.push_back(t.strand == '+' ? 0u : RSEM_REFSEQ_RC); s_dst.push_back(d);
                              d += len;
                          }
                          extracted[id] = 1;
                      }
                  },
                  [&](int64_t, int64_t) { flush(); in_batch.clear(); });
        stages.device_end();
        if (verbose) printf("%s is processed!\n", argv[i]);
    }
    std::stable_sort(chrvec.begin(), chrvec.end(), [](const Chr& a, const Chr& b) { return a.name < b.name; });

    // shrink (extractRef.cpp:218-254)
    std::vector<int> ids;
    int n_warns = 0;
    for (int i = 1; i <= M0; i++) {
        if (!extracted[i]) {
            if (++n_warns <= kMaxWarns)
                fprintf(stderr, "Warning: Cannot extract transcript %s's sequence since the chromosome it locates, %s, is absent!\n", G.tr[i].transcript_id.c_str(),
                        G.tr[i].seqname.c_str());
        } else ids.push_back(i);
    }
    if (n_warns > 0) fprintf(stderr, "Warning: %d transcripts are failed to extract because their chromosome sequences are absent.\n", n_warns);
    if (verbose) printf("%d transcripts are extracted.\n", (int)ids.size());
    const int M = (int)ids.size();
    if (M <= 0) general_die("The reference contains no transcripts!");
    std::vector<int> starts;
    std::string curgid = "";
    for (int k = 0; k < M; k++)
        if (curgid != G.tr[ids[k]].gene_id) { starts.push_back(k + 1); curgid = G.tr[ids[k]].gene_id; }
    starts.push_back(M + 1);
    if (verbose) printf("Extracting sequences is done!\n");

    // writeResults (extractRef.cpp:256-290)
    const std::string ref = argv[1];
    write_numbers(ref + ".grp", starts);
    if (verbose) printf("Group File is generated!\n");
    write_ti(ref + ".ti", G.tr, ids, 0);
    if (verbose) printf("Transcript Information File is generated!\n");
    {
        OutFile o(ref + ".chrlist");
        for (const Chr& c : chrvec) o.put(c.name + "\t" + std::to_string(c.len) + "\n");
    }
    if (verbose) printf("Chromosome List File is generated!\n");
    {
        stages.device_begin();
        std::vector<uint8_t> store((size_t)off[M0 + 1]);
        refseq_try(rsem_refseq_download(h, 0, off[M0 + 1], store.data()), "rsem_refseq_download");
        stages.device_end();
        stages.write_begin();
        OutFile o(ref + ".transcripts.fa");
        for (int id : ids) {
            o.put(">" + G.tr[id].transcript_id + "\n");
            o.put(store.data() + off[id], (size_t)G.tr[id].length);
            o.put("\n", 1);
        }
        o.close();
        stages.write_end();
    }
    if (verbose) printf("Extracted Sequences File is generated!\n");
    stages.report("rsem-extract-reference-transcripts", h);
    rsem_refseq_destroy(h);
    return 0;
}
