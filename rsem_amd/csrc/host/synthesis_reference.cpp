// rsem-synthesis-reference-transcripts on MI355X: same argv, same files as the reference program (synthesisRef.cpp).
//
//   rsem-synthesis-reference-transcripts refName quiet hasMappingFile<0|1|2> [mappingFile] reference_file_1 [...] [--device d]
//
// writes  refName.ti, refName.grp, refName.transcripts.fa; with hasMappingFile 2 also refName.gt and refName.ta
//
// Every record is a transcript (1, its length) on '+'.  The records' bytes go to the GPU a batch at a time: the line ends are dropped,
// the letters checked and mapped (rsem_refseq_load), and every record's bases are copied to its place in one output store
// (rsem_refseq_gather), which is downloaded once.  name2seq of the reference is a map: a name that comes again keeps its LAST sequence.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "refprep_host.hpp"

using namespace rsemh;

int main(int argc, char* argv[]) {
    Stages stages;
    const int device = strip_device(argc, argv);
    int has_mapping = 0;
    if (argc < 5 || ((has_mapping = atoi(argv[3])) && argc < 6)) {
        printf("Usage: synthesisRef refName quiet hasMappingFile<0,no;1,yes;2,allele-specific> [mappingFile] reference_file_1 [reference_file_2 ...]\n");
        exit(-1);
    }
    const bool verbose = !atoi(argv[2]);
    if (has_mapping != 0 && has_mapping != 1 && has_mapping != 2) die("hasMappingFile must be 0, 1 or 2!");  // (the reference stops at an assert here)
    std::map<std::string, std::string> mi_table, mi_table2;
    if (has_mapping) load_mapping_info(has_mapping, argv[4], mi_table, mi_table2);
    const int start = has_mapping ? 5 : 4;

    // every record's place in the store: its raw body is an upper bound of its bases; places are multiples of 16
    std::vector<MappedFile> files((size_t)(argc - start));
    std::vector<std::vector<FastaRecord>> recs((size_t)(argc - start));
    std::vector<std::vector<uint64_t>> slot((size_t)(argc - start));
    uint64_t store_bytes = 0;
    // (a file that cannot be opened stops the reference when its turn comes, after the files before it went through: the same here)
    int n_open = 0;
    for (int i = start; i < argc; i++, n_open++) {
        if (!files[i - start].open(argv[i])) break;
        recs[i - start] = frame_fasta(files[i - start].data, files[i - start].size);
        for (const FastaRecord& r : recs[i - start]) { slot[i - start].push_back(store_bytes); store_bytes += (r.hi - r.lo + 15) & ~15ull; }
    }
    rsem_refseq* h = nullptr;
    refseq_try(rsem_refseq_create(&h, device, store_bytes), "rsem_refseq_create");

    std::vector<RefTranscript> tr(1);
    std::map<std::string, std::pair<uint64_t, uint64_t>> name2seq;  // name -> (place, bases) of its last record
    std::string seqname;
    int M = 0;
    for (int i = start; i < argc; i++) {
        const int fi = i - start;
        if (fi >= n_open) die("Cannot open %s! It may not exist.", argv[i]);
        const MappedFile& f = files[fi];
        std::vector<int64_t> s_src;
        std::vector<uint32_t> s_first, s_len, s_flags;
        std::vector<uint64_t> s_dst;
        stages.device_begin();
        load_file(h, RSEM_REFSEQ_CHECKED, f.data, recs[fi], nullptr,
                  [&](int64_t r, uint64_t n_bases, int64_t bad) {
                      const FastaRecord& R = recs[fi][r];
                      first_token(f.data + R.head_lo, f.data + R.head_hi, seqname);
                      if (bad >= 0) die_bad_character(argv[i], f.data, (uint64_t)bad);
                      if (n_bases == 0) die("FASTA file %s: the record %s has an empty sequence!", argv[i], seqname.c_str());  // (an assert in the reference)
                      name2seq[seqname] = {slot[fi][r], n_bases};
                      RefTranscript t;
                      t.transcript_id = t.gene_id = t.seqname = seqname;
                      if (has_mapping) {
                          auto it = mi_table.find(seqname);
                          if (it == mi_table.end()) general_die("Mapping Info is not correct, cannot find " + seqname + "'s gene_id!");
                          t.gene_id = it->second;
                          if (has_mapping == 2) {
                              auto it2 = mi_table2.find(seqname);
                              if (it2 == mi_table2.end()) general_die("Mapping Info is not correct, cannot find allele " + seqname + "'s transcript_id!");
                              t.transcript_id = it2->second;
                          }
                      }
                      t.strand = '+';
                      t.length = (int)n_bases;
                      t.structure.push_back({1, (int)n_bases});
                      tr.push_back(std::move(t));
                      ++M;
                      if (verbose && M % 1000000 == 0) printf("%d sequences are processed!\n", M);
                      s_src.push_back(r); s_first.push_back(0); s_len.push_back((uint32_t)n_bases); s_flags.push_back(0); s_dst.push_back(slot[fi][r]);
                  },
                  [&](int64_t, int64_t) {
                      refseq_try(rsem_refseq_gather(h, (int64_t)s_src.size(), s_src.data(), s_first.data(), s_len.data(), s_dst.data(), s_flags.data()), "rsem_refseq_gather");
                      s_src.clear(); s_first.clear(); s_len.clear(); s_flags.clear(); s_dst.clear();
                  });
        stages.device_end();
    }
    if (M < 1) {
        fprintf(stderr, "Number of transcripts in the reference is less than 1!\n");
        exit(-1);
    }
    // Transcripts::sort (Transcript.h:53-55), stable
    std::vector<int> ids((size_t)M);
    for (int k = 0; k < M; k++) ids[k] = k + 1;
    std::stable_sort(ids.begin(), ids.end(), [&](int a, int b) {
        if (tr[a].gene_id != tr[b].gene_id) return tr[a].gene_id < tr[b].gene_id;
        if (tr[a].transcript_id != tr[b].transcript_id) return tr[a].transcript_id < tr[b].transcript_id;
        return tr[a].seqname < tr[b].seqname;
    });

    // writeResults (synthesisRef.cpp:72-130)
    const std::string ref = argv[1];
    write_ti(ref + ".ti", tr, ids, has_mapping == 2 ? 2 : 1);
    if (verbose) printf("Transcript Information File is generated!\n");
    std::vector<int> gi, gt, ta;
    std::string cur_gene_id = "", cur_transcript_id = "";
    for (int k = 1; k <= M; k++) {
        const RefTranscript& t = tr[ids[k - 1]];
        if (cur_gene_id != t.gene_id) {
            gi.push_back(k);
            if (has_mapping == 2) gt.push_back((int)ta.size());
            cur_gene_id = t.gene_id;
        }
        if (has_mapping == 2 && cur_transcript_id != t.transcript_id) { ta.push_back(k); cur_transcript_id = t.transcript_id; }
    }
    gi.push_back(M + 1);
    if (has_mapping == 2) { gt.push_back((int)ta.size()); ta.push_back(M + 1); }
    write_numbers(ref + ".grp", gi);
    if (verbose) printf("Group File is generated!\n");
    if (has_mapping == 2) {
        write_numbers(ref + ".gt", gt);
        write_numbers(ref + ".ta", ta);
        if (verbose) printf("Allele-specific group files are generated!\n");
    }
    {
        stages.device_begin();
        std::vector<uint8_t> store((size_t)store_bytes);
        refseq_try(rsem_refseq_download(h, 0, store_bytes, store.data()), "rsem_refseq_download");
        stages.device_end();
        stages.write_begin();
        OutFile o(ref + ".transcripts.fa");
        for (int k = 0; k < M; k++) {
            const std::string& name = tr[ids[k]].seqname;
            const auto& ps = name2seq[name];
            o.put(">" + name + "\n");
            o.put(store.data() + ps.first, (size_t)ps.second);
            o.put("\n", 1);
        }
        o.close();
        stages.write_end();
    }
    if (verbose) printf("Extracted Sequences File is generated!\n");
    stages.report("rsem-synthesis-reference-transcripts", h);
    rsem_refseq_destroy(h);
    return 0;
}
