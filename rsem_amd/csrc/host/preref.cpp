// rsem-preref on MI355X: same argv, same files as the reference program (preRef.cpp, Refs.h:83-114, RefSeq.h, PolyARules.h).
//
//   rsem-preref refFastaF polyAChoice refName [-l polyALen] [-f exceptionF] [-q] [--device d]
//
// writes  refName.seq, refName.idx.fa, refName.n2g.idx.fa
//
// The entries' bytes go to the GPU a batch at a time, unchecked: the line ends are dropped (rsem_refseq_load, raw mode) and every
// entry is written twice into one output store, upper-cased with N for anything but A, C, G, T and with its poly-A tail, and the same
// with every N as G (rsem_refseq_gather), which is downloaded once.  Tags, lengths and mask words are written on the host.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "refprep_host.hpp"

using namespace rsemh;

int main(int argc, char* argv[]) {
    if (argc < 4) {
        printf("USAGE : rsem-preref refFastaF polyAChoice refName [-l polyALen] [-f exceptionF] [-q]\n\n");
        printf("  refFastaF: a FASTA format file contains all reference transcripts\n");
        printf("  polyAChoice: choice for polyA tail padding.It is a number from {0,1,2}\n");
        printf("    0: pad polyA tail\n");
        printf("    1: do not pad polyA tail at all\n");
        printf("    2: pad polyA tail for all references but those in exceptionF\n");
        printf("  -l: polyALen: specify the length of polyA tail you want to pad. Default is 100\n");
        printf("  -f: exceptionF: file contains a list of exception reference ids. IDs starts from 1. Must set if polyAChoice = 2\n");
        printf("  -q: quiet\n");
        exit(-1);
    }
    Stages stages;
    const int choice = atoi(argv[2]);
    int poly_a = 125, device = 0;
    bool quiet = false;
    std::string exception_f;
    for (int i = 4; i < argc; i++) {
        const bool more = i + 1 < argc;
        if (!strcmp(argv[i], "-l") && more) poly_a = atoi(argv[i + 1]);
        if (!strcmp(argv[i], "-f") && more) exception_f = argv[i + 1];
        if (!strcmp(argv[i], "-q")) quiet = true;
        if (!strcmp(argv[i], "--device") && more) device = atoi(argv[i + 1]);
    }
    const bool verbose = !quiet;
    if (choice < 0 || choice > 2) die("polyAChoice must be 0, 1 or 2!");  // (the reference stops at an assert at the first entry)
    if (poly_a < 0) die("polyALen must not be negative!");                 // (likewise)
    std::set<std::string> exceptions;  // PolyARules.h:24-41
    if (choice == 2) {
        MappedFile e;
        if (!e.open(exception_f)) die("Cannot open %s! It may not exist.", exception_f.c_str());
        std::string tok;
        for (const char *p = e.data, *end = e.data + e.size; first_token(p, end, tok, &p);) exceptions.insert(tok);
    }

    MappedFile f;
    if (!f.open(argv[1])) die("Cannot open %s! It may not exist.", argv[1]);
    const std::vector<FastaRecord> recs = frame_fasta(f.data, f.size);
    const size_t n = recs.size();
    // an entry's two places in the store, from what its raw body and its tail can take at most; the second image lies behind the first
    std::vector<uint64_t> slot(n + 1, 0);
    std::vector<int> tail(n);
    for (size_t r = 0; r < n; r++) {
        const std::string tag(f.data + recs[r].head_lo, f.data + recs[r].head_hi);
        tail[r] = choice == 0 ? poly_a : choice == 1 ? 0 : (exceptions.count(tag) ? 0 : poly_a);  // PolyARules::getLenAt
        slot[r + 1] = slot[r] + ((recs[r].hi - recs[r].lo + (uint64_t)tail[r] + 15) & ~15ull);
    }
    const uint64_t image = slot[n];
    rsem_refseq* h = nullptr;
    refseq_try(rsem_refseq_create(&h, device, 2 * image), "rsem_refseq_create");
    std::vector<uint64_t> full(n, 0);
    std::vector<int64_t> s_src;
    std::vector<uint32_t> s_first, s_len, s_flags;
    std::vector<uint64_t> s_dst;
    stages.device_begin();
    load_file(h, RSEM_REFSEQ_RAW, f.data, recs, nullptr,
              [&](int64_t r, uint64_t n_bases, int64_t) {
                  full[r] = n_bases;
                  if (n_bases == 0) {  // Refs.h:103-106
                      fprintf(stderr, "Warning: Fasta entry %.*s has an empty sequence! It is omitted!\n", (int)(recs[r].head_hi - recs[r].head_lo), f.data + recs[r].head_lo);
                      return;
                  }
                  if (n_bases + (uint64_t)tail[r] > 0x7fffffffull) die("Fasta entry %lld: %llu bases with its tail (2^31 - 1 at most)", (long long)r + 1, (unsigned long long)(n_bases + tail[r]));
              },
              [&](int64_t first, int64_t last) {
                  for (int img = 0; img < 2; img++) {  // a gather an image: the destinations of one call ascend
                      for (int64_t r = first; r < last; r++) {
                          if (!full[r]) continue;
                          const uint32_t fl = RSEM_REFSEQ_UPPER_N | (img ? RSEM_REFSEQ_N2G : 0u);
                          s_src.push_back(r); s_first.push_back(0); s_len.push_back((uint32_t)full[r]); s_flags.push_back(fl); s_dst.push_back(img * image + slot[r]);
                          if (tail[r]) {
                              s_src.push_back(r); s_first.push_back(0); s_len.push_back((uint32_t)tail[r]); s_flags.push_back(RSEM_REFSEQ_FILL);
                              s_dst.push_back(img * image + slot[r] + full[r]);
                          }
                      }
                      refseq_try(rsem_refseq_gather(h, (int64_t)s_src.size(), s_src.data(), s_first.data(), s_len.data(), s_dst.data(), s_flags.data()), "rsem_refseq_gather");
                      s_src.clear(); s_first.clear(); s_len.clear(); s_flags.clear(); s_dst.clear();
                  }
              });
    if (verbose) printf("Refs.makeRefs finished!\n");

    std::vector<uint8_t> store((size_t)(2 * image));
    refseq_try(rsem_refseq_download(h, 0, 2 * image, store.data()), "rsem_refseq_download");
    stages.device_end();
    stages.write_begin();
    const std::string ref = argv[3];
    {  // Refs::saveRefs, RefSeq::write (RefSeq.h:130-138); the masks: RefSeq.h:32-37
        OutFile o(ref + ".seq");
        std::string s;
        for (size_t r = 0; r < n; r++) {
            if (!full[r]) continue;
            const int full_len = (int)full[r], tot_len = full_len + tail[r];
            o.put(std::to_string(full_len) + " " + std::to_string(tot_len) + "\n");
            o.put(f.data + recs[r].head_lo, (size_t)(recs[r].head_hi - recs[r].head_lo));
            o.put("\n", 1);
            o.put(store.data() + slot[r], (size_t)tot_len);
            o.put("\n", 1);
            std::vector<unsigned int> fmasks((size_t)((full_len - 1) / 32 + 1), 0u);
            if (tail[r] > 0)
                for (int i = std::max(full_len - kOLen + 1, 0); i < full_len; i++) fmasks[i / 32] |= 1u << (i % 32);
            s.clear();
            for (size_t k = 0; k < fmasks.size(); k++) s += std::to_string(fmasks[k]) + (k + 1 < fmasks.size() ? " " : "\n");
            o.put(s);
        }
    }
    if (verbose) printf("Refs.saveRefs finished!\n");
    for (int img = 0; img < 2; img++) {
        const std::string path = ref + (img ? ".n2g.idx.fa" : ".idx.fa");
        {
            OutFile o(path);
            for (size_t r = 0; r < n; r++) {
                if (!full[r]) continue;
                o.put(">", 1);
                o.put(f.data + recs[r].head_lo, (size_t)(recs[r].head_hi - recs[r].head_lo));
                o.put("\n", 1);
                o.put(store.data() + img * image + slot[r], (size_t)(full[r] + tail[r]));
                o.put("\n", 1);
            }
        }
        if (verbose) printf("%s is generated!\n", path.c_str());
    }
    stages.write_end();
    stages.report("rsem-preref", h);
    rsem_refseq_destroy(h);
    return 0;
}
