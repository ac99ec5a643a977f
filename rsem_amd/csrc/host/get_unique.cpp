// rsem-get-unique on MI355X: same argv, same BAM (decompressed) and same stdout as the reference program (getUnique.cpp).
//
//   rsem-get-unique number_of_threads unsorted_transcript_bam_input bam_output [--device d]
//
// writes  bam_output: the input's header as read, and the records of every read that has exactly one alignment (one record, or the
//         two records of a pair) and no unmapped record, as they are.
//
// The reference groups, decides and writes on one thread (its threads only deflate); here the records' names and flags go to the
// GPU, which cuts the groups and says which records stay (rsem_alncheck_unique, rsem_amd/csrc/alncheck.hip), and the threads copy
// and deflate the kept records (host/alncheck_host.hpp).  CRAM input is refused.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "alncheck_host.hpp"

using namespace rsemh;

int main(int argc, char* argv[]) {
    AlncheckOptions opt;
    bool ok = argc >= 4;
    for (int i = 4; ok && i < argc; i++) {  // --device d is this program's own
        if (!strcmp(argv[i], "--device") && i + 1 < argc) opt.device = atoi(argv[++i]);
        else ok = false;
    }
    if (!ok) {
        printf("Usage: rsem-get-unique number_of_threads unsorted_transcript_bam_input bam_output\n");
        exit(-1);
    }
    opt.threads = std::max(1, atoi(argv[1]));
    write_unique(argv[2], argv[3], opt);
    return 0;
}
