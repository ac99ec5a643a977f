// rsem-scan-for-paired-end-reads on MI355X: same argv, same BAM (decompressed), same stdout, stderr and exit status as the reference
// program (scanForPairedEndReads.cpp), which convert-sam-for-rsem runs between `samtools sort -n` and rsem-sam-validator.
//
//   rsem-scan-for-paired-end-reads number_of_threads input.[sam/bam] output.bam [--device d]
//
// writes  output.bam: the input's header as read and every record as it is; the records of a paired-end read -- which a name-sorted
//         file holds in any order -- so that the two mates of an alignment are adjacent: the properly paired records sorted by
//         (reference, smaller and larger of pos and mate pos, strand pattern), then first and second mates that are not, in turns.
//
// The reference groups, sorts and writes on one thread (its threads only deflate); here the records' names, flags and positions go to
// the GPU, which cuts the groups and says where every record goes (rsem_pairscan_reorder, rsem_amd/csrc/pairscan.hip), and the
// threads gather and deflate (host/pairscan_host.hpp).  Records that tie in the sort keep their order in the file (the reference
// leaves that order to std::sort: INTEGRATION.md).  CRAM input is refused.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "pairscan_host.hpp"

using namespace rsemh;

int main(int argc, char* argv[]) {
    AlncheckOptions opt;
    bool ok = argc >= 4;
    for (int i = 4; ok && i < argc; i++) {  // --device d is this program's own
        if (!strcmp(argv[i], "--device") && i + 1 < argc) opt.device = atoi(argv[++i]);
        else ok = false;
    }
    if (!ok) {
        printf("Usage: rsem-scan-for-paired-end-reads number_of_threads input.[sam/bam/cram] output.bam\n");
        exit(-1);
    }
    opt.threads = std::max(1, atoi(argv[1]));
    scan_for_paired_end_reads(argv[2], argv[3], opt);
    return 0;
}
