// rsem-tbam2gbam on MI355X: same argv, same genome BAM (decompressed) as the reference program (tbam2gbam.cpp:16-35, BamConverter.h).
//
//   rsem-tbam2gbam reference_name unsorted_transcript_bam_input genome_bam_output [-p number_of_threads] [--device d] [-q]
//
// reads   reference_name.ti (type 0: built from a genome), reference_name.chrlist, the transcript alignments (SAM text or BAM)
// writes  genome_bam_output: every mapped record on its chromosome with an M / N CIGAR, a read's alignments that land on one locus
//         merged with their weights added, in the order of the reference's std::map; unmapped reads as they are.
//
// The reference converts, collapses and writes on one thread; here the records become fields on the -p threads, the coordinate
// map and the per-read sort-and-merge run on the GPU (rsem_gmap_convert, rsem_amd/csrc/gmap.hip), and the -p threads put the
// output records together and deflate them (host/gbam_host.hpp).
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "gbam_host.hpp"

using namespace rsemh;

int main(int argc, char* argv[]) {
    GbamOptions opt;
    bool ok = argc >= 4;
    for (int i = 4; ok && i < argc; i++) {  // -p N as the reference takes it; --device d and -q are this program's own
        if (!strcmp(argv[i], "-q")) opt.quiet = true;
        else if (!strcmp(argv[i], "-p") && i + 1 < argc) opt.threads = std::max(1, atoi(argv[++i]));
        else if (!strcmp(argv[i], "--device") && i + 1 < argc) opt.device = atoi(argv[++i]);
        else ok = false;
    }
    if (!ok) {
        printf("Usage: rsem-tbam2gbam reference_name unsorted_transcript_bam_input genome_bam_output [-p number_of_threads]\n");
        exit(-1);
    }
    std::string command = argv[0];  // assemble_command (utils.h:159-164)
    for (int i = 1; i < argc; i++) command += " " + std::string(argv[i]);
    convert_transcript_bam(argv[1], argv[2], argv[3], opt, command);
    return 0;
}
