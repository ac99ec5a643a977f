// rsem-bam2readdepth on MI355X: same argv, same file as the reference program (bam2readdepth.cpp:11-27, wiggle.cpp:39-83,127-139),
// which rsem-plot-transcript-wiggles calls.
//
//   rsem-bam2readdepth sorted_bam_input readdepth_output [-p N] [--device d] [-q]
//
// reads   the alignments (SAM text or BAM; host/depth_host.hpp), every one weighted by its ZW tag
// writes  readdepth_output: for every run of records of one reference sequence name <TAB> length <TAB> the depth of every base as
//         `ostream << double` prints it, blanks between; behind them the sequences no record used, with NA.
//
// The sums are made on the GPU in the records' order (rsem_depth_accumulate, rsem_amd/csrc/depth.hip): the reference's doubles.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "depth_host.hpp"

using namespace rsemh;

int main(int argc, char* argv[]) {
    DepthOptions opt;
    if (argc < 3 || !parse_depth_options(argc, argv, 3, opt)) {
        printf("Usage: rsem-bam2readdepth sorted_bam_input readdepth_output\n");
        exit(-1);
    }
    FILE* fo = fopen(argv[2], "w");
    if (!fo) die("Cannot write to %s!", argv[2]);
    ReadDepthWriter writer;
    build_depth(argv[1], opt, writer, fo, argv[2]);
    if (fclose(fo) != 0) die("Cannot write %s!", argv[2]);
    return 0;
}
