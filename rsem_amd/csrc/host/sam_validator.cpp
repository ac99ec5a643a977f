// rsem-sam-validator on MI355X: same argv, same stdout, same exit status as the reference program (samValidator.cpp).
//
//   rsem-sam-validator <input.sam/input.bam> [-p number_of_threads] [--device d]
//
// prints  ".", one "." per million reads counted, then what the reference says about the first read it would stop at followed by
//         "The input file is not valid!", or "The input file is valid!"; exit status 0 either way.
//
// The reference checks record by record on one thread and keeps every read name in a std::set<std::string>; here the records become
// fields on the -p threads and the checks -- the set included, as sorted runs of hashes with the names' bytes behind them -- run on
// the GPU (rsem_alncheck_push, rsem_amd/csrc/alncheck.hip; host/alncheck_host.hpp).  A file that cannot be framed ends the program
// with a message of its own (the reference says "not valid" and nothing else).  CRAM input is refused.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "alncheck_host.hpp"

using namespace rsemh;

int main(int argc, char* argv[]) {
    AlncheckOptions opt;
    bool ok = argc >= 2;
    for (int i = 2; ok && i < argc; i++) {  // -p N and --device d are this program's own
        if (!strcmp(argv[i], "-p") && i + 1 < argc) opt.threads = std::max(1, atoi(argv[++i]));
        else if (!strcmp(argv[i], "--device") && i + 1 < argc) opt.device = atoi(argv[++i]);
        else ok = false;
    }
    if (!ok) {
        printf("Usage: rsem-sam-validator <input.sam/input.bam/input.cram>\n");
        exit(-1);
    }
    validate_alignments(argv[1], opt);
    return 0;
}
