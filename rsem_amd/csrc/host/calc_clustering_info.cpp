// rsem-for-ebseq-calculate-clustering-info on MI355X: same argv, same file as the reference program
// (EBSeq/calcClusteringInfo.cpp:92-144).
//
//   rsem-for-ebseq-calculate-clustering-info k input_reference_fasta_file output_file     + [--device d] [-q]
//
// reads   the FASTA file (host/fasta_codes.hpp: the reference's reader, letter for letter)
// writes  output_file: for every entry, in input order, name <TAB> value with "%.6g": -1 where the entry is shorter than k,
//         otherwise (k-mer start positions whose k-mer also occurs in another entry) / (len - k + 1).
//
// The reference lists every (entry, position), sorts the list on one thread with a comparator that walks two strings and counts;
// here the k-mers are sorted and counted on the GPU (rsem_kmer_shared_counts, rsem_amd/csrc/kmer.hip).  The count is an integer
// and the division is the reference's: the file is the reference's byte for byte.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/rsem_hip.h"
#include "fasta_codes.hpp"
#include "files.hpp"

using namespace rsemh;

namespace {

void usage() {
    printf("Usage: rsem-for-ebseq-calculate-clustering-info k input_reference_fasta_file output_file [--device d] [-q]\n");
    exit(-1);
}

}  // namespace

int main(int argc, char* argv[]) {
    if (argc < 4) usage();
    int device = 0;
    bool quiet = false;
    for (int i = 4; i < argc; i++) {
        if (!strcmp(argv[i], "-q")) quiet = true;
        else if (!strcmp(argv[i], "--device") && i + 1 < argc) device = atoi(argv[++i]);
        else usage();
    }
    const bool verbose = !quiet;
    const int k = atoi(argv[1]);  // calcClusteringInfo.cpp:98
    if (k < 1) die("rsem-for-ebseq-calculate-clustering-info: k = '%s': the k-mer size must be at least 1!", argv[1]);

    const auto t0 = std::chrono::steady_clock::now();
    FastaCodes fa;
    if (!read_fasta_codes(argv[2], fa)) die("Cannot open %s! It may not exist.", argv[2]);
    const int M = fa.M();
    if (verbose) printf("The reference is loaded.\n");

    std::vector<uint32_t> shared((size_t)M + 1, 0);
    rsem_kmer_info info;
    memset(&info, 0, sizeof(info));
    if (M > 0) {
        int ndev = 0;
        rsem_hip_device_count(&ndev);
        if (ndev < 1) die("rsem-for-ebseq-calculate-clustering-info: no usable GPU (this program has no CPU path)");
        if (device < 0 || device >= ndev) die("--device %d: only %d device(s) present", device, ndev);
        const int rc = rsem_kmer_shared_counts(device, M, fa.seq_off.data(), fa.codes.data(), k, shared.data(), &info);
        if (rc != RSEM_OK) die("rsem-for-ebseq-calculate-clustering-info: %s: %s", rsem_hip_strerror(rc), rsem_hip_last_error());
    }
    if (verbose) {
        printf("All %llu %d-mers are sorted: %llu distinct, %d batch(es), %d sort(s) each.\n", (unsigned long long)info.n_kmers, k,
               (unsigned long long)info.n_groups, info.n_batches, info.n_chunks);
        printf("[device] upload %.1f ms, kernels %.1f ms, %.1f MB of batch buffers\n", info.upload_ms, info.kernel_ms, (double)info.batch_bytes / 1e6);
    }

    FILE* fo = fopen(argv[3], "w");
    if (!fo) die("Cannot open %s for writing!", argv[3]);
    std::string out;
    char tmp[48];
    for (int i = 0; i < M; i++) {  // calcClusteringInfo.cpp:132-140
        const uint64_t len = fa.seq_off[i + 1] - fa.seq_off[i];
        const double v = len < (uint64_t)k ? -1.0 : (double)shared[i] / (double)(len - (uint64_t)k + 1);
        out.append(fa.names[i]);
        out.push_back('\t');
        out.append(tmp, (size_t)snprintf(tmp, sizeof(tmp), "%.6g", v));
        out.push_back('\n');
        if (out.size() >= (1u << 20)) { fwrite(out.data(), 1, out.size(), fo); out.clear(); }
    }
    fwrite(out.data(), 1, out.size(), fo);
    if (fclose(fo) != 0) die("Cannot write %s!", argv[3]);
    if (verbose) {
        printf("Clustering information is calculated.\n");
        printf("[host] %.2f s in all\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    }
    return 0;
}
