// depth_check.cpp -- TEST INFRASTRUCTURE: rsem-bam2wig and rsem-bam2readdepth without a device.  The programs' own host code
// (rsem_amd/csrc/host/depth_host.hpp: reader, records -> blocks, runs, hand-over, writers) runs unchanged; the entry point it
// calls, rsem_depth_accumulate, is defined HERE and walks the same steps as rsem_amd/csrc/depth.hip with the same functions of
// rsem_amd/csrc/depth_block.hpp: batches, entries in block order, a stable sort on the tile, the touched tiles, and for every one of
// them accumulate_tile -- the kernel's body -- on tests/simt_emu.hpp (one OS thread per lane, "LDS" in memory, the barrier a barrier).
// Built with AddressSanitizer and UBSan (tests/test_depth_cpu.py).  Never part of the product.
//
//   depth_check wig <alignments> <out> <track name> [--no-fractional-weight]
//   depth_check readdepth <alignments> <out>
//   depth_check fold <n_bases> < "start len weight-bits-as-hex" lines      prints the depth's bits, one base a line
//   depth_check tilebits <n_tiles> ...                                     prints tile_bits of every number
// Build: hipcc (host compilation of the HIP headers simt_emu.hpp pulls in) -DRSEM_EMU -fsanitize=address,undefined -fno-gpu-sanitize
#include "simt_emu.hpp"

#include "../rsem_amd/csrc/depth_block.hpp"
#include "../rsem_amd/csrc/host/depth_host.hpp"

using namespace rsem_depth;

namespace {

struct Job {
    emu::Block blk;
    TileEntry stage[kChunk];  // "LDS"
    uint64_t tile;
    uint32_t e0, ne;
    const uint32_t* blk_of;
    const uint64_t* start;
    const uint32_t* len;
    const double* w;
    double* depth;
    uint64_t n_bases;
};

void lane_body(Job* J, int tid) {
    emu::t_tid = tid;
    emu::t_blk = &J->blk;
    accumulate_tile(J->tile, J->e0, J->ne, J->blk_of, J->start, J->len, J->w, J->depth, J->n_bases, J->stage);
}

std::string g_error;

}  // namespace

extern "C" const char* rsem_hip_strerror(int) { return "error"; }
extern "C" const char* rsem_hip_last_error(void) { return g_error.c_str(); }

extern "C" int rsem_depth_accumulate(int, uint64_t n_bases, uint64_t n_blocks, const uint64_t* start, const uint32_t* len, const double* w, double* depth,
                                     rsem_depth_info* info) {
    static_assert(kTileThreads == 256 && RSEM_BDIM == 256, "the emulator's workgroup is the kernel's");
    for (uint64_t i = 0; i < n_blocks; i++) {
        uint64_t end;
        if (__builtin_add_overflow(start[i], (uint64_t)len[i], &end) || end > n_bases) { g_error = "a block runs past the bases"; return RSEM_ERR_INVALID; }
    }
    uint64_t budget = kDefaultBatchItems;
    if (const char* e = getenv("RSEM_DEPTH_BATCH_ITEMS")) budget = (uint64_t)atoll(e);
    if (info) { memset(info, 0, sizeof(*info)); info->batch_items = budget; }
    if (!n_blocks || !n_bases) return RSEM_OK;
    Job* J = new Job();
    const int bits = tile_bits((n_bases + kTile - 1) / kTile);  // depth.hip: the radix sort's end_bit
    const uint32_t key_mask = bits >= 32 ? 0xffffffffu : (1u << bits) - 1u;
    pthread_barrier_init(&J->blk.bar, nullptr, 256);
    for (int k = 0; k < 4; k++) pthread_barrier_init(&J->blk.w[k].bar, nullptr, 64);
    for (uint64_t lo = 0; lo < n_blocks;) {
        uint64_t items, entries;
        const uint64_t hi = batch_end(start, len, n_blocks, lo, budget, items, entries);
        // k_count, the scan and k_expand: one entry per (block, tile) pair, in block order
        std::vector<std::pair<uint32_t, uint32_t>> ent;
        for (uint64_t b = lo; b < hi; b++)
            for (uint64_t t = 0; t < tiles_of(start[b], len[b]); t++) ent.push_back({(uint32_t)(first_tile(start[b]) + t), (uint32_t)(b - lo)});
        if (ent.size() != entries) { g_error = "batch_end counts other entries than tiles_of"; return RSEM_ERR_STATE; }
        // on the tile ALONE, and like the radix sort on no more of its bits than tile_bits names
        std::stable_sort(ent.begin(), ent.end(), [key_mask](const auto& a, const auto& b) { return (a.first & key_mask) < (b.first & key_mask); });
        std::vector<uint32_t> blk_of(ent.size());
        for (size_t i = 0; i < ent.size(); i++) blk_of[i] = ent[i].second;
        for (size_t i = 0; i < ent.size();) {  // the run-length encoding of the tiles; one workgroup each
            size_t j = i;
            while (j < ent.size() && ent[j].first == ent[i].first) j++;
            // a tile is ONE run, one workgroup: two of a launch would both write its bases
            if (i > 0 && ent[i].first <= ent[i - 1].first) { g_error = "the sorted tiles do not ascend"; return RSEM_ERR_STATE; }
            J->tile = ent[i].first; J->e0 = (uint32_t)i; J->ne = (uint32_t)(j - i);
            J->blk_of = blk_of.data(); J->start = start + lo; J->len = len + lo; J->w = w + lo; J->depth = depth; J->n_bases = n_bases;
            std::vector<std::thread> th;
            for (int t = 0; t < 256; t++) th.emplace_back(lane_body, J, t);
            for (auto& t : th) t.join();
            if (info) info->n_tiles_touched++;
            i = j;
        }
        if (info) { info->n_entries += entries; info->n_batches++; }
        lo = hi;
    }
    delete J;
    return RSEM_OK;
}

int main(int argc, char* argv[]) {
    using namespace rsemh;
    if (argc >= 3 && !strcmp(argv[1], "fold")) {
        const uint64_t n_bases = strtoull(argv[2], nullptr, 10);
        std::vector<uint64_t> start;
        std::vector<uint32_t> len;
        std::vector<double> w, depth(n_bases, 0.0);
        unsigned long long s, l, bits;
        while (scanf("%llu %llu %llx", &s, &l, &bits) == 3) {
            double x;
            memcpy(&x, &bits, 8);
            start.push_back(s); len.push_back((uint32_t)l); w.push_back(x);
        }
        rsem_depth_info info;
        if (rsem_depth_accumulate(0, n_bases, start.size(), start.data(), len.data(), w.data(), depth.data(), &info) != RSEM_OK) {
            fprintf(stderr, "%s\n", g_error.c_str());
            return 2;
        }
        for (double d : depth) {
            memcpy(&bits, &d, 8);
            printf("%016llx\n", bits);
        }
        fprintf(stderr, "batches %d entries %llu tiles %llu\n", info.n_batches, (unsigned long long)info.n_entries, (unsigned long long)info.n_tiles_touched);
        return 0;
    }
    if (argc >= 3 && !strcmp(argv[1], "tilebits")) {
        for (int i = 2; i < argc; i++) printf("%d\n", tile_bits(strtoull(argv[i], nullptr, 10)));
        return 0;
    }
    DepthOptions opt;
    opt.quiet = true;
    opt.threads = 3;
    if (argc >= 5 && !strcmp(argv[1], "wig")) {
        opt.no_fractional_weight = argc == 6 && !strcmp(argv[5], "--no-fractional-weight");
        FILE* fo = fopen(argv[3], "w");
        if (!fo) return 2;
        const std::string head = WigWriter::header(argv[4]);
        fwrite(head.data(), 1, head.size(), fo);
        WigWriter wr;
        build_depth(argv[2], opt, wr, fo, argv[3]);
        return fclose(fo) ? 2 : 0;
    }
    if (argc == 4 && !strcmp(argv[1], "readdepth")) {
        FILE* fo = fopen(argv[3], "w");
        if (!fo) return 2;
        ReadDepthWriter wr;
        build_depth(argv[2], opt, wr, fo, argv[3]);
        return fclose(fo) ? 2 : 0;
    }
    fprintf(stderr, "usage: depth_check wig|readdepth|fold ...\n");
    return 2;
}
